"""Pitch_pathFinder in plain float64, as oracle/pce_oracle.c states it, on given candidates -- the reference of tests/test_pitch_path_host.py and of
stage B and the chain of tests/test_gpu_pitch_stages.py.

``path_finder`` takes one slice: candidates [T, K] (slot 0 the voiceless one, the first ``ncand[t]`` slots of a row count), the frame intensities,
the frame step and the five costs and thresholds.  It accumulates over the whole slice (no restart behind a frame with one candidate), forms the
octave-jump term as ``|log(f1 / f2) * log2e|`` and lets the first maximum win.  The recurrence runs frame by frame, each frame's K x K values in one
numpy expression; everything that does not depend on the recurrence is computed for all frames at once.

Besides the track it returns the *gap* of every arg-max it took: the best value minus the best value of a candidate that is not a twin of the
winner.  Twins are candidates of one frame to which any correct implementation gives bit-identical values whatever it rounds: all candidates with
f == 0 or f > ceiling (the same local term, the same transition class), and duplicates with equal f and s bits.  Among twins the first index wins
everywhere, so only the distance to the best non-twin says how much rounding a decision can take.
"""
import numpy as np

LOG2E = 1.4426950408889634073599246810018921374266


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def path_finder(cand_f, cand_s, ncand, intensity, dt, params, ceiling=None):
    """-> dict: ``f0``, ``strength`` [T]; ``psi`` int [T, K] (0 in frame 0 and in slots >= ncand); ``gap`` [T, K]: the gap of the arg-max behind
    psi[t, c] (+inf in frame 0, in slots >= ncand and where every predecessor is a twin of the winner); ``end_gap``: the same for the choice in the
    last frame; ``min_gap`` over both; ``max_abs_delta``: the largest |accumulated delta|; ``delta`` [T, K].  ``ceiling`` overrides
    ``params.pitch_ceiling`` (the analysis clamps it to the Nyquist frequency)."""
    f = np.array(cand_f, dtype=np.float64); s = np.array(cand_s, dtype=np.float64)
    n = np.asarray(ncand, dtype=np.int64); inten = np.asarray(intensity, dtype=np.float64)
    T = len(n)
    K = max(int(n.max()), 1)
    f = f[:, :K]; s = s[:, :K]
    valid = np.arange(K)[None, :] < n[:, None]
    f[~valid] = 0.0; s[~valid] = 0.0
    f[:, 0] = 0.0; s[:, 0] = 0.0                                          # the voiceless candidate
    ceiling = float(params.pitch_ceiling if ceiling is None else ceiling)
    vt, sil, oc = float(params.voicing_threshold), float(params.silence_threshold), float(params.octave_cost)
    corr = 0.01 / dt
    ojc, vuc = float(params.octave_jump_cost) * corr, float(params.voiced_unvoiced_cost) * corr
    uv = np.zeros(T) if sil <= 0.0 else 2.0 - inten / (sil / (1.0 + vt))
    uv = vt + np.where(uv > 0.0, uv, 0.0)
    vl_local = (f == 0.0) | (f > ceiling)
    vl_trans = (f <= 0.0) | (f >= ceiling)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(vl_local, uv[:, None], s - oc * (np.log(ceiling / f) * LOG2E))
        d[~valid] = 0.0
        # transition costs [T - 1, K (previous), K (current)]; +inf from a slot the previous frame does not have
        f1 = f[:-1, :, None]; f2 = f[1:, None, :]
        v1 = vl_trans[:-1, :, None]; v2 = vl_trans[1:, None, :]
        tc = np.where(v1 & v2, 0.0, np.where(v1 | v2, vuc, ojc * np.abs(np.log(f1 / f2) * LOG2E)))
    tc = np.where(valid[:-1, :, None], tc, np.inf)
    D = np.zeros((T, K)); psi = np.zeros((T, K), dtype=np.int64)
    D[0] = d[0]
    ar = np.arange(K)
    for t in range(1, T):
        v = (D[t - 1][:, None] - tc[t - 1]) + d[t][None, :]
        p = v.argmax(axis=0)                                              # first maximum
        psi[t] = p; D[t] = v[p, ar]
    D[~valid] = 0.0; psi[~valid] = 0
    # the gaps, from the same values recomputed for all frames at once (the same operations on the same operands: the same bits)
    fb, sb = _bits(f), _bits(s)
    gap = np.full((T, K), np.inf)
    if T > 1:
        V = (D[:-1, :, None] - tc) + d[1:, None, :]
        best = np.take_along_axis(V, psi[1:, None, :], axis=1)[:, 0, :]
        wf = np.take_along_axis(fb[:-1], psi[1:], axis=1); ws = np.take_along_axis(sb[:-1], psi[1:], axis=1)
        wv = np.take_along_axis(vl_local[:-1], psi[1:], axis=1)
        twin = ((fb[:-1, :, None] == wf[:, None, :]) & (sb[:-1, :, None] == ws[:, None, :])) | (vl_local[:-1, :, None] & wv[:, None, :])
        other = np.where(twin, -np.inf, V).max(axis=1)
        gap[1:] = np.where(valid[1:], best - other, np.inf)
    last = np.where(valid[T - 1], D[T - 1], -np.inf)
    place = int(last.argmax())
    twin = ((fb[T - 1] == fb[T - 1, place]) & (sb[T - 1] == sb[T - 1, place])) | (vl_local[T - 1] & vl_local[T - 1, place])
    end_gap = float(last[place] - np.where(twin, -np.inf, last).max())
    f0 = np.zeros(T); st = np.zeros(T)
    for t in range(T - 1, -1, -1):
        f0[t] = f[t, place]; st[t] = s[t, place]
        place = int(psi[t, place])
    return dict(f0=f0, strength=st, psi=psi, gap=gap, end_gap=end_gap, min_gap=float(min(gap.min(), end_gap)),
                max_abs_delta=float(np.abs(D[valid]).max()), delta=D)


def gap_bound(n_frames, max_abs_delta):
    """What a decision's gap must exceed for two correct float64 implementations to agree on it: B = 8 (L + 8) u M, u = 2^-53.  Along a slice of
    L frames each side rounds twice per frame (the subtraction of the transition cost, the addition of the local term), each by at most u M with M
    the largest accumulated value: 2 L u M per side.  The transition cost itself differs by a few ulp of a logarithm between log2 f1 - log2 f2
    and log2(f1 / f2) (the + 8, generously: |log2 f| < 10 and the costs are below 1, against M >= 0.45).  Both sides: 4 (L + 8) u M, and a
    factor of two."""
    return 8.0 * (n_frames + 8) * 2.0 ** -53 * max_abs_delta
