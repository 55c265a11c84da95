"""BS.1770 loudness as csrc/pce_lufs.hip computes it, restated stage by stage in numpy with ``np.longdouble`` (64-bit significand where the host has it)
as the high-precision type, with a bound for every stage counted from the kernels' own operations.  tests/test_lufs_host.py holds the restatement
against the oracle and a float64 emulation of the kernels (``emulate``) against the bounds; tests/test_gpu_lufs_stages.py holds what
``ProsodyEngine.lufs_fetch_stages`` copies out against the same bounds.

All stages take ``x = float64(raw) / float64(peak)`` as given: the same IEEE division as the kernel's, so x is exact.

Bounds.  U = 1.001 x 2^-53: one rounding of a float64 result r is at most 2^-53 |r|; the 0.1 % covers the second-order terms (magnitudes are taken from the
long-double values, which differ from the device's by the error being bounded), the long double's own roundings (2^-11 of a float64's) and the double
rounding of the emulated fma.

  * Cascade.  The error of the four states obeys d' = A d + eta with A the zero-input transition matrix and eta the local roundings of one sample
    (every product, sum and difference of lu_run adds U of its magnitude; the rounding of y reaches the states through |a1|, |a2|, |c0|, |c1|, |c2| and
    that of u through |d1|, |d2|).  Hence |d_n| <= sum_k |A^(n-k)| eta_k <= G sum_k eta_k with G the entrywise maximum of |A^m| over the m that can occur
    (0 .. 256 inside a chunk; every m for the whole slice).  Letting earlier error pass through the absolute values of the COEFFICIENTS instead would not
    give a usable bound: |A| has a spectral radius of about 2.4 (both biquads have |a1| near 2), so that recursion grows by 2.4 per sample.
  * Power table.  transition_powers forms P_L = A P_(L-1) with four products and three sums per entry: E_L = A E_(L-1) + eta_L,
    |eta_L| <= 4 U |A| |P_(L-1)| + |dA| |P_(L-1)| (dA: the two roundings in each of A's two composed entries), so |E_L| <= sum_k |A^(L-k)| |eta_k|.
  * lu_matvec: two fmas, one product, one fma and one sum per row, five roundings of partial sums none of which exceeds sum_j |m_rj| |s_j| + |e_r|:
    5 U (|m| |s| + |e|).  The 4 x 4 product of level 1 has the same five roundings per entry: 5 U |A| |M|.
  * Scan.  Inside a group state_init[c + 1] is one lu_matvec of the device's own state_init[c], state_end[c] and table entry.  The first chunk of a group
    (and of a 1024-chunk block: the value the level-2 chain leaves after lane 63 is what lane 0 takes in the next round, the same expression) is
    lu_matvec(M_g, s, z_g) of the previous group's begin state s, with M_g and z_g folded over the group's chunks in float64: their errors obey the same
    recursion as above through the following chunks' table entries, which are powers of A to 1e-13, so |dz| <= G sum_k 5 U (|A_k| |z_k| + |e_k|) and
    |dM| <= G sum_k 5 U |A_k| |M_k|; the step's bound is |dM| |s| + |dz| + 5 U (|M_g| |s| + |z_g|).
  * Whole slice.  Step k of the scan adds xi_k = E_len |s_k| + pass 1's local errors of state_end[k] + the scan bound of the step to the begin state's
    error, which then decays with the filter: |d_c| <= sum_(k<c) H(distance) xi_k, H(d) the entrywise supremum of |A^m| over m >= d (``envelope``,
    ``propagate``); pass 2 starts from there (``cascade(..., e0=)``).
  * Gate.  z is float64 sums and one product in chunk order: reproduced bit for bit.  The means: a lane adds ceil(n_blocks / 64) - 1 times, the butterfly
    six times, one division, all of positive numbers: (ceil(n_blocks / 64) + 6) U relative, 10 / ln 10 of that in LU; then the device's log10
    (EPS_LOG10 ulps of its result), the product by 10 and the sum with -0.691, one rounding each."""
import math

import numpy as np

LD = np.longdouble
U = 1.001 * 2.0 ** -53
LMAX, GROUP, WAVE = 256, 16, 64                  # LU_LMAX, LU_GROUP of csrc/pce_lufs.hip; the wavefront
T_G, STEP, GAMMA_A = 0.400, 1.0 - 0.75, -70.0
OK, TOO_SHORT, EMPTY = 0, 1, 2
# The device's log10 against the long double's, in ulps of the result, measured over the cases of tests/test_gpu_lufs_stages.py (its docstring has the
# figure), times four for inputs they did not see.
EPS_LOG10_MEASURED = 1.56
EPS_LOG10 = 4.0 * EPS_LOG10_MEASURED


# ------------------------------------------------------------------------------------------------------------------ plan
def plan(ns, rate):
    """The chunk and block tables of one slice of ``ns`` samples under a meter of ``rate``: pyloudnorm's block count and bounds in float64 exactly as
    oracle.lufs_numpy forms them; the points sorted and made unique, pieces of at most 256 samples, bounds clamped to the slice."""
    ns = int(ns)
    if ns == 0:
        return dict(status=EMPTY, rel=np.zeros(0, np.int64), len=np.zeros(0, np.int32), c0=np.zeros(0, np.int32), c1=np.zeros(0, np.int32), lo=[], up=[])
    if ns < T_G * rate:
        return dict(status=TOO_SHORT, rel=np.zeros(0, np.int64), len=np.zeros(0, np.int32), c0=np.zeros(0, np.int32), c1=np.zeros(0, np.int32), lo=[], up=[])
    T = ns / rate
    nb = int(np.round(((T - T_G) / (T_G * STEP))) + 1)
    lo, up = [], []
    for j in range(nb):
        l = min(int(T_G * (j * STEP) * rate), ns); u = min(int(T_G * (j * STEP + 1) * rate), ns)
        lo.append(l); up.append(max(u, l))
    pts = sorted(set([0] + lo + up))
    rel, ln, at = [], [], {}
    for p, q in zip(pts, pts[1:]):
        at[p] = len(rel)
        for a in range(p, q, LMAX):
            rel.append(a); ln.append(min(LMAX, q - a))
    at[pts[-1]] = len(rel)
    return dict(status=OK, rel=np.array(rel, np.int64), len=np.array(ln, np.int32), c0=np.array([at[l] for l in lo], np.int32),
                c1=np.array([at[u] for u in up], np.int32), lo=lo, up=up)


def slice_samples(clip, begin, end):
    """int64 samples of ``[begin, end)`` in clip coordinates, zeros outside the clip."""
    out = np.zeros(end - begin, np.int64)
    a, b = max(begin, 0), min(end, len(clip))
    if b > a:
        out[a - begin:b - begin] = clip[a:b]
    return out


def peak_of(raw):
    p = int(np.abs(raw).max()) if len(raw) else 0
    return p or 1


# ------------------------------------------------------------------------------------------------------------------ the transition matrix and its powers
def transition_matrix(coef, dtype=np.float64):
    """As transition_powers builds it (state order z0, z1, w0, w1), in ``dtype`` arithmetic."""
    k = np.asarray(coef, np.float64).astype(dtype)
    a1, a2, c0, c1, c2, d1, d2 = k[4], k[5], k[6], k[7], k[8], k[10], k[11]
    A = np.zeros((4, 4), dtype)
    A[0, 0] = -a1; A[0, 1] = 1; A[1, 0] = -a2
    A[2, 0] = c1 - d1 * c0; A[2, 2] = -d1; A[2, 3] = 1
    A[3, 0] = c2 - d2 * c0; A[3, 2] = -d2
    return A


def powers_float64(coef, n=LMAX):
    """transition_powers' own arithmetic: s = 0; s += A[r][t] * prev[t][q] for t = 0 .. 3, in float64."""
    A = transition_matrix(coef)
    pw = np.zeros((n + 1, 4, 4)); pw[0] = np.eye(4)
    for L in range(1, n + 1):
        p = pw[L - 1]
        pw[L] = ((A[:, 0:1] * p[0:1] + A[:, 1:2] * p[1:2]) + A[:, 2:3] * p[2:3]) + A[:, 3:4] * p[3:4]
    return pw


def powers_ld(coef, n=LMAX):
    A = transition_matrix(coef, LD)
    pw = np.zeros((n + 1, 4, 4), LD); pw[0] = np.eye(4)
    for L in range(1, n + 1):
        pw[L] = A @ pw[L - 1]
    return pw


def table_bound(coef, n=LMAX):
    """-> (the long-double powers, the entrywise bound on what transition_powers' float64 table may be off them)."""
    P = powers_ld(coef, n)
    absP = np.abs(P)
    Aabs = np.abs(transition_matrix(coef, LD))
    dA = np.zeros((4, 4), LD)
    k = np.asarray(coef, np.float64).astype(LD)
    dA[2, 0] = U * (abs(k[10] * k[6]) + abs(k[7] - k[10] * k[6])); dA[3, 0] = U * (abs(k[11] * k[6]) + abs(k[8] - k[11] * k[6]))
    eta = np.zeros((n + 1, 4, 4), LD)
    for L in range(1, n + 1):
        eta[L] = 4 * U * (Aabs @ absP[L - 1]) + dA @ absP[L - 1]
    E = np.zeros((n + 1, 4, 4), LD)
    for L in range(1, n + 1):
        E[L] = np.einsum("kij,kjl->il", absP[L - 1::-1][:L], eta[1:L + 1])
    return P, E.astype(np.float64)


def growth(coef, upto=None):
    """G: the entrywise maximum of |A^m| over m = 0 .. ``upto`` (None: over every m; the powers are followed until they have decayed below 1e-9 of G)."""
    A = transition_matrix(coef, LD)
    P = np.eye(4, dtype=LD); G = np.abs(P)
    m = 0
    while True:
        P = A @ P; m += 1
        G = np.maximum(G, np.abs(P))
        if upto is not None:
            if m >= upto:
                break
        elif m > 1000 and np.all(np.abs(P) < 1e-9 * np.maximum(G, 1e-300)):
            break
        assert m < 4_000_000, "the cascade does not decay"
    return G


HGRID = 32


def envelope(coef):
    """H[j]: the entrywise supremum of |A^m| over m >= 32 j, followed until the powers have decayed below 1e-9 of their maximum (the last entry stands for
    every later m)."""
    A = transition_matrix(coef, LD)
    P = np.eye(4, dtype=LD); rows = [np.abs(P)]; G = np.abs(P)
    m = 0
    while True:
        P = A @ P; m += 1
        rows.append(np.abs(P)); G = np.maximum(G, rows[-1])
        if m % HGRID == 0 and m > 1000 and np.all(rows[-1] < 1e-9 * np.maximum(G, 1e-300)):
            break
        assert m < 4_000_000, "the cascade does not decay"
    a = np.array(rows, LD)
    sup = np.maximum.accumulate(a[::-1], 0)[::-1]
    return sup[::HGRID].astype(np.float64) * 1.001


def propagate(H, rel, ln, xi):
    """The bound on the begin states' error: d_c <= sum_(k<c) sup_(m >= distance) |A^m| xi_k, distance = rel[c] - (rel[k] + len[k])."""
    n = len(rel)
    out = np.zeros((n, 4))
    end = np.asarray(rel, np.int64) + np.asarray(ln, np.int64)
    for a in range(0, n, 128):
        c = np.arange(a, min(a + 128, n))
        d = np.asarray(rel, np.int64)[c][:, None] - end[None, :]
        live = np.arange(n)[None, :] < c[:, None]
        Hs = H[np.clip(d // HGRID, 0, len(H) - 1)] * live[:, :, None, None]
        out[c] = np.einsum("ckij,kj->ci", Hs, xi)
    return out


# ------------------------------------------------------------------------------------------------------------------ the cascade
def chunk_matrix(x, rel, ln, width=LMAX):
    """x [ns] -> [n_chunks, width], row c = x[rel[c] : rel[c] + len[c]], zero filled."""
    idx = np.asarray(rel, np.int64)[:, None] + np.arange(width)[None, :]
    live = np.arange(width)[None, :] < np.asarray(ln)[:, None]
    return np.where(live, np.asarray(x)[np.minimum(idx, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)


def cascade(coef, xm, lens, s0=None, e0=None, G=None, keep_u2=False):
    """Every row of ``xm`` (float64 [n, L], ``lens`` live samples each) through lu_run in long double from begin states ``s0`` [n, 4] (default zero), one
    numpy step per sample position.  ``e0`` [n, 4]: a bound on the error the begin states already carry (default none).
    -> dict(state LD [n, 4], energy LD [n], state_bound [n, 4], energy_bound [n], u2 LD [n, L] if asked)."""
    n, L = xm.shape
    k = np.asarray(coef, np.float64).astype(LD)
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = k[0], k[1], k[2], k[4], k[5], k[6], k[7], k[8], k[10], k[11]
    G = growth(coef, LMAX) if G is None else G
    GT = np.asarray(G, LD).T
    s0 = np.zeros((n, 4), LD) if s0 is None else np.asarray(s0).astype(LD)
    z0, z1, w0, w1 = (s0[:, t].copy() for t in range(4))
    S = np.zeros((n, 4), LD) if e0 is None else np.asarray(e0).astype(LD).copy()
    acc = np.zeros(n, LD); eacc = np.zeros(n, LD)
    u2 = np.zeros((n, L), LD) if keep_u2 else None
    lens = np.asarray(lens)
    ab = abs
    for p in range(L):
        act = p < lens
        if not act.any():
            break
        x = xm[:, p].astype(LD)
        t = b0 * x; y = t + z0; ey = U * (ab(t) + ab(y))
        p1 = b1 * x; p2 = a1 * y; dd = p1 - p2; nz0 = dd + z1
        l0 = U * (ab(p1) + ab(p2) + ab(dd) + ab(nz0)) + ab(a1) * ey
        q1 = b2 * x; q2 = a2 * y; nz1 = q1 - q2
        l1 = U * (ab(q1) + ab(q2) + ab(nz1)) + ab(a2) * ey
        t2 = c0 * y; u = t2 + w0; eu = ab(c0) * ey + U * (ab(t2) + ab(u))
        r1 = c1 * y; r2 = d1 * u; rr = r1 - r2; nw0 = rr + w1
        l2 = U * (ab(r1) + ab(r2) + ab(rr) + ab(nw0)) + ab(c1) * ey + ab(d1) * eu
        v1 = c2 * y; v2 = d2 * u; nw1 = v1 - v2
        l3 = U * (ab(v1) + ab(v2) + ab(nw1)) + ab(c2) * ey + ab(d2) * eu
        est = S @ GT                                              # the states' error at this sample
        du = ab(c0) * est[:, 0] + est[:, 2] + eu
        sq = u * u; nacc = acc + sq
        neacc = eacc + 2 * ab(u) * du + du * du + U * (sq + nacc)
        z0 = np.where(act, nz0, z0); z1 = np.where(act, nz1, z1); w0 = np.where(act, nw0, w0); w1 = np.where(act, nw1, w1)
        acc = np.where(act, nacc, acc); eacc = np.where(act, neacc, eacc)
        S += np.where(act[:, None], np.stack([l0, l1, l2, l3], 1), 0)
        if keep_u2:
            u2[:, p] = np.where(act, sq, 0)
    out = dict(state=np.stack([z0, z1, w0, w1], 1), energy=acc, state_bound=(S @ GT).astype(np.float64), energy_bound=eacc.astype(np.float64),
               local=S.astype(np.float64))
    if keep_u2:
        out["u2"] = u2
    return out


ROW = 250     # the piece length of ``sequential``: no multiple of a chunk, so that its borders are not the device's


def sequential(coef, x, row=ROW):
    """The cascade over the whole of ``x`` in long double -> u^2 of every sample (LD [ns]).  The recurrence is run over pieces of ``row`` samples at once:
    each from a zero state, the true begin states chained through A^row in long double, then again from those (the filter is linear; both orders carry
    long-double roundings only, 2^-11 of what the float64 bounds allow: tests/test_lufs_host.py compares this with a sample-by-sample loop)."""
    ns = len(x)
    if ns == 0:
        return np.zeros(0, LD)
    nr = -(-ns // row)
    rel = np.arange(nr, dtype=np.int64) * row
    ln = np.minimum(row, ns - rel)
    xm = chunk_matrix(x, rel, ln, row)
    G = np.zeros((4, 4))
    zs = cascade(coef, xm, ln, G=G)["state"]
    Ar = powers_ld(coef, row)[row]
    s = np.zeros((nr, 4), LD)
    for r in range(1, nr):
        s[r] = Ar @ s[r - 1] + zs[r - 1]
    u2 = cascade(coef, xm, ln, s0=s, G=G, keep_u2=True)["u2"]
    return u2.reshape(-1)[:ns] if nr * row == ns else np.concatenate([u2[:-1].reshape(-1), u2[-1, :ln[-1]]])


def sequential_plain(coef, x):
    """The same sample by sample (a scalar loop: short inputs only)."""
    k = np.asarray(coef, np.float64).astype(LD)
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = k[0], k[1], k[2], k[4], k[5], k[6], k[7], k[8], k[10], k[11]
    z0 = z1 = w0 = w1 = LD(0)
    out = np.zeros(len(x), LD)
    for i, v in enumerate(np.asarray(x, np.float64).astype(LD)):
        y = b0 * v + z0; z0 = b1 * v - a1 * y + z1; z1 = b2 * v - a2 * y
        u = c0 * y + w0; w0 = c1 * y - d1 * u + w1; w1 = c2 * y - d2 * u
        out[i] = u * u
    return out


# ------------------------------------------------------------------------------------------------------------------ the scan
def _rowsum(m, s, e):
    return np.abs(m) @ np.abs(s) + np.abs(e)


def scan_check(apow, ln, state_init, state_end, Ginf):
    """Every step of k_lufs_scan for one slice from the device's own values -> dict of the worst |got - want| / bound per kind of step (None where the
    slice has no such step) and ``bound`` [n_chunks, 4], the bound of the step INTO every chunk (0 for chunk 0)."""
    n = len(ln)
    A = np.asarray(apow, np.float64).astype(LD)
    si = np.asarray(state_init, np.float64).astype(LD); se = np.asarray(state_end, np.float64).astype(LD)
    worst = {"inside": None, "group": None, "carry": None}
    bound = np.zeros((n, 4))
    Ginf = 1.001 * np.asarray(Ginf, LD)       # of the true powers; the table's entries are those to 1e-13
    for c in range(1, n):
        if c % GROUP:
            m = A[ln[c - 1]]
            want = m @ si[c - 1] + se[c - 1]
            b = 5 * U * _rowsum(m, si[c - 1], se[c - 1])
            kind = "inside"
        else:
            g0 = c - GROUP
            s = si[g0].copy(); z = np.zeros(4, LD); M = np.eye(4, dtype=LD)
            lz = np.zeros(4, LD); lM = np.zeros((4, 4), LD)
            for q in range(g0, c):
                m = A[ln[q]]
                lz += 5 * U * _rowsum(m, z, se[q]); lM += 5 * U * (np.abs(m) @ np.abs(M))
                z = m @ z + se[q]; M = m @ M
                s = m @ s + se[q]
            want = s
            b = (Ginf @ lM) @ np.abs(si[g0]) + Ginf @ lz + 5 * U * _rowsum(M, si[g0], z)
            kind = "carry" if c % (GROUP * WAVE) == 0 else "group"
        bound[c] = b.astype(np.float64)
        err = np.abs(si[c] - want)
        r = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))))
        worst[kind] = r if worst[kind] is None else max(worst[kind], r)
    return worst, bound


# ------------------------------------------------------------------------------------------------------------------ the gate
def block_z(energy, c0, c1, inv_norm):
    """k_lufs_gate's z: the chunk energies of [c0, c1) added in chunk order in float64, times inv_norm.  Bit for bit."""
    energy = np.asarray(energy, np.float64)
    c0 = np.asarray(c0, np.int64); c1 = np.asarray(c1, np.int64)
    e = np.zeros(len(c0))
    for k in range(int((c1 - c0).max()) if len(c0) else 0):
        live = c0 + k < c1
        e = np.where(live, e + energy[np.minimum(c0 + k, len(energy) - 1)], e)
    return np.float64(inv_norm) * e


def level_ld(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return LD(-0.691) + LD(10) * np.log10(np.asarray(z).astype(LD))


def level_allowance(nb):
    """How far the device's float64 level of a block, or of the first gate's mean, can lie from the long double's, in LU: the mean's roundings, the log10,
    the product and the sum (levels between -200 and +10 LU)."""
    return float(10 / math.log(10) * (-(-nb // WAVE) + 6) * U + (EPS_LOG10 * 2.0 ** -52 * 20 * 10) + U * 200 + U * 200)


def gate_ld(z):
    """The two gates decided in long double from given z -> dict(set1, set2 (bool arrays), margin (the least distance of a level from a threshold it is
    compared with, LU), lufs (LD; -inf for an empty second set))."""
    z = np.asarray(z)
    l = level_ld(z)
    s1 = l >= GAMMA_A
    margin = float(np.min(np.abs(l[np.isfinite(l)] - GAMMA_A))) if np.isfinite(l).any() else np.inf
    if not s1.any():
        return dict(set1=s1, set2=s1.copy(), margin=margin, lufs=LD(-np.inf), gamma_r=LD(np.nan))
    gr = level_ld(z[s1].astype(LD).mean()) - 10
    fin = np.isfinite(l)
    if fin.any():
        margin = min(margin, float(np.min(np.abs(l[fin] - gr))))
    s2 = (l > gr) & (l > GAMMA_A)
    lufs = level_ld(z[s2].astype(LD).mean()) if s2.any() else LD(-np.inf)
    return dict(set1=s1, set2=s2, margin=margin, lufs=lufs, gamma_r=gr)


def lufs_bound(nb, lufs):
    """|device - long double| of the final value: the derived part (lane sums, butterfly, division) and the log10 part."""
    v = abs(float(lufs)) + 0.691
    derived = 10 / math.log(10) * (-(-nb // WAVE) + 6) * U
    return derived + EPS_LOG10 * 10 * _ulp(v / 10) + U * v + U * abs(float(lufs))


def _ulp(v):
    return float(np.spacing(np.float64(abs(v)))) if v else 2.0 ** -1074


def wave_mean(z, sel):
    """k_lufs_gate's mean of z[sel] bit for bit: lane j adds blocks j, j + 64, ... in order, the butterfly adds lane ^ 32, 16, .. 1, one division."""
    z = np.asarray(z, np.float64); sel = np.asarray(sel, bool)
    s = np.zeros(WAVE); cnt = np.zeros(WAVE)
    for j in range(len(z)):
        if sel[j]:
            s[j % WAVE] = s[j % WAVE] + z[j]; cnt[j % WAVE] += 1.0
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off:
        s = s + s[lane ^ off]; cnt = cnt + cnt[lane ^ off]
        off >>= 1
    return (s[0] / cnt[0]) if cnt[0] > 0 else None


def gate_float64(z):
    """pyloudnorm's gating in its own float64 arithmetic, as oracle.lufs_numpy has it (what "on the threshold" means is defined here only)."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = [-0.691 + 10.0 * np.log10(v) for v in z]
        J = [j for j, lj in enumerate(l) if lj >= GAMMA_A]
        zavg = np.mean([z[j] for j in J]) if J else np.nan
        gr = -0.691 + 10.0 * np.log10(zavg) - 10.0
        J = [j for j, lj in enumerate(l) if (lj > gr and lj > GAMMA_A)]
        zavg = np.mean([z[j] for j in J]) if J else 0.0
        return float(-0.691 + 10.0 * np.log10(zavg))


# ------------------------------------------------------------------------------------------------------------------ one slice, every stage
def _ratio(err, bound):
    err = np.asarray(err, np.float64); bound = np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


class Tables:
    """What depends on the coefficients only: computed once per meter rate."""

    def __init__(self, coef):
        self.coef = np.asarray(coef, np.float64).copy()
        self.P, self.E = table_bound(coef)
        self.G256 = growth(coef, LMAX)
        self.Ginf = growth(coef)
        self.H = envelope(coef)

    def table_ratio(self, apow):
        return _ratio(np.abs(np.asarray(apow, np.float64).astype(LD) - self.P).astype(np.float64)[1:], self.E[1:])


def check_slice(tab, rate, x, st, lufs):
    """Every stage of one live slice.  ``x``: float64 [ns], raw / peak.  ``st``: what the device (or ``emulate``) left for it: dict of ``apow`` [257, 4, 4],
    ``rel``, ``len``, ``state_end`` [n, 4], ``state_init`` [n, 4], ``energy`` [n], ``c0``, ``c1``, ``z``.  ``lufs``: the final value.
    -> dict(ratios: the worst |got - want| / bound per stage (None: no such element), tables_equal, tiles, covers, z_equal, margin, sets_equal, counts)."""
    pl = plan(len(x), rate)
    rel, ln = np.asarray(st["rel"]), np.asarray(st["len"])
    c0, c1 = np.asarray(st["c0"]), np.asarray(st["c1"])
    out = {"tables_equal": all(np.array_equal(np.asarray(st[k]), pl[k]) for k in ("rel", "len", "c0", "c1"))}
    last = max(pl["up"]) if pl["up"] else 0
    out["tiles"] = bool(len(rel) and rel[0] == 0 and np.array_equal(rel[1:], (rel + ln)[:-1]) and rel[-1] + ln[-1] == last and ln.min() >= 1 and ln.max() <= LMAX)
    n = len(rel)
    ok = lambda c: 0 <= c <= n
    out["covers"] = all(ok(a) and ok(b) and a <= b and (rel[a] if a < n else last) == l and (rel[b] if b < n else last) == u
                        for a, b, l, u in zip(c0, c1, pl["lo"], pl["up"]))
    if not (out["tables_equal"] and out["tiles"] and out["covers"]):
        return out
    coef = tab.coef
    xm = chunk_matrix(x, rel, ln)
    se = np.asarray(st["state_end"], np.float64); si = np.asarray(st["state_init"], np.float64); en = np.asarray(st["energy"], np.float64)
    rat = {}
    p1 = cascade(coef, xm, ln, G=tab.G256)
    rat["pass1"] = _ratio(np.abs(se.astype(LD) - p1["state"]).astype(np.float64), p1["state_bound"])
    worst, sbound = scan_check(st["apow"], ln, si, se, tab.Ginf)
    rat["scan_inside"], rat["scan_group"], rat["scan_carry"] = worst["inside"], worst["group"], worst["carry"]
    out["init0_zero"] = bool(np.all(si[0] == 0.0))
    p2 = cascade(coef, xm, ln, s0=si, G=tab.G256)
    rat["pass2"] = _ratio(np.abs(en.astype(LD) - p2["energy"]).astype(np.float64), p2["energy_bound"])
    # whole slice, against the filter run over pieces that are not the device's
    u2 = sequential(coef, x)
    cs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    want_en = np.array([u2[rel[c]:rel[c] + ln[c]].sum() for c in range(n)], LD)
    xi = (tab.E[ln] @ np.abs(si)[:, :, None])[:, :, 0] + p1["local"] + np.concatenate([sbound[1:], np.zeros((1, 4))])
    e0 = propagate(tab.H, rel, ln, xi)
    out["state_bound_max"] = float(e0.max())
    pw = cascade(coef, xm, ln, s0=si, e0=e0, G=tab.G256)
    rat["chunk"] = _ratio(np.abs(en.astype(LD) - want_en).astype(np.float64), pw["energy_bound"])
    blk_got = np.array([en[a:b].astype(LD).sum() for a, b in zip(c0, c1)], LD)
    blk_want = np.array([u2[l:u].sum() for l, u in zip(pl["lo"], pl["up"])], LD)
    blk_bound = np.array([pw["energy_bound"][a:b].sum() for a, b in zip(c0, c1)])
    rat["block"] = _ratio(np.abs(blk_got - blk_want).astype(np.float64), blk_bound)
    out["block_rel"] = float(np.max(np.abs(blk_got - blk_want) / np.where(blk_want > 0, blk_want, 1))) if len(blk_want) else 0.0
    # gate
    z = np.asarray(st["z"], np.float64)
    out["z_equal"] = bool(np.array_equal(z, block_z(en, c0, c1, coef[12])))
    g = gate_ld(z)
    out["margin"] = g["margin"]; out["n_set1"] = int(g["set1"].sum()); out["n_set2"] = int(g["set2"].sum())
    out["absolute_dropped"] = int((~g["set1"]).sum()); out["relative_dropped"] = int((g["set1"] & ~g["set2"]).sum())
    want = float(g["lufs"])
    if np.isinf(want):
        out["lufs_equal_inf"] = bool(lufs == want)
        rat["lufs"] = None if lufs == want else np.inf
    else:
        rat["lufs"] = abs(float(LD(lufs) - g["lufs"])) / lufs_bound(len(z), want)
        m = wave_mean(z, g["set2"])
        # the device's log10 alone: its mean is reproduced bit for bit, so what is left of the difference is log10, the product and the sum
        out["log10_ulps"] = abs(float(LD(lufs) - level_ld(m))) / (10 * _ulp(math.log10(m))) if m and m > 0 else 0.0
    out["ratios"] = rat
    out["n_chunks"] = n; out["n_blocks"] = len(z); out["min_len"] = int(ln.min())
    return out


# ------------------------------------------------------------------------------------------------------------------ the kernels' arithmetic in float64
def _fma(a, b, c):
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def _matvec(m, s, e):
    """lu_matvec."""
    return _fma(m[:, 1], s[1], _fma(m[:, 0], s[0], e)) + _fma(m[:, 3], s[3], m[:, 2] * s[2])


def _matmul(A, M):
    """The 4 x 4 product of level 1."""
    return _fma(A[:, 1:2], M[1:2, :], A[:, 0:1] * M[0:1, :]) + _fma(A[:, 3:4], M[3:4, :], A[:, 2:3] * M[2:3, :])


def _run64(coef, xm, lens, s0, drop_last_of=None):
    k = np.asarray(coef, np.float64)
    n, L = xm.shape
    z0, z1, w0, w1 = (np.array(s0[:, t], np.float64) for t in range(4))
    acc = np.zeros(n)
    lens = np.asarray(lens).copy()
    if drop_last_of is not None:
        lens[drop_last_of] -= 1
    for p in range(L):
        act = p < lens
        x = xm[:, p]
        y = k[0] * x + z0
        nz0 = k[1] * x - k[4] * y + z1
        nz1 = k[2] * x - k[5] * y
        u = k[6] * y + w0
        nw0 = k[7] * y - k[10] * u + w1
        nw1 = k[8] * y - k[11] * u
        z0 = np.where(act, nz0, z0); z1 = np.where(act, nz1, z1); w0 = np.where(act, nw0, w0); w1 = np.where(act, nw1, w1)
        acc = np.where(act, acc + u * u, acc)
    return np.stack([z0, z1, w0, w1], 1), acc


MUTATIONS = ("border_sample", "clip_mask", "group_zero", "carry_dropped", "table_entry", "block_plus_one", "gate_strict")


def emulate_gate(z, mutation=None):
    """k_lufs_gate's two passes in float64 (numpy's log10 for the device's)."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        s1 = (l > GAMMA_A) if mutation == "gate_strict" else (l >= GAMMA_A)
        m1 = wave_mean(z, s1)
        gr = -0.691 + 10.0 * np.log10(np.float64(np.nan if m1 is None else m1)) - 10.0
        s2 = (l > gr) & (l > GAMMA_A)
        m2 = wave_mean(z, s2)
        return float(-0.691 + 10.0 * np.log10(np.float64(0.0 if m2 is None else m2)))


def emulate(coef, rate, pcm, clip_lo, clip_hi, begin, end, mutation=None):
    """The four kernels on one slice in float64, operation for operation (the fmas of the scan through the long double).  ``pcm``: the resident
    buffer (int16); the slice is [begin, end) of it in the buffer's coordinates (may leave it), its clip [clip_lo, clip_hi).  ``mutation``: one of
    MUTATIONS.  -> (stages dict as check_slice takes it, lufs, peak)."""
    ns = end - begin
    pl = plan(ns, rate)
    rel, ln, c0, c1 = pl["rel"], pl["len"], pl["c0"], pl["c1"]
    n = len(rel)
    g = begin + np.arange(ns)
    inside = (g >= 0) & (g < len(pcm))
    raw = np.where(inside, np.asarray(pcm, np.int64)[np.clip(g, 0, len(pcm) - 1)], 0)
    real = (g >= clip_lo) & (g < clip_hi)
    peak = peak_of(raw[real])
    if mutation == "clip_mask":
        real = (g >= clip_lo) & (g < clip_hi + 1)
    x = np.where(real, raw, 0).astype(np.float64) / np.float64(peak)
    xm = chunk_matrix(x, rel, ln)
    drop = n // 2 if mutation == "border_sample" else None
    apow = powers_float64(coef)
    if mutation == "table_entry":
        apow[200] = apow[199]
    se, _ = _run64(coef, xm, ln, np.zeros((n, 4)), drop)
    si = np.zeros((n, 4))
    carry = np.zeros(4)
    for g0 in range(0, -(-n // GROUP), WAVE):
        groups = range(g0, min(g0 + WAVE, -(-n // GROUP)))
        zg, Mg = {}, {}
        for gi in groups:
            z = np.zeros(4); M = np.eye(4)
            for c in range(gi * GROUP, min(gi * GROUP + GROUP, n)):
                A = apow[ln[c]]
                z = _matvec(A, z, se[c]); M = _matmul(A, M)
            zg[gi], Mg[gi] = z, M
        if mutation == "carry_dropped" and g0 > 0:
            carry = np.zeros(4)
        begin_of = {}
        for gi in groups:
            begin_of[gi] = carry.copy()
            carry = _matvec(Mg[gi], carry, zg[gi])
        for gi in groups:
            b = begin_of[gi]
            if mutation == "group_zero" and gi == 3:
                b = np.zeros(4)
            for c in range(gi * GROUP, min(gi * GROUP + GROUP, n)):
                si[c] = b
                b = _matvec(apow[ln[c]], b, se[c])
    _, en = _run64(coef, xm, ln, si, drop)
    z = block_z(en, c0, c1 + 1 if mutation == "block_plus_one" else c1, coef[12]) if n else np.zeros(0)
    lufs = emulate_gate(z, mutation)
    return dict(apow=apow, rel=rel, len=ln, state_end=se, state_init=si, energy=en, c0=c0, c1=c1, z=z), lufs, peak


def kweight_float64(rate):
    """The 13 numbers of LuCoef as kweight_design forms them (pyloudnorm's design, float64)."""
    G, Q, fc = 4.0, 1 / np.sqrt(2), 1500.0
    A = 10 ** (G / 40.0); w0 = 2.0 * np.pi * (fc / rate); alpha = np.sin(w0) / (2.0 * Q)
    b0 = A * ((A + 1) + (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha)
    b1 = -2 * A * ((A - 1) + (A + 1) * np.cos(w0))
    b2 = A * ((A + 1) + (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha)
    a0 = (A + 1) - (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha
    a1 = 2 * ((A - 1) - (A + 1) * np.cos(w0))
    a2 = (A + 1) - (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha
    k = [b0 / a0, b1 / a0, b2 / a0, a0 / a0, a1 / a0, a2 / a0]
    Q, fc = 0.5, 38.0
    w0 = 2.0 * np.pi * (fc / rate); alpha = np.sin(w0) / (2.0 * Q)
    b0 = (1 + np.cos(w0)) / 2; b1 = -(1 + np.cos(w0)); b2 = (1 + np.cos(w0)) / 2
    a0 = 1 + alpha; a1 = -2 * np.cos(w0); a2 = 1 - alpha
    k += [b0 / a0, b1 / a0, b2 / a0, a0 / a0, a1 / a0, a2 / a0, 1.0 / (0.400 * rate)]
    return np.array(k, np.float64)


def lufs_restated(samples, rate):
    """peak-normalise -> K-weighting -> blocks -> gates -> LUFS in long double from float64 coefficients (raises ValueError where pyloudnorm does)."""
    raw = np.asarray(samples, np.float64)
    pl = plan(len(raw), rate)
    if pl["status"] != OK:
        raise ValueError("Audio must have length greater than the block size.")
    x = raw / (np.abs(raw).max() or 1.0)
    coef = kweight_float64(rate)
    u2 = sequential(coef, x)
    z = np.array([LD(coef[12]) * u2[l:u].sum() for l, u in zip(pl["lo"], pl["up"])], LD)
    return float(gate_ld(z)["lufs"]), z
