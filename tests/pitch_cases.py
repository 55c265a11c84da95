"""Inputs of the Praat pitch stage tests (tests/test_pitch_path_host.py, tests/test_gpu_pitch_stages.py): the clip sets of stage A, one per
instantiation of k_pitch_frames, with the CPU oracle's candidates computed once per process, and the builders of stage B's injected candidates.
Everything here runs on the CPU."""
import functools
import os
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 16                                                                    # row width of the candidate arrays of the two hooks (PI_MAXC)

# id -> (rate, floor, max_candidates, the k_pitch_frames form the plan selects, N = nsampFFT).  The form and N are labels here: that the plan
# selects them for the (rate, floor) pair is checked by the table in instantiations() of tests/host/pitch_plan_main.cpp (tests/test_pitch_plan_host.py),
# which holds a row for each pair below -- a pair added here needs its row there.
FORMS = {
    "16k-150": (16000, 150.0, 15, "<4,2,true>", 512),
    "16k-75": (16000, 75.0, 15, "<4,1,false>", 1024),
    "8k-150": (8000, 150.0, 15, "<4,0,false>", 256),
    "8k-75": (8000, 75.0, 15, "<4,2,true>", 512),                          # two frames per wavefront, both through the rare path
    "44k1-150": (44100, 150.0, 15, "<4,3,false>", 2048),
    "44k1-75": (44100, 75.0, 15, "<2,0,false>", 4096),
    "48k-50": (48000, 50.0, 15, "<1,0,false>", 8192),
    "16k-150-c16": (16000, 150.0, 16, "<4,2,true>", 512),                  # max_candidates = 16: lane 15 holds a candidate
}
CEILING = 600.0


def params(form_id):
    rate, floor, maxc, _, _ = FORMS[form_id]
    p = O.praat_params(floor, CEILING)
    p.max_candidates = maxc
    return p


@functools.lru_cache(maxsize=None)
def _c1():
    return np.load(os.path.join(GOLDEN, "c1_segment_ph9_16k.npz"))["pcm"][:32000].copy()          # C1, first 2 s


@functools.lru_cache(maxsize=None)
def _demo():
    z = np.load(os.path.join(GOLDEN, "demo_excerpts.npz"))
    rate = int(z["rate"])
    assert rate == 44100
    return z["segment_ph2"][: int(1.2 * rate)].copy()


def mixture(speech, rate, seed):
    """0.5 x speech under two high tones, one of them beating at 3 Hz: many local maxima of comparable height (3000 and 2300 Hz at 8 kHz, scaled
    with the rate), plus noise of a few LSB."""
    t = np.arange(len(speech)) / rate
    k = rate / 8000.0
    rng = np.random.default_rng(seed)
    x = (0.5 * speech.astype(np.float64) + 2000.0 * np.sin(2 * np.pi * 3000.0 * k * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
         + 1000.0 * np.sin(2 * np.pi * 2300.0 * k * t) + 3.0 * rng.standard_normal(len(t)))
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def periodic(rate, period, seconds=0.5, tail=0.15):
    """A harmonic complex whose period is a whole number of samples, exactly periodic in int16: the autocorrelation's maxima sit on samples (the
    refinement starts within 0.03 lags of one: Praat's own iterates).  A tail of zeros behind it gives frames whose local peak is 0."""
    n = np.arange(period)
    one = 6000.0 * np.cos(2 * np.pi * n / period) + 2500.0 * np.cos(2 * np.pi * 2 * n / period + 0.7) + 1200.0 * np.cos(2 * np.pi * 5 * n / period + 1.9)
    one = np.round(one).astype(np.int16)
    reps = int(seconds * rate) // period
    return np.concatenate([np.tile(one, reps), np.zeros(int(tail * rate), np.int16)])


def high_tone(rate, seconds=0.3):
    """A tone with a period of 3.1 samples over a weaker 200 Hz one: every frame has a maximum at lag 3, a candidate above 0.3 x rate, which the
    refinement interpolates at depth 700 -- unclamped only where the half window exceeds 700 lags (44.1 kHz / 75 Hz, 48 kHz / 50 Hz)."""
    t = np.arange(int(seconds * rate)) / rate
    rng = np.random.default_rng(rate)
    x = 6000.0 * np.sin(2 * np.pi * (rate / 3.1) * t) + 3000.0 * np.sin(2 * np.pi * 200.0 * t + 0.3) + 2.0 * rng.standard_normal(len(t))
    return np.round(x).astype(np.int16)


def shortest_length(rate, p):
    """The smallest number of samples Praat analyses under ``p`` (one frame); one fewer is refused."""
    lo, hi = 1, rate
    def ok(n):
        try:
            O.pitch_plan(n, 1.0 / rate, 0.5 / rate, p)
            return True
        except O.PraatError:
            return False
    assert ok(hi) and not ok(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def clips(form_id):
    """[(name, int16 clip)] of one form."""
    rate, floor, _, _, _ = FORMS[form_id]
    p = params(form_id)
    if rate == 16000:
        c1 = _c1()
        n1 = shortest_length(rate, p)
        return [("c1", c1), ("mixture", mixture(c1, rate, 16)), ("periodic", periodic(rate, 80)), ("zeros", np.zeros(8000, np.int16)),
                ("len-edge", c1[4000:4000 + n1].copy()), ("len-edge-1", c1[4000:4000 + n1 - 1].copy()), ("len-edge+hop", c1[4000:4000 + n1 + int(np.ceil(0.75 / floor * rate))].copy())]
    if rate == 8000:
        c8 = O.resample_int16(_c1(), 16000, 8000)
        return [("c1@8k", c8), ("mixture", mixture(c8, rate, 8)), ("periodic", periodic(rate, 40))]
    if rate == 44100:
        return [("demo", _demo()), ("periodic", periodic(rate, 220)), ("high-tone", high_tone(rate))]
    assert rate == 48000
    return [("demo@48k", O.resample_int16(_demo(), 44100, 48000)), ("periodic", periodic(rate, 240)), ("high-tone", high_tone(rate))]


@functools.lru_cache(maxsize=None)
def oracle(form_id):
    """[(name, clip, result of O.pitch_ac(want_candidates=True) or None where Praat refuses the length)] of one form; read only."""
    rate = FORMS[form_id][0]
    out = []
    for name, c in clips(form_id):
        try:
            w = O.pitch_ac(c.astype(np.float64) / 32768.0, 1.0 / rate, 0.5 / rate, params(form_id), want_candidates=True)
        except O.PraatError:
            w = None
        out.append((name, c, w))
    return out


def edge_counts(form_id):
    """The edges of k_pitch_frames and k_pitch_refine, counted in the oracle's output of one form."""
    rate, _, maxc, _, _ = FORMS[form_id]
    cnt = dict(rare_frames=0, depth700=0, low_lag=0, near_sample=0, local_peak_zero=0, full_without_replacement=0, frames=0, candidates=0)
    for name, c, w in oracle(form_id):
        if w is None:
            continue
        n = w["ncand"]; cf = w["cand_f"]
        live = (np.arange(cf.shape[1])[None, :] < n[:, None]) & (np.arange(cf.shape[1])[None, :] >= 1)
        lag = np.where(live, rate / np.where(live, cf, 1.0), np.nan)
        cnt["frames"] += len(n); cnt["candidates"] += int(live.sum())
        cnt["rare_frames"] += int(np.count_nonzero(w["n_maxima"] > maxc - 1))
        cnt["depth700"] += int(np.count_nonzero(live & (cf > 0.3 * rate)))
        cnt["low_lag"] += int(np.count_nonzero(lag <= 8.0))
        cnt["near_sample"] += int(np.count_nonzero(np.abs(lag - np.rint(lag)) < 0.03))
        if np.any(c != 0):                                               # (a clip of zeros has no global peak: another early exit)
            cnt["local_peak_zero"] += int(np.count_nonzero(w["intensity"] == 0.0))
        cnt["full_without_replacement"] += int(np.count_nonzero((n == maxc) & (w["n_maxima"] == maxc - 1)))
    return cnt


def min_replace_margin(form_id):
    return min([float(w["replace_margin"].min()) for _, _, w in oracle(form_id) if w is not None and len(w["replace_margin"])] + [np.inf])


EDGES = ("rare_frames", "depth700", "low_lag", "near_sample", "local_peak_zero")


def assert_stage_a_preconditions(form_id):
    """On the oracle's output alone: the set holds every edge, at least 5 frames with more maxima than slots, and no replacement decision closer
    than 1e-9."""
    cnt = edge_counts(form_id)
    assert cnt["rare_frames"] >= 5, (form_id, cnt)
    for k in EDGES:
        assert cnt[k] > 0, (form_id, k, cnt)
    for name, _, w in oracle(form_id):
        if w is not None:
            assert np.all(w["replace_margin"] > 1e-9), (form_id, name, float(w["replace_margin"].min()))
    return cnt


def sustained_tone():
    """6 s of a harmonic tone at 220 Hz, 16 kHz: one run of multi-candidate frames longer than k_pitch_path keeps back-pointers in LDS for."""
    t = np.arange(6 * 16000) / 16000.0
    x = 0.3 * 32768 * (np.sin(2 * np.pi * 220.0 * t) + 0.3 * np.sin(2 * np.pi * 440.0 * t + 0.4) + 0.15 * np.sin(2 * np.pi * 660.0 * t + 1.1))
    return np.round(0.6 * x).astype(np.int16)


def longest_run(ncand):
    best = cur = 0
    for m in np.asarray(ncand) > 1:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return best


# ------------------------------------------------------------------------------------------------------------------ stage B: given candidates

def path_params(ceiling=CEILING, silence_threshold=0.03, max_candidates=15, **kw):
    """The costs and thresholds of parselmouth's to_pitch as a plain namespace (what ``path_finder`` reads); ``engine_params`` makes the C struct."""
    d = dict(time_step=0.0, pitch_floor=75.0, periods_per_window=3.0, max_candidates=max_candidates, silence_threshold=silence_threshold,
             voicing_threshold=0.45, octave_cost=0.01, octave_jump_cost=0.35, voiced_unvoiced_cost=0.14, pitch_ceiling=ceiling)
    d.update(kw)
    return SimpleNamespace(**d)


def engine_params(p):
    from prosody_control_french_tts_amd import PitchParams
    return PitchParams(p.time_step, p.pitch_floor, p.periods_per_window, int(p.max_candidates), 0, p.silence_threshold, p.voicing_threshold,
                       p.octave_cost, p.octave_jump_cost, p.voiced_unvoiced_cost, p.pitch_ceiling)


def blank(T):
    """A slice of T cut frames: (cand_f, cand_s [T, 16] with NaN in every slot a kernel must not read, ncand, intensity)."""
    cf = np.full((T, K), np.nan); cs = np.full((T, K), np.nan)
    cf[:, 0] = 0.0; cs[:, 0] = 0.0
    return cf, cs, np.ones(T, np.int32), np.full(T, 0.5)


def random_slice(rng, T, n_lo=2, n_hi=15, p_cut=0.0, f_lo=60.0, f_hi=700.0, cut_frames=(), s_lo=0.05):
    """T frames of n_lo .. n_hi candidates (slot 0 included), f log-uniform over [f_lo, f_hi], s and intensity uniform; a share p_cut of frames, and
    the frames listed, hold the voiceless candidate alone."""
    cf, cs, n, inten = blank(T)
    n[:] = rng.integers(n_lo, n_hi + 1, T)
    n[rng.random(T) < p_cut] = 1
    n[list(cut_frames)] = 1
    live = (np.arange(K)[None, :] < n[:, None]) & (np.arange(K)[None, :] >= 1)
    cf[live] = np.exp(rng.uniform(np.log(f_lo), np.log(f_hi), int(live.sum())))
    cs[live] = rng.uniform(s_lo, 1.0, int(live.sum()))
    inten[:] = rng.uniform(0.0, 1.0, T)
    return cf, cs, n, inten


def concat(slices):
    """[(cf, cs, n, inten)] -> the arrays of one call and frame_off."""
    off = np.concatenate([[0], np.cumsum([len(s[2]) for s in slices])]).astype(np.int64)
    return (off, np.concatenate([s[2] for s in slices]).astype(np.int32), np.concatenate([s[3] for s in slices]),
            np.concatenate([s[0] for s in slices]), np.concatenate([s[1] for s in slices]))


# Each batch is one call of pce_selftest_pitch_path: (path parameters, dt, [slices]).  The seeds were picked on the CPU so that every arg-max of
# every slice clears the gap bound (pitch_restatement.gap_bound); both test files assert that they do.
LADDER = (1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 1280, 1281, 2049)       # run lengths around PT_CHUNK, BT_TILE and PT_CAP


def _run_between_cuts(rng, lengths, **kw):
    """One slice: a cut frame, then each run of the given length followed by a cut frame."""
    T = 1 + sum(L + 1 for L in lengths)
    cuts, pos = [0], 1
    for L in lengths:
        pos += L; cuts.append(pos); pos += 1
    return random_slice(rng, T, cut_frames=cuts, **kw)


def _forced(T, voiced, f=200.0):
    """T frames; the frames listed in ``voiced`` hold one strong candidate (f scalar or per listed frame), all others are cuts: the path takes it."""
    cf, cs, n, inten = blank(T)
    voiced = np.asarray(voiced, dtype=np.int64)
    n[voiced] = 2; cf[voiced, 1] = f; cs[voiced, 1] = 1.0
    return cf, cs, n, inten


def exact_cases():
    """Slices with exact ties or class boundaries, and what a correct path finder returns for them, worked out by hand (ceiling 600, silence
    threshold 0: the unvoiced strength is 0.45 in every frame; dt = 0.01: costs 0.35 per octave and 0.14; octave cost 0.01).
    -> [(name, slice, expected f0, {(frame, slot): expected psi})]"""
    C = CEILING
    up, down = np.nextafter(C, np.inf), np.nextafter(C, -np.inf)
    out = []
    def one(name, frames, f0, psi):
        cf, cs, n, inten = blank(len(frames))
        for t, cands in enumerate(frames):
            n[t] = 1 + len(cands)
            for j, (f, s) in enumerate(cands, start=1):
                cf[t, j] = f; cs[t, j] = s
        out.append((name, (cf, cs, n, inten), np.array(f0, dtype=np.float64), psi))
    # f == ceiling is voiced in the local term: 0.45 - 0.01 log2(1) = 0.45 exactly, a tie with the voiceless 0.45 -> the first (F0 = 0)
    one("tie-at-threshold", [[(C, 0.45)]], [0.0], {})
    one("just-above-threshold", [[(C, np.nextafter(0.45, 1.0))]], [C], {})
    # ... and voiceless in a transition.  Frame 1 holds (300, 0.9): local 0.9 - 0.01 = 0.89.
    #   f = C:     into slot 1: 0.45 - 0.14 + 0.89 = 1.20 from slot 0, 0.5 - 0.14 + 0.89 = 1.25 from slot 1 (voiced there: 0.5 - 0.35 + 0.89 = 1.04)
    #              into slot 0: 0.45 + 0.45 = 0.90 from slot 0, 0.5 - 0 + 0.45 = 0.95 from slot 1
    #   f = C+:    slot 1 is a twin of slot 0 (local 0.45, voiceless in transitions): all values tie, slot 0 wins
    #   f = C-:    voiced: into slot 1 0.5 - 0.35 + 0.89 = 1.04 < 1.20, into slot 0 0.5 - 0.14 + 0.45 = 0.81 < 0.90
    one("at-ceiling", [[(C, 0.5)], [(300.0, 0.9)]], [C, 300.0], {(1, 0): 1, (1, 1): 1})
    one("above-ceiling", [[(up, 0.5)], [(300.0, 0.9)]], [0.0, 300.0], {(1, 0): 0, (1, 1): 0})
    one("below-ceiling", [[(down, 0.5)], [(300.0, 0.9)]], [0.0, 300.0], {(1, 0): 0, (1, 1): 0})
    # several above-ceiling twins and the voiceless candidate: whatever points at them names slot 0; (200, 0.3) is the only other candidate:
    #   into (210, 0.95) [local 0.95 - 0.01 log2(600 / 210) = 0.9349]: 0.45 - 0.14 from the twins, 0.3 - 0.01585 - 0.35 log2(1.05) = 0.2595 from slot 2
    one("twins-above-ceiling", [[(5000.0, 0.99), (200.0, 0.3), (up, 0.2), (650.0, 0.8)], [(210.0, 0.95)]], [0.0, 210.0], {(1, 0): 0, (1, 1): 0})
    # duplicates in slots 2 < 4 of frame 0 (250, 0.9), stronger than everything else: every back-pointer of frame 1 names slot 2,
    # in the middle of a run, as the last frame before a cut (the run's end is chosen among them) and as the last frame of a slice
    dup = [(120.0, 0.2), (250.0, 0.9), (480.0, 0.3), (250.0, 0.9)]
    nxt = [(245.0, 0.8), (130.0, 0.7), (500.0, 0.6)]
    one("duplicates-mid-run", [dup, nxt, [(240.0, 0.8)]], [250.0, 245.0, 240.0], {(1, 0): 2, (1, 1): 2, (1, 2): 2, (1, 3): 2})
    one("duplicates-before-cut", [[(255.0, 0.8)], dup, [], [(240.0, 0.8)]], [255.0, 250.0, 0.0, 240.0], {(1, 2): 1, (1, 4): 1, (2, 0): 2})
    one("duplicates-at-slice-end", [[(255.0, 0.8)], dup], [255.0, 250.0], {(1, 2): 1, (1, 4): 1})
    # The cut frame of duplicates-before-cut has no back-pointer on the device (k_pitch_path stores none for a frame with one candidate), so its
    # (2, 0): 2 is checked on the host only, and the track cannot tell slot 2 from slot 4: equal bits.  The first-maximum rule at the end of a run
    # is seen on the device through twins that differ in frequency: with nothing voiced in the frame, the voiceless candidate and the two above
    # the ceiling tie at 0.45 and slot 0 must win -- F0 = 0, where the last maximum would give 650 -- before a cut and at a slice end
    one("twins-before-cut", [[(5000.0, 0.99), (650.0, 0.8)], []], [0.0, 0.0], {(1, 0): 0})
    one("twins-at-slice-end", [[(5000.0, 0.99), (650.0, 0.8)]], [0.0], {})
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """name -> (path parameters, dt, [slices])"""
    B = {}
    rng = np.random.default_rng(2301)
    whole = [random_slice(rng, L, n_hi=6) for L in LADDER]
    between = [_run_between_cuts(rng, [L], n_hi=6) for L in LADDER] + [_run_between_cuts(rng, [L for L in LADDER if L <= 257], n_hi=6)]
    B["ladder"] = (path_params(), 0.01, whole + between)
    B["alone-1025"] = (path_params(), 0.01, [whole[LADDER.index(1025)]])
    B["alone-2049"] = (path_params(), 0.01, [whole[LADDER.index(2049)]])
    B["alone-2049-between-cuts"] = (path_params(), 0.01, [between[LADDER.index(2049)]])
    rng = np.random.default_rng(2302)
    B["run-lists-alternating"] = (path_params(), 0.01, [random_slice(rng, 20000, n_hi=4, cut_frames=range(1, 20000, 2))])   # 10 000 runs: 156 per list
    B["run-lists-one-frame-slices"] = (path_params(), 0.01, [random_slice(rng, 1, n_hi=5) for _ in range(4096)])
    rng = np.random.default_rng(2303)
    B["counts"] = (path_params(), 0.01, [random_slice(rng, 40, n_lo=n, n_hi=n) for n in (2, 3, 8, 15)] + [random_slice(rng, 70, n_lo=2, n_hi=15)])
    B["counts-16"] = (path_params(max_candidates=16), 0.01, [random_slice(rng, 40, n_lo=16, n_hi=16), random_slice(rng, 70, n_lo=2, n_hi=16, p_cut=0.1)])
    # candidate classes: a third of the candidates sits at the ceiling, one ulp beside it or far above
    rng = np.random.default_rng(2304)
    cls = []
    special = np.array([CEILING, np.nextafter(CEILING, np.inf), np.nextafter(CEILING, -np.inf), 5000.0, 650.0, 1e6])
    for T in (60, 200):
        cf, cs, n, inten = random_slice(rng, T, n_lo=2, n_hi=9, p_cut=0.1)
        live = (np.arange(K)[None, :] < n[:, None]) & (np.arange(K)[None, :] >= 1)
        pick = live & (rng.random((T, K)) < 0.35)
        cf[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        cls.append((cf, cs, n, inten))
    B["classes"] = (path_params(), 0.01, cls)
    B["exact"] = (path_params(silence_threshold=0.0), 0.01, [c[1] for c in exact_cases()])
    # the unvoiced term 0.45 + max(0, 2 - intensity / (0.03 / 1.45)) has its zero at intensity 0.04138; the time-step correction 0.01 / dt
    for dt in (0.005, 0.01, 0.015):
        for sil in (0.03, 0.0, -1.0):
            rng = np.random.default_rng(2305)
            sl = []
            for T in (50, 120):
                s = random_slice(rng, T, n_lo=1, n_hi=7)
                s[3][:] = rng.choice([0.0, 0.02, 0.0413, 0.0414, 0.0415, 0.06, 0.5, 1.0], T)
                sl.append(s)
            B[f"terms-dt{dt}-sil{sil}"] = (path_params(silence_threshold=sil), dt, sl)
    rng = np.random.default_rng(2306)
    B["random"] = (path_params(), 0.01, [random_slice(rng, int(rng.integers(1, 301)), n_lo=1, n_hi=15, p_cut=0.2) for _ in range(64)])
    # medians: the in-LDS sort holds 16 384 frames, k_pitch_median_long takes longer slices
    rng = np.random.default_rng(2327)
    last_byte = (np.float64(200.0).view(np.int64) + rng.permutation(256)).view(np.float64)       # 256 values that differ in the last mantissa byte only
    B["medians"] = (path_params(), 0.01, [
        random_slice(rng, 16384, n_hi=3, p_cut=0.1, s_lo=0.7), random_slice(rng, 16385, n_hi=3, p_cut=0.1, s_lo=0.7), random_slice(rng, 37, n_hi=5, p_cut=0.3),
        _forced(9, []), _forced(9, [4]), _forced(9, [2, 6], f=[180.0, 190.0]), _forced(40, range(0, 40, 3), f=200.0 + np.arange(14)),
        _forced(41, range(1, 41, 3), f=230.0 - np.arange(14)), _forced(30, range(30)), _forced(256, range(256), f=last_byte),
        _forced(255, range(255), f=last_byte[:255]), random_slice(rng, 16385, n_hi=2, p_cut=0.98), _forced(16390, range(5, 16390, 64))])
    rng = np.random.default_rng(2328)
    B["median-40000"] = (path_params(), 0.01, [random_slice(rng, 40000, n_hi=3, p_cut=0.25, s_lo=0.6)])
    rng = np.random.default_rng(2309)
    lb = (np.float64(200.0).view(np.int64) + rng.integers(0, 256, 20000)).view(np.float64)
    B["median-long-last-byte"] = (path_params(), 0.01, [_forced(20000, range(20000), f=lb), _forced(17001, range(17001))])
    return B


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's result for every slice of a batch (read only), with the slice's gap bound: [dict]."""
    from pitch_restatement import path_finder, gap_bound
    p, dt, slices = batches()[name]
    out = []
    for cf, cs, n, inten in slices:
        r = path_finder(cf, cs, n, inten, dt, p)
        r["bound"] = gap_bound(len(n), r["max_abs_delta"])
        out.append(r)
    return out
