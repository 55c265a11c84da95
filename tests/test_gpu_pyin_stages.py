"""The two pYIN kernels of csrc/pce_pyin.hip stage by stage against float64 (oracle/pyin_oracle.py), every frame and every entry.

Stage A, k_pyin_frames against ``PO.observations(exact=True)``, through pce_pyin_run and pce_pyin_fetch_observations.  Per frame: the number
of observations, the status and every pitch bin are EQUAL, no frame or entry left out (the inputs are chosen, and asserted, to hold no
candidate whose unrounded bin index 12 n log2(f / fmin) is within 1e-9 of a half-integer, where the two log2 could round apart).  With
u = 2^-53 and n_thr = 100 thresholds:
  * log_probs against np.log(p + tiny): a probability is a sum of at most n_thr + 1 positive terms of three factors, (n_thr + 4) u relative,
    which is that much absolute in its logarithm; plus one ulp of |log p| for each of the two logarithms (numpy's, and the device's: the HIP
    math API's accuracy table gives log in double precision as 1 ULP);
  * voiced_prob against the oracle's: the same (n_thr + 4) u plus n u for the sum of the frame's n observations, relative to the sum (all terms
    positive), before the clip to [0, 1];
  * log_unvoiced against np.log((1 - vp) / n_bins + tiny) of the DEVICE's vp: the two ulp of the logarithms (the argument is the same three
    correctly rounded operations on both sides).
Entries of a list beyond n keep the caller's prefill.

Each edge is a condition counted in the oracle's output and asserted to occur, so that no edge can be passed by missing it (EDGES below;
the counts are in MEASURED).  ``bin == n_bins`` cannot be reached at fmax = 2000 with any of the five rates -- the shortest period a refined
trough can have is min_period (lag index 0 is not refined, index 1 shifts by less than one lag), and 12 n log2(sr / min_period / fmin) is at
most 607.46 < 607.5 (44100 and 22050 Hz) -- so the 16 kHz clips run a second time under fmax = 1990 (607 bins; 2000 Hz is bin 607).

Stage B, k_pyin_viterbi against ``PO.viterbi_log`` on given observation lists, through pce_selftest_pyin_viterbi (the run's own launch): the
decoded states are EQUAL in every frame, unvoiced indices included, no allowance -- the kernel adds what the dense evaluation adds, in its
order, and takes the first maximum.  Out-of-band predecessors tie on the ROUNDED sum V + log(tiny): the two-frame case of
tests/test_pyin.py (probabilities 0.5 and 0.5 (1 + 1e-15) next to each other, a target beyond the band of both) and its mirror image
decoded [101, 300] / [501, 300] on the kernel that scanned V itself (prefix / suffix maximum first, log(tiny) added afterwards); they decode
[100, 300] / [500, 300] as the dense argmax does since the scans run over V + log(tiny).

The chain: for every stage-A clip the device's own observation lists go through ``PO.viterbi_log`` on the host, and the result equals the
device's states in every frame.  With stage A that closes the path from samples to states.

MEASURED (MI355X, worst |got - want| / bound over every entry of every frame of every clip):
  set              log_probs   voiced_prob   log_unvoiced   edges counted in the oracle's output (dropped / overwritten / vp clipped / acf clamped)
  16000            0.276       0.055         0              0 / 0 / 8 / 6
  44100            0.276       0.076         0              0 / 53 / 0 / 7      (one frame with several candidates in bin 0)
  8000             0.276       0.118         0              0 / 0 / 8 / 6
  22050            0.276       0.069         0              0 / 0 / 0 / 6
  64000            0.276       0.053         0              0 / 273 / 1 / 6
  16000-fmax1990   0.276       0.055         0              15 / 0 / 0 / 6
  hop 1 (8000)     0.065       0.057         0              (frames 0, 1, 4095, 4096, 4097, 4200 of 4201)
  all sets                                                  15 / 326 / 17 / 37
(0.276 is the no-trough mass 0.01 x sum(beta) of a frame's global minimum: 4 ulp of log 0.01.)  log_unvoiced equals numpy's logarithm bit for bit on
every frame, voiced_prob == 1 (log(tiny)) included.  Stage B and the chain: every state equal, 9 plans and 7 clip sets.
"""
import functools

import numpy as np
import pytest

from oracle import pyin_oracle as PO
from prosody_control_french_tts_amd.visualisation import acoustic_analysis as AA

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
W = 512                                                              # row width of an observation list
RATES = [16000, 44100, 8000, 22050, 64000]                          # 5 lag groups, 12, the generic form twice, all 16 (max_period capped at 1023)
HOP = 256
EDGES = ("dropped", "overwritten", "vp_clipped", "acf_clamped")


def _clips(rate):
    """Short clips (at most 12 frames) that reach the edges of k_pyin_frames; deterministic."""
    rng = np.random.default_rng(rate)
    n = 10 * HOP
    t = np.arange(n) / rate
    f_lo = rate / (np.ceil(rate / 60.0) - 1.5) if rate < 64000 else 63.0   # troughs in the last lags: several candidates in bin 0
    def tone(f, a=9000.0, noise=200.0, h2=0.3):
        return np.round(a * np.sin(2 * np.pi * f * t) + h2 * a * np.sin(4 * np.pi * f * t + 0.5) + noise * rng.standard_normal(n)).astype(np.int16)
    square = np.where((np.arange(n) // 40) % 2 == 0, 32767, -32768).astype(np.int16)          # period 80 samples, exactly periodic
    quiet = rng.integers(1, 4, n) * rng.choice([-1, 1], n)                                      # +-1 .. 3 LSB
    quiet[: 4 * HOP] = rng.choice([-1, 1], 4 * HOP)                                             # +-1 LSB: window energy 1024 x 2^-30 < 1e-6
    quiet[4 * HOP: 6 * HOP][rng.random(2 * HOP) < 0.5] = 0                                      # ... and below it
    clips = [("harmonic", tone(rate / 97.3 if rate > 8000 else 196.0)),
             ("chirp", np.round(9000 * np.sin(2 * np.pi * (150 + 200 * t) * t) + 300 * rng.standard_normal(n)).astype(np.int16)),
             ("zeros", np.zeros(n, np.int16)),
             ("quiet", quiet.astype(np.int16)),
             ("square", square),
             ("near2000", tone(1993.0, noise=30.0, h2=0.0)),
             ("near60", tone(f_lo, noise=400.0)),
             ("noise", (rng.standard_normal(n) * 2500).astype(np.int16))]
    base = tone(rate / 61.7 if rate > 8000 else 131.0)
    for name, m in (("len1", 1), ("len3", 3), ("k_hop_m1", 3 * HOP - 1), ("k_hop", 3 * HOP), ("k_hop_p1", 3 * HOP + 1)):
        clips.append((name, base[:m].copy()))
    return clips


def _sets():
    """(id, rate, plan keywords): the five rates under the viewers' plan, and 16 kHz under fmax = 1990 for the bin == n_bins drop."""
    return [(str(r), r, {}) for r in RATES] + [("16000-fmax1990", 16000, dict(fmax=1990.0))]


@functools.lru_cache(maxsize=None)
def _oracle(set_id):
    _, rate, kw = next(s for s in _sets() if s[0] == set_id)
    out = []
    for name, c in _clips(rate):
        obs, vp, info = PO.observations(c.astype(np.float32) / np.float32(32768.0), rate, hop_length=HOP, exact=True, **kw)
        out.append((name, c, obs, vp, info))
    return out


def _edge_counts(set_id):
    cnt = dict.fromkeys(EDGES, 0)
    for _, _, _, _, info in _oracle(set_id):
        cnt["dropped"] += int(info["dropped"].sum()); cnt["overwritten"] += int(info["overwritten"].sum())
        cnt["vp_clipped"] += int(np.count_nonzero(info["vp_sum"] > 1.0)); cnt["acf_clamped"] += int(np.count_nonzero(info["acf_clamped"]))
    return cnt


def _assert_no_half_integer_bins(info):
    nb = info["n_pitch_bins"]
    for raw in info["raw"]:
        r = raw[(raw > -1.0) & (raw < nb + 1.0)]
        assert np.all(np.abs(r - np.floor(r) - 0.5) > 1e-9)


def test_every_edge_occurs_in_the_oracle_output():
    """No GPU needed: the inputs hold every named edge, and no candidate on a rounding boundary of the bins."""
    total = dict.fromkeys(EDGES, 0)
    for set_id, _, _ in _sets():
        for _, _, _, _, info in _oracle(set_id):
            _assert_no_half_integer_bins(info)
        for k, v in _edge_counts(set_id).items():
            total[k] += v
        if set_id != "16000-fmax1990":
            assert _edge_counts(set_id)["dropped"] == 0                     # unreachable at fmax = 2000 (docstring)
    print("edge counts", total, {s[0]: _edge_counts(s[0]) for s in _sets()})
    assert all(v > 0 for v in total.values()), total
    n0 = 0                                                                   # several troughs land in bin 0 of one frame: the later one wins
    for _, _, _, _, info in _oracle("44100"):
        n0 += sum(int(np.count_nonzero(np.round(raw) <= 0) >= 2) for raw in info["raw"])
    print("frames with several candidates in bin 0 (44100 Hz):", n0)
    assert n0 > 0


def _dense_logs(plan, obs_rows):
    """log_obs [T][2 nb] from lists [(bins, log_probs, log_unvoiced)], as the kernel fills its column: log(0 + tiny) where nothing was observed."""
    nb = plan.n_pitch_bins
    lo = np.full((len(obs_rows), 2 * nb), np.log(PO.TINY64))
    for t, (b, lp, lu) in enumerate(obs_rows):
        lo[t, b] = lp
        lo[t, nb:] = lu
    return lo


@functools.lru_cache(maxsize=None)
def _dense_trans(nb, width):
    T = np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), PO.transition_local_triangle(nb, width))
    return np.log(T + PO.TINY64), np.log(np.ones(2 * nb) / (2 * nb) + PO.TINY64)


class _Worst:
    def __init__(self):
        self.r = {"log_probs": 0.0, "voiced_prob": 0.0, "log_unvoiced": 0.0}
    def add(self, key, got, want, bound):
        got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(bound)
        if got.size:
            ratio = np.abs(got - want) / bound
            self.r[key] = max(self.r[key], float(np.max(ratio)))


def _check_stage_a(dev, obs, vp, n_bins, n_thr, worst, label):
    """One clip: the device's lists ``dev`` (pyin_fetch_observations) against the oracle's, every frame."""
    assert len(dev["n"]) == len(obs), label
    for f, (b, p) in enumerate(obs):
        n = len(b)
        assert dev["n"][f] == n and dev["status"][f] == 0, (label, f, dev["n"][f], n)
        assert np.array_equal(dev["bins"][f, :n], b), (label, f, dev["bins"][f, :n], b)
        assert np.all(dev["bins"][f, n:] == -1) and np.all(np.isnan(dev["log_probs"][f, n:])), (label, f)     # nothing beyond n
        want = np.log(p + PO.TINY64)
        worst.add("log_probs", dev["log_probs"][f, :n], want, (n_thr + 4) * U + 2 * np.spacing(np.abs(want)))
        s = float(np.sum(p))
        worst.add("voiced_prob", dev["voiced_prob"][f], vp[f], max((n_thr + 4 + n) * U * s, 5e-324))
        dvp = dev["voiced_prob"][f]
        assert 0.0 <= dvp <= 1.0
        want_lu = np.log((1 - dvp) / n_bins + PO.TINY64)
        worst.add("log_unvoiced", dev["log_unvoiced"][f], want_lu, 2 * np.spacing(np.abs(want_lu)))


@pytest.mark.parametrize("set_id", [s[0] for s in _sets()])
def test_frames_kernel_against_float64_and_the_chain_to_states(engine, set_id):
    _, rate, kw = next(s for s in _sets() if s[0] == set_id)
    ora = _oracle(set_id)
    plan, tables, _ = AA.pyin_plan(rate, hop_length=HOP, **kw)
    engine.upload([c for _, c, _, _, _ in ora], rate)
    engine.pyin_run(plan, tables)
    nb = plan.n_pitch_bins
    log_trans, log_pinit = _dense_trans(nb, plan.trans_width)
    worst = _Worst()
    for i, (name, c, obs, vp, info) in enumerate(ora):
        assert info["n_pitch_bins"] == nb and info["max_period"] == plan.max_period and len(obs) == 1 + len(c) // HOP
        _assert_no_half_integer_bins(info)
        dev = engine.pyin_fetch_observations(i)
        _check_stage_a(dev, obs, vp, nb, plan.n_thresholds, worst, (set_id, name))
        # the chain: the device's own lists, decoded densely on the host, are the device's states
        states, dvp, status = engine.pyin_fetch(i)
        assert status == 0 and np.array_equal(dvp, dev["voiced_prob"])
        rows = [(dev["bins"][f, :dev["n"][f]], dev["log_probs"][f, :dev["n"][f]], dev["log_unvoiced"][f]) for f in range(len(obs))]
        want_states = PO.viterbi_log(_dense_logs(plan, rows), log_trans, log_pinit)
        assert np.array_equal(states, want_states), (set_id, name, states, want_states)
    print("stage A", set_id, "worst |got - want| / bound:", worst.r, "edges:", _edge_counts(set_id))
    assert all(v <= 1.0 for v in worst.r.values()), worst.r


def test_grid_stride_second_pass_and_width_one(engine):
    """4201 frames (hop 1): the grid of k_pyin_frames covers 4096, its stride loop makes a second pass; transition width 1 (half == 0)."""
    rate, kw = 8000, dict(fmin=150.0, fmax=400.0, hop_length=1)      # lags 20 .. 54: a period near 21 samples has two troughs in them
    rng = np.random.default_rng(42)
    t = np.arange(4200) / rate
    c = np.round(8000 * np.sin(2 * np.pi * (365 + 20 * t) * t) + 2500 * np.sin(2 * np.pi * 2 * (365 + 20 * t) * t + 1.0) + 300 * rng.standard_normal(4200)).astype(np.int16)
    sel = [0, 1, 4095, 4096, 4097, 4200]
    plan, tables, _ = AA.pyin_plan(rate, **kw)
    assert plan.trans_width == 1 and plan.n_pitch_bins == 170
    obs, vp, info = PO.observations(c.astype(np.float32) / np.float32(32768.0), rate, exact=True, frames=sel, **kw)
    _assert_no_half_integer_bins(info)
    assert all(len(b) >= 1 for b, _ in obs) and all(len(obs[i][0]) == 2 for i in (2, 3, 4, 5))          # both passes of the grid see real work
    engine.upload([c], rate)
    engine.pyin_run(plan, tables)
    dev = engine.pyin_fetch_observations(0)
    assert len(dev["n"]) == 4201
    worst = _Worst()
    _check_stage_a({k: v[sel] for k, v in dev.items()}, obs, vp, plan.n_pitch_bins, plan.n_thresholds, worst, "hop1")
    print("stage A hop 1 worst:", worst.r)
    assert all(v <= 1.0 for v in worst.r.values()), worst.r
    # the chain over all 4201 frames (340 states: the dense decoding is cheap)
    states, _, status = engine.pyin_fetch(0)
    rows = [(dev["bins"][f, :dev["n"][f]], dev["log_probs"][f, :dev["n"][f]], dev["log_unvoiced"][f]) for f in range(4201)]
    log_trans, log_pinit = _dense_trans(plan.n_pitch_bins, 1)
    assert status == 0 and np.array_equal(states, PO.viterbi_log(_dense_logs(plan, rows), log_trans, log_pinit))


# ------------------------------------------------------------------------------------------------------------------ stage B

def _plan_for(n_bins, rate, hop=HOP, fmin=60.0):
    """A plan with exactly ``n_bins`` pitch bins, through fmax (0.1-semitone bins: n_bins = floor(120 log2(fmax / fmin)) + 1)."""
    plan, tables, _ = AA.pyin_plan(rate, fmin=fmin, fmax=fmin * 2.0 ** ((n_bins - 0.5) / 120.0), hop_length=hop)
    assert plan.n_pitch_bins == n_bins
    return plan, tables


PLANS = {"16k": lambda: AA.pyin_plan(16000)[:2],                     # 608 bins, width 71
         "44k1": lambda: AA.pyin_plan(44100)[:2],                    # 608 bins, width 31
         "nb63": lambda: _plan_for(63, 44100), "nb64": lambda: _plan_for(64, 44100), "nb65": lambda: _plan_for(65, 44100),
         "nb640": lambda: _plan_for(640, 44100),                     # VT_THREADS
         "smallest-w31": lambda: _plan_for(32, 44100),               # n_bins == 2 half + 2
         "smallest-w71": lambda: _plan_for(72, 16000),
         "width1": lambda: _plan_for(121, 8000, hop=1, fmin=200.0)}


def _frame(nb, bins, probs, vp=None):
    """(bins, log_probs, log_unvoiced) as k_pyin_frames would leave them for these probabilities."""
    b = np.asarray(bins, dtype=np.int64); p = np.asarray(probs, dtype=np.float64)
    vp = min(max(float(np.sum(p)), 0.0), 1.0) if vp is None else vp
    return b, np.log(p + PO.TINY64), float(np.log((1 - vp) / nb + PO.TINY64))


def _cases(nb, half, seed):
    rng = np.random.default_rng(seed)
    def random_clip(T, p_silent=0.1, p_full=0.15):
        fr, centre = [], int(rng.integers(0, nb))
        for _ in range(T):
            u = rng.random()
            if u < p_silent:
                fr.append(_frame(nb, [], [])); continue
            k = int(rng.integers(1, 6))
            centre = int(np.clip(centre + rng.integers(-2 * half - 3, 2 * half + 4), 0, nb - 1))
            bins = np.unique(np.clip(centre + rng.integers(-half - 2, half + 3, k), 0, nb - 1))
            p = rng.random(len(bins)) + 0.05
            p = p / p.sum() * (1.0 if u < p_silent + p_full else rng.random())
            fr.append(_frame(nb, bins, p, vp=1.0 if u < p_silent + p_full else None))
        return fr
    cases = {f"random-T{T}": random_clip(T) for T in (1, 2, 64, 65, 70)}
    n = int(rng.integers(3, 40))
    cases["random-T%d-any" % n] = random_clip(n)
    cases["silence"] = [_frame(nb, [], []) for _ in range(9)]                                     # every comparison a tie
    cases["silence-T1"] = [_frame(nb, [], [])]
    cases["all-voiced"] = random_clip(12, p_silent=0.0, p_full=1.0)                                # log_unvoiced = log(tiny) throughout
    far = min(nb - 1, half + 1 + int(rng.integers(0, 5)))
    # jumps beyond the band: down to and up from the edges, and targets within `half` of bin 0 / nb - 1
    ups = [0, far, min(nb - 1, 2 * far), nb - 1, max(0, nb - 1 - half // 2), nb - 1, half // 2, 0]
    cases["jumps"] = [_frame(nb, [b], [1.0], vp=1.0) for b in ups]
    cases["jumps-soft"] = [_frame(nb, [b, (b + 1) % nb], [0.6, 0.3]) for b in ups[::-1]]
    a, b = (100, 300) if nb > 520 else (0, nb - 1)
    c, d = (500, 300) if nb > 520 else (nb - 2, 0)
    assert abs(b - a) > half + 1 and abs(d - c) > half + 1
    # (width 1: the only in-band predecessor carries log(0.99), so the pair gets probability 1 to win from out of band; given lists need not sum to <= 1)
    pair = [0.5, 0.5 * (1 + 1e-15)] if half > 0 else [1.0, 1.0 + 2.0 ** -50]
    assert np.log(pair[1] + PO.TINY64) > np.log(pair[0] + PO.TINY64)
    cases["rounded-tie-prefix"] = [_frame(nb, [a, a + 1], pair, vp=1.0), _frame(nb, [b], [1.0])]
    cases["rounded-tie-suffix"] = [_frame(nb, [c, c + 1], pair, vp=1.0), _frame(nb, [d], [1.0])]
    return cases


def _run_viterbi(engine, plan, tables, clips):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clips])]).astype(np.int64)
    total = int(off[-1])
    n = np.zeros(total, np.int32); lu = np.zeros(total); bins = np.zeros((total, W), np.int32); lp = np.zeros((total, W))
    f = 0
    for c in clips:
        for b, l, u in c:
            n[f] = len(b); bins[f, :len(b)] = b; lp[f, :len(b)] = l; lu[f] = u; f += 1
    st = engine.selftest_pyin_viterbi(plan, tables, off, n, lu, bins, lp)
    return [st[off[i]:off[i + 1]] for i in range(len(clips))]


@pytest.mark.parametrize("name", list(PLANS))
def test_viterbi_kernel_against_the_dense_argmax(engine, name):
    plan, tables = PLANS[name]()
    nb, half = plan.n_pitch_bins, plan.trans_width // 2
    assert nb >= 2 * half + 2 and (not name.startswith("smallest") or nb == 2 * half + 2) and (name != "width1" or half == 0)
    log_trans, log_pinit = _dense_trans(nb, plan.trans_width)
    cases = _cases(nb, half, seed=nb * 1000 + half)
    want = {k: PO.viterbi_log(_dense_logs(plan, c), log_trans, log_pinit) for k, c in cases.items()}
    lo_a = int(cases["rounded-tie-prefix"][0][0][0]); lo_c = int(cases["rounded-tie-suffix"][0][0][0])
    assert want["rounded-tie-prefix"][0] == lo_a and want["rounded-tie-suffix"][0] == lo_c          # the dense answer: the first of the tie
    assert np.all(want["silence"] >= nb) and np.all(want["all-voiced"] < nb)
    got = dict(zip(cases, _run_viterbi(engine, plan, tables, list(cases.values()))))               # one batch of clips of unequal T
    for k in cases:
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    for k in ("random-T65", "silence", "rounded-tie-suffix", "random-T1"):                          # ... and each clip alone: the same states
        assert np.array_equal(_run_viterbi(engine, plan, tables, [cases[k]])[0], got[k]), (name, k)


def test_viterbi_selftest_refuses_what_the_kernel_cannot_take(engine):
    from prosody_control_french_tts_amd import PceError
    plan, tables = PLANS["nb64"]()
    ok = [_frame(64, [3], [0.5])]
    assert len(_run_viterbi(engine, plan, tables, [ok, []])[1]) == 0                                # an empty clip beside a real one
    for bad in ([_frame(64, [64], [0.5])], [_frame(64, [-1], [0.5])], [_frame(64, [5, 5], [0.2, 0.3])]):
        with pytest.raises(PceError):
            _run_viterbi(engine, plan, tables, [bad])
    with pytest.raises(PceError):
        engine.selftest_pyin_viterbi(plan, tables[:-1], [0, 1], [0], [0.0], np.zeros((1, W), np.int32), np.zeros((1, W)))
    small, st = AA.pyin_plan(44100, fmax=60.0 * 2.0 ** (30.5 / 120.0))[:2]                          # 31 bins under width 31: below 2 half + 2
    with pytest.raises(PceError):
        engine.selftest_pyin_viterbi(small, st, [0, 1], [0], [0.0], np.zeros((1, W), np.int32), np.zeros((1, W)))
    # a resident run is not disturbed
    engine.upload([np.zeros(600, np.int16)], 16000)
    p16, t16 = PLANS["16k"]()
    engine.pyin_run(p16, t16)
    before = engine.pyin_fetch(0)[0].copy()
    _run_viterbi(engine, plan, tables, [ok])
    assert np.array_equal(engine.pyin_fetch(0)[0], before)
