"""The Praat pitch kernels of csrc/pce_pitch.hip stage by stage in float64: the candidates, then the path.

Stage A, k_pitch_frames + k_pitch_refine against the CPU oracle's candidates (oracle/pce_oracle.c, ``want_candidates``), through pce_pitch_run and
pce_pitch_fetch_candidates.  One clip set per instantiation of k_pitch_frames (tests/pitch_cases.py: FORMS), every set under both refine modes,
the 16 kHz / 150 Hz set a second time with max_candidates = 16.  Every frame and every slot, nothing left out:
  * ncand EQUAL;
  * slot for slot, cand_f within 1e-6 relative and cand_s within 1e-6 absolute (the project's gate for the refined maximum: the comment on
    k_pitch_refine says why the seeded search and Praat's iterates end that close and no closer);
  * slots at or beyond ncand keep the caller's prefill, slot 0 reads 0 / 0;
  * intensity within 8 u relative, u = 2^-53: the same few correctly rounded operations on both sides.
Edges, each counted in the oracle's output and asserted to occur in every form (pitch_cases.EDGES; the counts are in MEASURED): frames with more
local maxima than candidate slots (the "rare" path: first-pass strengths and Praat's replacement rule), at least 5 per form; candidates above
0.3 x rate (sinc depth 700, lags below 3.33: the speech at 44.1 / 48 kHz holds no maximum that short, a tone of period 3.1 samples does, and there
the half window is longer than 700 lags, so the depth is not clamped); candidates at lag <= 8 (outside the register window of the refinement); refined lags
within 0.03 of a sample (Praat's own iterates in the seeded mode); frames whose local peak is 0.  Frames that fill every slot without a
replacement (ncand == maxc, n_maxima == maxc - 1) are counted and not required.  Precondition, asserted for every frame: every replacement
decision of the oracle has a margin |new - weakest| above 1e-9, so that no frame's candidate set hangs on the last bits of a first-pass strength.

Stage B, k_pitch_delta + k_pitch_path + k_pitch_median + k_pitch_median_long on given candidates against tests/pitch_restatement.py, through
pce_selftest_pitch_path (the tail of a real run's launch code).  psi EQUAL for every (frame with more than one candidate, slot < ncand) -- a frame
with the voiceless candidate alone has no back-pointers on the device: the choice made in front of it shows in the track (through candidates that
tie bit for bit but differ in frequency: ``twins-before-cut`` of ``exact_cases``); f0 and strength EQUAL
in every frame (they are copies of candidates); n_voiced EQUAL; median_f0 == np.median of the track; mean_log_f0 within (n_voiced + 2) u x
mean |log f| of math.fsum.  Precondition per slice, asserted: every arg-max of the restatement has a gap (to the best candidate that is no twin of
the winner) above B = 8 (L + 8) u M (pitch_restatement.gap_bound), so the device may round differently and still must decide the same.  The
only decisions not held to it are the two exact ties of ``exact_cases`` whose operands are exact on both sides (0.45 against 0.45).
The batches (tests/pitch_cases.py: batches): run lengths around PT_CHUNK = 16, BT_TILE = 256 and PT_CAP = 1024 as whole slices and between cut
frames, all in one call and 1025 / 2049 alone; 10 000 runs in one slice (more than 64 per run list) and 4096 one-frame slices; 2, 3, 8, 15 and 16
candidates; candidates at the ceiling, one ulp beside it and far above, twins included; exact ties by hand; both signs of the silence threshold,
intensities on both sides of the zero of the unvoiced term, three frame steps; 64 random slices; the medians at 16 384 / 16 385 frames, 40 000
frames, 0 / 1 / 2 / odd / even voiced counts, equal values and values that differ in the last mantissa byte.

The chain: for every stage-A set, and for a 6 s sustained tone whose 1197 frames are one run (asserted on the oracle: longer than PT_CAP, the
branch that back-tracks through global memory), the device's own candidates go through ``path_finder`` on the host and the result equals the
device's f0 and strength of pce_pitch_fetch in every frame, under the same gap precondition on the device's candidates.  With stage A that
closes the path from samples to track.

MEASURED (MI355X; worst |got - want| / bound over every slot of every frame of the set; cand_s stays below 1e-3 of its bound and the intensities
equal the oracle's bit for bit in every set; edges counted in the oracle's output):
  set           cand_f seeded  cand_f praat   frames  candidates  rare frames  f > 0.3 rate  lag <= 8  within 0.03 of a sample  local peak 0  full, no replacement
  16k-150       0.457          0.0001         1021    6135        270          351           795       598                      27            11
  16k-75        0.346          < 1e-4         506     3567        182          173           367       407                      12            5
  8k-150        0.491          0.0013         921     4683        159          334           836       288                      27            21
  8k-75         0.376          0.0002         456     2980        128          103           241       350                      12            3
  44k1-150      0.379          0.0388         418     2004        79           56            213       166                      27            0
  44k1-75       0.413          0.0004         204     1179        39           27            104       188                      12            3
  48k-50        0.219          < 1e-4         134     893         23           17            60        172                      7             1
  16k-150-c16   0.457          0.0001         1021    6405        255          354           805       608                      27            15
The smallest replacement margin of any frame is 6.4e-6 (16k-150), the smallest gap of a decision on the oracle's candidates 5.5e-6 against bounds
below 1e-10.  Stage B, the chain and the 1197-frame run: every back-pointer, every frame and every summary as stated, 23 batches.
First run, before the two fixes this file brought about: in the seeded mode cand_f stood at 1.03 (8k-75), 1.83 (44k1-150), 3.80 (44k1-75) and 5.10
(48k-50) times its bound on candidates of short lag of the speech excerpts (k_pitch_refine now replays Praat's iterates where the minimiser's tolerance exceeds 1e-6 of
the lag), and the clip of zeros read NaN as the intensity of every frame (0 / 0 in k_pitch_frames, which now stores 0).
"""
import math

import numpy as np
import pytest

import pitch_cases as PC
from pitch_restatement import gap_bound, path_finder

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
K = PC.K

def _engine_pitch_params(form_id):
    from prosody_control_french_tts_amd import PitchParams
    rate, floor, maxc, _, _ = PC.FORMS[form_id]
    p = PitchParams.praat(floor, PC.CEILING)
    p.max_candidates = maxc
    return p


def _chain(dev_f, dev_s, dev_n, dev_i, f0, strength, dt, p, ceiling, label):
    """The device's candidates through the host restatement are the device's track; the decisions on them clear the gap bound."""
    r = path_finder(dev_f, dev_s, dev_n, dev_i, dt, p, ceiling=ceiling)
    assert r["min_gap"] > gap_bound(len(dev_n), r["max_abs_delta"]), (label, r["min_gap"])
    assert np.array_equal(r["f0"], f0) and np.array_equal(r["strength"], strength), (label, np.flatnonzero(r["f0"] != f0)[:8])


def _check_summary(row, f0, label):
    v = f0[f0 > 0]
    assert row["n_frames"] == len(f0) and row["n_voiced"] == len(v), (label, row, len(v))
    if len(v) == 0:
        assert row["median_f0"] == 0.0 and row["mean_log_f0"] == 0.0, (label, row)
        return
    assert row["median_f0"] == np.median(v), (label, row["median_f0"], np.median(v))
    logs = [math.log(x) for x in v]
    want = math.fsum(logs) / len(v)
    bound = (len(v) + 2) * U * (math.fsum(abs(x) for x in logs) / len(v))
    assert abs(row["mean_log_f0"] - want) <= bound, (label, row["mean_log_f0"], want, bound)


@pytest.mark.parametrize("mode", ["seeded", "praat"])
@pytest.mark.parametrize("form_id", list(PC.FORMS))
def test_candidates_against_the_oracle_and_the_chain_to_the_track(engine, form_id, mode):
    rate, floor, maxc, _, _ = PC.FORMS[form_id]
    cnt = PC.assert_stage_a_preconditions(form_id)
    ora = PC.oracle(form_id)
    engine.pitch_set_refine(mode)
    try:
        engine.upload([c for _, c, _ in ora], rate)
        engine.pitch_run(engine.whole_clip_slices(), _engine_pitch_params(form_id))
        dev = engine.pitch_fetch_candidates()
        res = engine.pitch_fetch(want_strength=True)
    finally:
        engine.pitch_set_refine("seeded")
    off = dev["frame_offsets"]
    worst = dict(cand_f=0.0, cand_s=0.0, intensity=0.0)                  # for the printed figure; np.max carries a NaN through
    failed = []                                                          # (bound, clip) pairs with an element over its bound or not finite

    def hold(key, ratio, label):
        if ratio.size:
            worst[key] = float(np.max([worst[key], np.max(ratio)]))
            if not np.all(ratio <= 1.0):                                  # elementwise: a NaN is not <= 1
                failed.append((key, label, int(np.count_nonzero(~(ratio <= 1.0)))))
    for i, (name, c, w) in enumerate(ora):
        a, b = int(off[i]), int(off[i + 1])
        label = (form_id, mode, name)
        if w is None:                                                     # Praat refuses the length: no frames, and the status says so
            assert a == b and res["summary"][i]["status"] != 0, label
            continue
        nF, mc = w["cand_f"].shape
        assert b - a == nF and mc == maxc and res["summary"][i]["status"] == 0, label
        n = dev["ncand"][a:b]; cf = dev["cand_f"][a:b]; cs = dev["cand_s"][a:b]
        assert np.array_equal(n, w["ncand"]), (label, np.flatnonzero(n != w["ncand"])[:8])
        live = np.arange(K)[None, :] < n[:, None]
        assert np.all(np.isnan(cf[~live])) and np.all(np.isnan(cs[~live])), label           # the prefill beyond ncand
        assert np.all(cf[:, 0] == 0.0) and np.all(cs[:, 0] == 0.0), label
        want_f = np.zeros((nF, K)); want_s = np.zeros((nF, K))
        want_f[:, :mc] = w["cand_f"]; want_s[:, :mc] = w["cand_s"]
        real = live & (np.arange(K)[None, :] >= 1)
        di, wi = dev["intensity"][a:b], w["intensity"]
        assert np.all(np.isfinite(cf[real])) and np.all(np.isfinite(cs[real])) and np.all(np.isfinite(di)), label
        hold("cand_f", np.abs(cf[real] - want_f[real]) / (1e-6 * want_f[real]), label)
        hold("cand_s", np.abs(cs[real] - want_s[real]) / 1e-6, label)
        assert np.all(di[wi == 0.0] == 0.0), label
        hold("intensity", np.abs(di - wi)[wi > 0] / (8 * U * wi[wi > 0]), label)
        # the chain
        _chain(cf, cs, n, di, res["f0"][a:b], res["strength"][a:b], w["plan"].dt, PC.params(form_id), w["plan"].ceiling, label)
        _check_summary(res["summary"][i], res["f0"][a:b], label)
    print("stage A", form_id, mode, "worst |got - want| / bound:", {k: round(v, 4) for k, v in worst.items()}, "edges:", cnt)
    assert not failed and all(v <= 1.0 for v in worst.values()), (form_id, mode, worst, failed)


def test_sustained_tone_is_one_long_run_through_a_real_analysis(engine):
    """A run of more than PT_CAP frames reaches k_pitch_path's back-tracking through global memory from samples."""
    from prosody_control_french_tts_amd import PitchParams
    c = PC.sustained_tone()
    w = PC.O.pitch_ac(c.astype(np.float64) / 32768.0, 1.0 / 16000, 0.5 / 16000, PC.params("16k-150"), want_candidates=True)
    assert PC.longest_run(w["ncand"]) == len(w["ncand"]) > 1024
    engine.upload([c], 16000)
    engine.pitch_run(engine.whole_clip_slices(), PitchParams.praat(150.0, PC.CEILING))
    dev = engine.pitch_fetch_candidates()
    res = engine.pitch_fetch(want_strength=True)
    assert np.array_equal(dev["ncand"], w["ncand"])
    _chain(dev["cand_f"], dev["cand_s"], dev["ncand"], dev["intensity"], res["f0"], res["strength"], w["plan"].dt, PC.params("16k-150"),
           w["plan"].ceiling, "tone")
    v = w["f0"] > 0
    assert np.array_equal(res["f0"] > 0, v) and np.max(np.abs(res["f0"][v] - w["f0"][v]) / w["f0"][v]) < 1e-6
    _check_summary(res["summary"][0], res["f0"], "tone")


# ------------------------------------------------------------------------------------------------------------------ stage B

def _run_batch(engine, name):
    p, dt, slices = PC.batches()[name]
    off, n, inten, cf, cs = PC.concat(slices)
    got = engine.selftest_pitch_path(PC.engine_params(p), dt, off, n, inten, cf, cs)
    return off, n, got


@pytest.mark.parametrize("name", list(PC.batches()))
def test_path_finder_and_medians_on_given_candidates(engine, name):
    exp = PC.expected(name)
    labels = [c[0] for c in PC.exact_cases()] if name == "exact" else [None] * len(exp)
    for label, r in zip(labels, exp):                                    # the precondition, on CPU values alone
        if label not in ("tie-at-threshold", "just-above-threshold"):
            assert r["min_gap"] > r["bound"], (name, label, r["min_gap"], r["bound"])
    off, n, got = _run_batch(engine, name)
    for i, r in enumerate(exp):
        a, b = int(off[i]), int(off[i + 1])
        label = (name, i, labels[i])
        assert np.array_equal(got["f0"][a:b], r["f0"]), (label, np.flatnonzero(got["f0"][a:b] != r["f0"])[:8])
        assert np.array_equal(got["strength"][a:b], r["strength"]), label
        Kr = r["psi"].shape[1]
        ns = n[a:b]
        live = (np.arange(Kr)[None, :] < ns[:, None]) & (ns[:, None] > 1)
        gp = got["psi"][a:b, :Kr].astype(np.int64)
        assert np.array_equal(gp[live], r["psi"][live]), (label, np.argwhere(live & (gp != r["psi"]))[:8])
        _check_summary(got["summary"][i], r["f0"], label)
    if name == "exact":                                                  # ... and the numbers worked out by hand
        for i, (label, _, f0, psi) in enumerate(PC.exact_cases()):
            a = int(off[i])
            assert np.array_equal(got["f0"][a:int(off[i + 1])], f0), (label, got["f0"][a:int(off[i + 1])], f0)
            for (t, c), want in psi.items():
                if n[a + t] > 1:
                    assert got["psi"][a + t, c] == want, (label, t, c)


def test_a_long_run_alone_equals_the_same_run_in_the_batch(engine):
    """1025 and 2049 frames alone in a call and among the 35 slices of the ladder: the same track and back-pointers."""
    off, n, all_ = _run_batch(engine, "ladder")
    for L in (1025, 2049):
        i = PC.LADDER.index(L)
        _, _, alone = _run_batch(engine, f"alone-{L}")
        a, b = int(off[i]), int(off[i + 1])
        live = np.arange(K)[None, :] < n[a:b, None]
        assert b - a == L and np.array_equal(alone["f0"], all_["f0"][a:b]) and np.array_equal(alone["psi"][live], all_["psi"][a:b][live])


def test_selftest_refuses_what_the_kernels_cannot_take_and_gives_the_buffers_back(engine):
    from prosody_control_french_tts_amd import PceError, PitchParams
    cf, cs, n, inten = PC.random_slice(np.random.default_rng(5), 6)
    p = PC.engine_params(PC.path_params())
    for bad in (0, 17, -1):
        m = n.copy(); m[3] = bad
        with pytest.raises(PceError):
            engine.selftest_pitch_path(p, 0.01, [0, 6], m, inten, cf, cs)
    with pytest.raises(PceError):
        engine.selftest_pitch_path(PC.engine_params(PC.path_params(max_candidates=17)), 0.01, [0, 6], n, inten, cf, cs)
    with pytest.raises(PceError):
        engine.selftest_pitch_path(p, 0.0, [0, 6], n, inten, cf, cs)
    with pytest.raises(PceError):
        engine.selftest_pitch_path(p, 0.01, [0, 4, 3, 6], n, inten, cf, cs)
    # a resident analysis: the hook works in its buffers, the fetch is refused afterwards, and the next run plans afresh and returns the same
    from prosody_control_french_tts_amd import synth
    engine.upload([synth.synth_clip(3, seconds=1.0)], 16000)
    pp = PitchParams.praat(150.0, 600.0)
    before = engine.pitch(engine.whole_clip_slices(), pp, want_strength=True)
    cand = engine.pitch_fetch_candidates()
    engine.selftest_pitch_path(p, 0.01, [0, 2, 2, 6], n, inten, cf, cs)          # an empty slice beside two real ones
    with pytest.raises(PceError):
        engine.pitch_fetch()
    with pytest.raises(PceError):
        engine.pitch_fetch_candidates()
    after = engine.pitch(engine.whole_clip_slices(), pp, want_strength=True)
    assert np.array_equal(before["f0"], after["f0"]) and np.array_equal(before["strength"], after["strength"])
    again = engine.pitch_fetch_candidates()
    for k in ("ncand", "intensity"):
        assert np.array_equal(cand[k], again[k])
    assert np.array_equal(cand["cand_f"], again["cand_f"], equal_nan=True) and np.array_equal(cand["cand_s"], again["cand_s"], equal_nan=True)
