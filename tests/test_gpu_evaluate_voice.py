"""``pce_dtw_series`` and ``Pipeline/evaluate_voice.py`` on the device against the plain restatements of
tests/test_evaluate_voice_host.py.  Paths and distances are compared EXACTLY: the arithmetic is float64 adds and compares in a fixed
order (include/pce.h), there is no tolerance to choose."""
import json
import struct

import numpy as np
import pytest

from prosody_control_french_tts_amd import engine as E
from prosody_control_french_tts_amd import synth
from prosody_control_french_tts_amd.Pipeline import evaluate_voice as EV
from prosody_control_french_tts_amd.visualisation.acoustic_analysis import pyin_plan
from tests.test_evaluate_voice_host import (EMPTY, NO_PATH, OK, WER_CASES, random_monotone_path, random_walk, ref_dtw, ref_edit_distance,
                                            ref_fastdtw, ref_rmse)

pytestmark = pytest.mark.gpu
R, C = E.DTW_SERIES_ROWS, E.DTW_SERIES_COLS


def bits(x):
    return struct.pack("<d", x)


def assert_same(got, want, what=""):
    path, dist, status = got
    want_path, want_dist, want_status = want
    assert status == want_status, what
    assert bits(dist) == bits(want_dist) or (np.isnan(dist) and np.isnan(want_dist)), (what, dist, want_dist)
    assert path.shape == want_path.shape and np.array_equal(path, want_path), what


def quantised(rng, n):
    """A log-F0 contour on pYIN's own pitch grid (the frequencies ``pyin_plan`` returns): many exactly equal values."""
    freqs = pyin_plan(22050, EV.C2_HZ, EV.C6_HZ, hop_length=512)[2]
    idx = np.clip(len(freqs) // 2 + np.cumsum(rng.integers(-2, 3, n)), 0, len(freqs) - 1)
    return np.log(freqs[idx])


def test_exact_tile_edges(engine):
    rng = np.random.default_rng(1)
    sizes = [(1, 1), (1, 37), (41, 1)] + [(n, m) for n in (R - 1, R, R + 1, C - 1, C, C + 1) for m in (R - 1, R, R + 1, C - 1, C, C + 1)]
    pairs = [(random_walk(rng, n), random_walk(rng, m)) for n, m in sizes]
    got = engine.dtw_series(pairs)
    for (a, b), g, s in zip(pairs, got, sizes):
        assert_same(g, ref_dtw(a, b), s)


def test_exact_ragged_batch_and_kinds_of_series(engine):
    rng = np.random.default_rng(2)
    sizes = [(1, 1), (5000, 7000), (7000, 1), (3, 2999), (0, 50), (1500, 1500), (2049, 1025), (64, 65), (700, 0), (2500, 4100), (1, 7000), (333, 4097), (1025, 1025)]
    kinds = [random_walk, lambda r, n: np.full(n, 5.25), quantised]
    pairs = [(kinds[k % 3](rng, n), kinds[k % 3](rng, m)) for k, (n, m) in enumerate(sizes)]
    got = engine.dtw_series(pairs)
    assert len(got) >= 12
    for (a, b), g, s in zip(pairs, got, sizes):
        assert_same(g, ref_dtw(a, b), s)
    for k in (4, 8):
        assert got[k][2] == EMPTY and got[k][0].shape == (0, 2) and np.isnan(got[k][1])
    # all ties (pair 7 is constant): "up" is the first candidate and wins wherever it is finite, so the walk back from (63, 64) climbs the
    # last column to row 0 and then follows row 0 -- the path runs along row 0 first, then down the last column
    assert np.array_equal(got[7][0], np.array([(0, j) for j in range(65)] + [(i, 64) for i in range(1, 64)])) and got[7][1] == 0.0


def random_window(rng, n, m, slack):
    path = random_monotone_path(rng, n, m)
    lo = np.full(n, m); hi = np.zeros(n, int)
    np.minimum.at(lo, path[:, 0], path[:, 1]); np.maximum.at(hi, path[:, 0], path[:, 1] + 1)
    lo = np.maximum.accumulate(np.clip(lo - rng.integers(0, slack, n), 0, m))
    hi = np.maximum.accumulate(np.clip(hi + rng.integers(0, slack, n), 0, m))
    return lo.astype(np.int32), hi.astype(np.int32)


def test_windowed(engine):
    rng = np.random.default_rng(3)
    sizes = [(2500, 4500, 40), (1100, 2100, 3), (300, 200, 1), (2049, 6200, 700)]
    pairs = [(random_walk(rng, n), quantised(rng, m)) for n, m, _ in sizes]
    wins = [random_window(rng, n, m, s) for n, m, s in sizes]
    # the band of a real fastdtw level
    x, y = random_walk(rng, 3000), random_walk(rng, 2600)
    coarse = engine.dtw_series([(EV.reduce_by_half(x), EV.reduce_by_half(y))])[0][0]
    pairs.append((x, y)); wins.append(EV.expand_window(coarse, len(x), len(y), 25))
    pairs.append((random_walk(rng, 1200), random_walk(rng, 900))); wins.append(None)           # a pair without a window beside them
    got = engine.dtw_series(pairs, wins)
    for k, ((a, b), w, g) in enumerate(zip(pairs, wins, got)):
        assert_same(g, ref_dtw(a, b, *(w if w is not None else (None, None))), k)
        assert g[2] == OK


def test_window_without_a_path_leaves_the_other_pairs_alone(engine):
    rng = np.random.default_rng(4)
    pairs = [(random_walk(rng, n), random_walk(rng, m)) for n, m in [(1300, 2300), (1500, 2500), (90, 70), (2100, 5000)]]
    full = [(np.zeros(len(a), np.int32), np.full(len(a), len(b), np.int32)) for a, b in pairs]
    lo1, hi1 = full[1]
    hi1 = hi1.copy(); hi1[-1] = len(pairs[1][1]) - 1                           # (n - 1, m - 1) is outside
    lo3 = full[3][0].copy(); hi3 = full[3][1].copy(); lo3[1024:] = 4096; hi3[:1024] = 2048      # the last tile is never swept, nor its neighbours
    wins = [None, (lo1, hi1), full[2], (lo3, hi3)]
    got = engine.dtw_series(pairs, wins)
    for k in (1, 3):
        assert got[k][2] == NO_PATH and got[k][0].shape == (0, 2) and got[k][1] == np.inf
        assert ref_dtw(*pairs[k], *wins[k])[2] == NO_PATH
    for k in (0, 2):
        assert_same(got[k], ref_dtw(*pairs[k]), k)


def test_bad_arguments_are_refused(engine):
    with pytest.raises(E.PceError):
        engine.dtw_series([(np.array([1.0, np.nan]), np.array([1.0]))])
    with pytest.raises(E.PceError):
        engine.dtw_series([(np.array([1.0]), np.array([np.inf, 2.0]))])
    with pytest.raises(E.PceError):
        engine.dtw_series([(np.ones(3), np.ones(4))], [(np.zeros(3, np.int32), np.full(3, 5, np.int32))])
    assert engine.dtw_series([]) == []


def test_large_pair_alone_and_in_a_batch(engine):
    rng = np.random.default_rng(5)
    n, m = 40000, 36000
    a, b = random_walk(rng, n), random_walk(rng, m)
    path, dist, status = engine.dtw_series([(a, b)])[0]
    assert status == OK and tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n - 1, m - 1)
    steps = np.diff(path, axis=0)
    assert set(map(tuple, steps.tolist())) <= {(1, 0), (0, 1), (1, 1)}
    total = 0.0
    for v in np.abs(a[path[:, 0]] - b[path[:, 1]]).tolist():                    # the same chain of additions the kernel made
        total += v
    assert bits(total) == bits(dist)
    fast_dist, fast_path = EV.fastdtw(a, b, 25, engine)
    assert dist <= fast_dist and tuple(fast_path[-1]) == (n - 1, m - 1)
    others = [(random_walk(rng, 3000), random_walk(rng, 5000)), (random_walk(rng, 10), random_walk(rng, 2)),
              (random_walk(rng, 9000), random_walk(rng, 1000)), (random_walk(rng, 2048), random_walk(rng, 1024))]
    batch = engine.dtw_series(others[:2] + [(a, b)] + others[2:])
    assert bits(batch[2][1]) == bits(dist) and np.array_equal(batch[2][0], path) and batch[2][2] == OK
    for k, (x, y) in zip((0, 1, 3, 4), others):
        alone = engine.dtw_series([(x, y)])[0]
        assert np.array_equal(batch[k][0], alone[0]) and bits(batch[k][1]) == bits(alone[1])


def test_fastdtw_on_the_device_equals_the_pure_restatement(engine):
    rng = np.random.default_rng(6)
    pairs = [(random_walk(rng, 3000), random_walk(rng, 2500)), (quantised(rng, 700), quantised(rng, 901)), (random_walk(rng, 26), random_walk(rng, 400)),
             (random_walk(rng, 27), random_walk(rng, 27)), (np.full(333, 5.0), np.full(280, 5.0))]
    got = EV.fastdtw_batch(pairs, 25, engine)
    for k, ((x, y), (dist, path)) in enumerate(zip(pairs, got)):
        want_dist, want_path = ref_fastdtw(x, y, 25)
        assert bits(dist) == bits(want_dist) and np.array_equal(path, want_path), k
    one = EV.fastdtw(*pairs[1], radius=25, engine=engine)
    assert bits(one[0]) == bits(got[1][0]) and np.array_equal(one[1], got[1][1])


def test_contour_level_rmse(engine):
    rng = np.random.default_rng(7)
    f = 200.0 * 2.0 ** np.cumsum(rng.normal(0.0, 0.01, 1800))
    f[100:160] = np.nan; f[900:930] = np.nan
    for method in ("fastdtw", "exact"):
        assert EV.f0_contour_rmse(f, f, method=method, engine=engine) == 0.0
        c = np.full(1400, 180.0); c2 = np.full(1733, 180.0 * 2.0 ** (1 / 12))
        assert abs(EV.f0_contour_rmse(c, c2, method=method, engine=engine) - np.log(2.0) / 12) <= 1e-12
        assert np.isnan(EV.f0_contour_rmse(np.full(50, np.nan), f, method=method, engine=engine))
        assert np.isnan(EV.f0_contour_rmse(f, np.full(50, np.nan), method=method, engine=engine))
    # NaN frames are dropped BEFORE the DTW: the same contour with more unvoiced frames in other places scores the same
    g = 210.0 * 2.0 ** np.cumsum(rng.normal(0.0, 0.01, 1500))
    f_holes = np.insert(f, [5, 5, 700], np.nan)
    got = EV.f0_contour_rmse_batch([(f, g), (f_holes, g)], engine=engine)
    assert got[0] == got[1] == ref_rmse(f, g)
    assert EV.f0_contour_rmse(f, g, method="exact", engine=engine) == ref_rmse(f, g, exact=True)


def test_audio_level_rmse(engine):
    sr = 16000
    c0, c1 = synth.synth_clip(40, seconds=9.0, rate=sr), synth.synth_clip(41, seconds=8.0, rate=sr)
    silence = np.zeros(8 * sr, np.int16)
    f0 = EV.extract_f0_batch(engine, [c0, c1], sr)
    assert np.isfinite(f0[0]).sum() > 50 and np.isfinite(f0[1]).sum() > 50
    assert EV.compute_f0_rmse(engine, c0, c1, sr) == ref_rmse(f0[0], f0[1])
    assert EV.compute_f0_rmse(engine, c0, c1, sr, method="exact") == ref_rmse(f0[0], f0[1], exact=True)
    assert EV.compute_f0_rmse(engine, c0, c0, sr) == 0.0
    assert np.isnan(EV.compute_f0_rmse(engine, c0, silence, sr)) and np.isnan(EV.compute_f0_rmse(engine, silence, c1, sr))
    # floating-point audio in [-1, 1) is the same recording
    assert EV.compute_f0_rmse(engine, c0 / 32768.0, c1.astype(np.float32) / 32768.0, sr) == ref_rmse(f0[0], f0[1])


def test_wer_through_the_device(engine):
    for ref, hyp, want in WER_CASES:
        assert EV.compute_wer(ref, hyp, engine) == want
    with pytest.raises(ValueError):
        EV.compute_wer("  ", "un mot", engine)
    rng = np.random.default_rng(8)
    vocab = ["le", "la", "les", "un", "une", "chat", "chien", "maison", "voilà", "très", "été", "où", "ça", "mange", "dort", "aujourd'hui", "et", "ou", "mais"]
    pairs = []
    for _ in range(200):
        ref = [vocab[i] for i in rng.integers(0, len(vocab), rng.integers(1, 120))]
        hyp = [w for w in ref if rng.random() > 0.1]
        for _ in range(rng.integers(0, 8)):
            hyp.insert(rng.integers(0, len(hyp) + 1), vocab[rng.integers(0, len(vocab))])
        pairs.append((" ".join(ref), "  ".join(hyp)))
    got = EV.compute_wer_batch(pairs, engine)
    assert got == [ref_edit_distance(r.split(), h.split()) / len(r.split()) for r, h in pairs]


def test_evaluate_all_on_three_episodes(engine, tmp_path):
    from tests.test_gpu_aligner import write_model_dir
    from tests.test_gpu_c5 import WORDS, write_wav
    model_root = tmp_path / "whisper_dir"
    write_model_dir(model_root, merges=WORDS, word_gain=3.0, eot_gain=0.3)
    model = EV.WhisperHandle.load(engine, "medium", str(model_root))
    voice, results, save = tmp_path / "voice", tmp_path / "results", tmp_path / "evaluation"
    audio = {}
    for k, ep in enumerate(["EP01", "EP02", "EP03"]):
        ref = synth.synth_clip(60 + k, seconds=9.0 + k, rate=22050)
        write_wav(voice / ep / "brute" / "segment_demucs.wav", ref, 22050)
        (results / ep).mkdir(parents=True)
        if ep != "EP02":
            write_wav(results / ep / "OUT.wav", synth.synth_clip(70 + k, seconds=8.0 + k, rate=16000), 16000)       # resampled to 22 050 Hz
        audio[ep] = ref
    df = EV.evaluate_all(voice, results, save, engine=engine, model=model)
    assert list(df.index) == ["EP01", "EP03"] and df.index.name == "episode" and list(df.columns) == ["rmse_f0", "f1_break", "wer"]
    for ep in ("EP01", "EP03"):
        d = save / ep
        assert sorted(p.name for p in d.iterdir()) == sorted(EV.SIDE_FILES)
        rate_r, y_ref = EV.H.decode_wav(d / "reference.wav")
        rate_s, y_sys = EV.H.decode_wav(d / "synthetic.wav")
        assert rate_r == rate_s == 22050 and np.array_equal(y_ref, audio[ep])
        f0 = EV.extract_f0_batch(engine, [y_ref, y_sys], 22050)
        want_rmse = ref_rmse(f0[0], f0[1])
        assert df.loc[ep, "rmse_f0"] == want_rmse or (np.isnan(want_rmse) and np.isnan(df.loc[ep, "rmse_f0"]))
        ref_txt = (d / "reference_transcript.txt").read_text(encoding="utf-8"); sys_txt = (d / "synthetic_transcript.txt").read_text(encoding="utf-8")
        assert df.loc[ep, "wer"] == ref_edit_distance(EV.wer_words(ref_txt), EV.wer_words(sys_txt)) / len(EV.wer_words(ref_txt))
        br = [[float(v) for v in (d / f"{side}_breaks.txt").read_text().split()] for side in ("reference", "synthetic")]
        segs = [json.loads((d / f"{side}_segments.json").read_text()) for side in ("reference", "synthetic")]
        for b, s in zip(br, segs):
            assert b == [x["end"] for x in s[:-1]] and all(set(x) == {"start", "end", "text"} for x in s)
        assert df.loc[ep, "f1_break"] == EV.compute_f1_break(br[0], br[1], tol=0.3)[0]
    # the episode without OUT.wav is reported and skipped; its reference side was still written
    assert {"reference.wav", "reference_transcript.txt"} <= {p.name for p in (save / "EP02").iterdir()} and not (save / "EP02" / "synthetic.wav").exists()
