"""pce_silence_* on the device against the integer restatement (tests/silence_restatement.py): every comparison exact.

Sizes of the scan levels (csrc/pce_silence.hip): k_ms_energy scans 256 bins per workgroup and k_silence_scan carries over tiles of 64 chunks
(16 384 bins); the range pass takes 1 024 window starts per workgroup and carries over tiles of 64 of those (65 536 starts).  The long clip
(135 s at 16 kHz, 4.3 MB) has 135 001 prefix entries -- 528 chunks, 9 carry tiles -- and at min_silence_len 40, step 1, 134 961 starts: 132
tiles, 3 carry tiles."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silence_restatement as R
from prosody_control_french_tts_amd import hostrules as H
from prosody_control_french_tts_amd.engine import SLICE_EMPTY, SLICE_OK, PceError, make_slices

pytestmark = pytest.mark.gpu

RATES = (16000, 22050, 44100)
RUNS = ((1000, 1), (100, 1), (40, 1), (250, 7))
LONG_SECONDS = 135


@functools.lru_cache(maxsize=None)
def long_clip():
    rng = np.random.default_rng(11)
    plan, total = [], 0
    while total < LONG_SECONDS * 1000:
        plan += [(int(rng.integers(30, 1500)), 0), (int(rng.integers(1, 400)), 1)]
        total += plan[-2][0] + plan[-1][0]
    return R.bursts(16000, plan, 12)[:LONG_SECONDS * 16000]


@functools.lru_cache(maxsize=None)
def batch(rate):
    """-> (clips, slices as (clip, begin, end)): every case clip whole, then slices that begin before a clip, run past its end, lie outside
    it, and empty ones."""
    cases = R.case_clips(rate)
    names = list(cases)
    clips = [cases[k] for k in names]
    if rate == 16000:
        names.append("long"); clips.append(long_clip())
    sl = [(i, 0, len(c)) for i, c in enumerate(clips)]
    g, t = names.index("gaps"), names.index("lead_tail")
    sl += [(g, -rate // 3, len(clips[g]) // 2), (g, 1234, len(clips[g]) + 777), (t, -5, len(clips[t]) + 5 + rate // 2), (t, 999, 999),
           (g, len(clips[g]) + 10, len(clips[g]) + 10 + rate), (t, -rate, 0), (names.index("straddle"), 3, 2 * rate + 1), (g, 0, 0)]
    return clips, sl


@functools.lru_cache(maxsize=None)
def expected(rate, L, step, T=103):
    clips, sl = batch(rate)
    return [R.detect_silence(R.slice_samples(clips[c], b, e), rate, L, T=T, step=step) for c, b, e in sl]


def run(engine, rate, clips, sl, L, step, rms_max=103, channels=1):
    engine.upload(clips, rate)
    c, b, e = zip(*sl)
    engine.silence_run(make_slices(c, b, e), rms_max, L, step, channels)
    res = engine.silence_fetch()
    off = res["range_offsets"]
    return [res["ranges"][off[i]:off[i + 1]].tolist() for i in range(len(sl))], res


@pytest.mark.parametrize("L,step", RUNS)
@pytest.mark.parametrize("rate", RATES)
def test_batch_matches_the_restatement(engine, rate, L, step):
    clips, sl = batch(rate)
    got, res = run(engine, rate, clips, sl, L, step)
    want = expected(rate, L, step)
    assert res["len_ms"].tolist() == [w[1] for w in want]
    assert res["status"].tolist() == [SLICE_EMPTY if e == b else SLICE_OK for _, b, e in sl]
    assert np.diff(res["range_offsets"]).tolist() == [len(w[0]) for w in want]
    for i, w in enumerate(want):
        assert got[i] == w[0], (sl[i], L, step)
    assert sum(len(w[0]) for w in want) > 5 and any(w[0] == [] and w[1] >= L for w in want) and any(w[0] == [[0, w[1]]] for w in want)


def test_a_clip_alone_and_in_the_batch_gives_the_same_ranges(engine):
    clips, sl = batch(16000)
    k = len(clips) - 1
    in_batch, _ = run(engine, 16000, clips, sl, 40, 1)
    alone, _ = run(engine, 16000, [clips[k]], [(0, 0, len(clips[k]))], 40, 1)
    assert alone[0] == in_batch[k] == expected(16000, 40, 1)[k][0] and len(alone[0]) > 100


def test_per_slice_thresholds_from_the_energy_kernel(engine):
    """The strip of synthesis padding (Code/audioPipeline.py:786-797): detect_nonsilent(min_silence_len=40, silence_thresh=seg.dBFS - 30) per file.
    The threshold lies 30 dB under the file's rms and the tone's rms is above the file's, so a 40 ms window may hold 40 * 10^-3 ms of tone
    and stay silent: the nonsilent extent is the tone's, to the millisecond."""
    rate = 22050
    clips, tones = [], []
    for i, (lead, dur, tail, amp) in enumerate(((300, 700, 450, 20000), (120, 1500, 95, 900), (41, 333, 1000, 60))):
        t = np.arange(int(dur * rate / 1000)) / rate
        tone = np.round(amp * np.sign(np.sin(2 * np.pi * 441.0 * t + 0.1))).astype(np.int16)      # a square wave: every sample at the amplitude
        clips.append(np.concatenate([np.zeros(lead * rate // 1000, np.int16), tone, np.zeros(tail * rate // 1000, np.int16)]))
        tones.append((lead, lead + dur))
    engine.upload(clips, rate)
    sl = engine.whole_clip_slices()
    en = engine.energy(sl)
    thresh = [H.pydub_dbfs(int(e["sum_sq"]), int(e["n"])) - 30 for e in en]
    assert len(set(H.silence_rms_max(t) for t in thresh)) == 3
    got = engine.detect_nonsilent(sl, min_silence_len=40, silence_thresh=thresh)
    for i, c in enumerate(clips):
        silent, len_ms = R.detect_silence(c, rate, 40, silence_thresh=thresh[i])
        assert got[i] == H.nonsilent_from_silent(silent, len_ms)
        assert len(got[i]) == 1 and abs(got[i][0][0] - tones[i][0]) <= 1 and abs(got[i][0][1] - tones[i][1]) <= 1
    assert engine.detect_silence(sl, 40, thresh) == [R.detect_silence(c, rate, 40, silence_thresh=t)[0] for c, t in zip(clips, thresh)]


def test_two_channels_against_the_literal_loop(engine):
    rate = 16000
    x = R.bursts(rate, [(310, 0), (200, 1), (500, 0), (3, 1), (400, 0), (350, 1), (237, 0)], 21, channels=2)
    x[1::2] //= 3                                                       # the channels differ
    for L, step in ((100, 1), (250, 7)):
        want = R.detect_silence_literal(x, rate, L, -50, step, channels=2)
        assert want == R.detect_silence(x, rate, L, step=step, channels=2, silence_thresh=-50) and len(want[0]) >= 2
        engine.upload([x, x[:-2]], rate)
        sl = make_slices([0, 1, 0], [0, 0, 400], [len(x), len(x) - 2, len(x) + 4000])
        got = engine.detect_silence(sl, L, -50, step, channels=2)
        assert got[0] == want[0]
        assert got[1] == R.detect_silence_literal(x[:-2], rate, L, -50, step, channels=2)[0]
        assert got[2] == R.detect_silence_literal(R.slice_samples(x, 400, len(x) + 4000), rate, L, -50, step, channels=2)[0]
        ms, frames = engine.split_on_silence(sl[:1], L, -50, step, keep_silence=30, channels=2)
        cut = H.split_ranges(H.nonsilent_from_silent(want[0], want[1]), 30, want[1])
        assert ms[0] == cut and frames[0] == [H.pydub_slice_frames(len(x) // 2, rate, a, b) for a, b in cut]


def test_error_returns(engine):
    engine.upload([np.zeros(1000, np.int16)], 16000)
    engine._si_n = 1
    with pytest.raises(PceError, match="status -4"):
        engine.silence_fetch()
    sl = engine.whole_clip_slices()
    for kw in (dict(min_silence_len=0), dict(seek_step=0), dict(channels=0), dict(rms_max=-1)):
        args = dict(rms_max=103, min_silence_len=10, seek_step=1, channels=1); args.update(kw)
        with pytest.raises(PceError, match="status -1"):
            engine.silence_run(sl, **args)
    for b, e in ((1, 1000), (0, 999), (-3, 1000)):
        with pytest.raises(PceError, match="status -1"):
            engine.silence_run(make_slices([0], [b], [e]), 103, 10, 1, 2)
    with pytest.raises(PceError, match="status -5"):
        engine.silence_run(make_slices([0], [0], [16 * 2 ** 31 + 16]), 103, 10, 1, 1)
    with pytest.raises(PceError, match="status -4"):                    # a failed run leaves nothing to fetch
        engine.silence_fetch()
    engine.silence_run(make_slices([0, 0], [0, 5], [1000, 5]), 103, 10, 1, 1)
    res = engine.silence_fetch()
    assert res["ranges"].tolist() == [[0, 62]] and res["len_ms"].tolist() == [62, 0] and res["status"].tolist() == [SLICE_OK, SLICE_EMPTY]


def test_preprocess_audio_end_to_end(engine, tmp_path):
    from prosody_control_french_tts_amd.Preprocessing import preprocess_audio as PA
    rate = 44100
    x = R.bursts(rate, [(1200, 0), (900, 1), (1500, 0), (400, 1), (1100, 0), (1300, 1), (1600, 0)], 31)
    src = tmp_path / "episode.wav"
    PA.Segment(x, rate).export(src)
    PA.main(str(src), str(tmp_path / "audio"), engine=engine)                    # the reference's defaults: 1000, -50, 300
    silent, len_ms = R.detect_silence(x, rate, 1000, silence_thresh=-50)
    cut = H.split_ranges(H.nonsilent_from_silent(silent, len_ms), 300, len_ms)
    assert len(cut) == 3 and len_ms == 8000
    assert sorted(os.listdir(tmp_path / "audio")) == ["segment_ph1.wav", "segment_ph2.wav", "segment_ph3.wav"]
    for i, (a, b) in enumerate(cut):
        f0, f1 = H.pydub_slice_frames(len(x), rate, a, b)
        r, ch, pcm = H.decode_wav_channels(tmp_path / "audio" / f"segment_ph{i + 1}.wav")
        assert (r, ch, len(pcm)) == (rate, 1, f1 - f0) and np.array_equal(pcm, R.slice_samples(x, f0, f1))
    y = R.bursts(16000, [(300, 1), (1100, 0), (200, 1), (1000, 0), (5, 1)], 32, channels=2)
    other = tmp_path / "stereo16k.wav"
    PA.Segment(y, 16000, 2).export(other)
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"nothing")
    res = PA.segment_audio_files([str(src), str(other), str(bad)], engine=engine)
    assert isinstance(res[str(bad)], H.CouldntDecodeError)
    assert [s.samples.tolist() for s in res[str(src)]] == [R.slice_samples(x, *H.pydub_slice_frames(len(x), rate, a, b)).tolist() for a, b in cut]
    silent, len_ms = R.detect_silence_literal(y, 16000, 1000, -50, channels=2)
    cut = H.split_ranges(H.nonsilent_from_silent(silent, len_ms), 300, len_ms)
    assert len(cut) == 3 and [(s.frame_rate, s.channels, len(s)) for s in res[str(other)]] == [(16000, 2, b - a) for a, b in cut]
    for s, (a, b) in zip(res[str(other)], cut):
        f0, f1 = H.pydub_slice_frames(len(y) // 2, 16000, a, b)
        assert np.array_equal(s.samples, R.slice_samples(y, 2 * f0, 2 * f1))
