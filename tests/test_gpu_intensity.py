"""GPU tests of Praat intensity on the device (pce_intensity_*, csrc/pce_intensity.hip) against the float64 restatement of
tests/intensity_restatement.py, and of visualisation/Compare_speech_noenhanced.py end to end.

Bounds (derived in intensity_restatement.py and the issue that asked for the kernel): contour 1e-9 dB absolute; mean_positive within
n 2^-52 relative of np.nanmean over the n positive values; frame counts, offsets, t1, status and n_positive exact."""
import math
import os
import wave

import numpy as np
import pytest

import intensity_restatement as R
import prosody_control_french_tts_amd as P
from prosody_control_french_tts_amd import hostrules as H
from prosody_control_french_tts_amd.engine import make_slices
from prosody_control_french_tts_amd.visualisation import Compare_speech_noenhanced as M

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
RATES = (16000, 44100)
# (pitch_floor, time_step, subtract_mean)
PARAMS = [(100.0, 0.0, True), (50.0, 0.0, True), (75.0, 0.0, True), (400.0, 0.0, True), (100.0, 0.0, False), (100.0, 0.01, True)]


def make_clips(rate):
    """1.3 s clips whose DC offset is of the order of their RMS: amplitude-modulated noise, a tone on an offset, silence, a constant,
    and isolated least-significant bits (levels below 0 dB, which the summary must leave out)."""
    rng = np.random.default_rng(rate)
    n = int(1.3 * rate) + 7
    t = np.arange(n) / rate
    am = (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) * rng.standard_normal(n) * 2500 + 2200
    tone = 6000 * np.sin(2 * np.pi * 187.0 * t) * (0.2 + 0.8 * t / t[-1]) - 5000
    sparse = (rng.random(n) < 0.05).astype(np.int16)
    loud = rng.standard_normal(n) * 9000 - 7000
    return [np.clip(np.round(x), -32768, 32767).astype(np.int16) for x in (am, tone, np.zeros(n), np.full(n, -1234.0), sparse, loud)]


def make_batch(rate, pitch_floor):
    clips = make_clips(rate)
    n = len(clips[0])
    n_min = math.ceil(6.4 / pitch_floor * rate)                         # shortest sound that holds one window
    assert H.intensity_frames(n_min, rate, 0.0, pitch_floor)[0] == 1 and H.intensity_frames(n_min - 1, rate, 0.0, pitch_floor)[0] == 0
    dx = 1.0 / rate
    rows = [(c, 0, n, 0.5 * dx) for c in range(len(clips))]              # whole clips
    rows += [(0, 777, 777 + n_min, 777.5 * dx),                         # exactly one window: one frame, begin != 0
             (5, 0, n_min - 1, 0.5 * dx),                               # a sample short, between live neighbours
             (1, 1001, 1001 + 2 * n_min + 37, 0.123),                   # its own x1
             (5, n - n_min - 300, n + 500, 0.5 * dx),                   # runs past its clip's end
             (0, -250, 3 * n_min + 11, -0.01),                          # starts before its clip
             (1, 40, 40, 0.0),                                          # empty
             (5, 5, 5 + n_min + 1, 0.5 * dx)]
    return clips, make_slices([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])


def check_against_restatement(res, clips, slices, rate, pitch_floor, time_step, subtract_mean):
    off, summ, vals = res["frame_offsets"], res["summary"], res["values"]
    worst = 0.0
    for i, s in enumerate(slices):
        x = R.slice_samples(clips[s["clip"]], int(s["begin"]), int(s["end"]))
        want, t1, status = R.intensity(x, rate, float(s["x1"]), pitch_floor, time_step, subtract_mean)
        got = vals[off[i]:off[i + 1]]
        assert summ["status"][i] == status and summ["n_frames"][i] == len(want) == len(got), i
        assert summ["t1"][i] == t1, (i, summ["t1"][i], t1)
        assert np.array_equal(got == -300.0, want == -300.0), i
        if len(want):
            worst = max(worst, float(np.max(np.abs(got - want))))
        assert summ["n_positive"][i] == np.sum(want > 0) == np.sum(got > 0), i
        pos = got[got > 0]
        if len(pos):
            assert abs(summ["mean_positive"][i] - np.nanmean(pos)) <= len(pos) * 2.0 ** -52 * np.nanmean(pos), i
        else:
            assert math.isnan(summ["mean_positive"][i]), i
    print(f"rate {rate} floor {pitch_floor} step {time_step} subtract {subtract_mean}: worst |dB difference| {worst:.3e}")
    assert worst <= R.CONTOUR_TOL_DB
    return worst


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("pitch_floor,time_step,subtract_mean", PARAMS)
def test_ragged_batch_matches_restatement(engine, rate, pitch_floor, time_step, subtract_mean):
    clips, slices = make_batch(rate, pitch_floor)
    engine.upload(clips, rate)
    params = P.IntensityParams.praat(pitch_floor, time_step, subtract_mean)
    plan_off, plan_status = engine.intensity_plan(slices, params)
    res = engine.intensity(slices, params)
    assert np.array_equal(res["frame_offsets"], plan_off) and np.array_equal(res["summary"]["status"], plan_status)
    assert list(plan_status[6:12]) == [0, 1, 0, 0, 0, 2] and plan_off[7] - plan_off[6] == 1
    hs, taps = H.intensity_window(rate, pitch_floor)
    assert len(taps) % 2 == 1 and (pitch_floor != 100.0 or len(taps) == {16000: 1025, 44100: 2823}[rate])
    check_against_restatement(res, clips, slices, rate, pitch_floor, time_step, subtract_mean)
    if subtract_mean:                                                    # silence and a constant: exactly nothing remains
        for i in (2, 3):
            assert np.all(res["values"][plan_off[i]:plan_off[i + 1]] == -300.0) and res["summary"]["n_positive"][i] == 0
    assert np.any((res["values"] < 0) & (res["values"] > -300.0))       # the isolated bits sit below 0 dB
    # summaries alone: same numbers, no contour
    again = engine.intensity(slices, params, want_contour=False)
    assert again["values"] is None and again["summary"].tobytes() == res["summary"].tobytes()


def test_real_recording(engine):
    pcm = np.load(os.path.join(G, "c1_segment_ph9_16k.npz"))["pcm"]
    engine.upload([pcm], 16000)
    sl = engine.whole_clip_slices()
    res = engine.intensity(sl)
    check_against_restatement(res, [pcm], sl, 16000, 100.0, 0.0, True)
    assert res["summary"]["n_frames"][0] in (617, 618) and res["summary"]["n_positive"][0] > 0   # (5 - 0.064) / 0.008 = 617 to rounding


def test_bits_do_not_depend_on_the_batch(engine):
    rate = 16000
    clips = make_clips(rate)
    rng = np.random.default_rng(3)
    others = [(rng.standard_normal(int(rng.integers(1100, 9000))) * 3000).astype(np.int16) for _ in range(32)]
    params = P.IntensityParams.praat()

    def run(batch, which):
        engine.upload(batch, rate)
        res = engine.intensity(engine.whole_clip_slices(), params)
        o = res["frame_offsets"]
        return res["values"][o[which]:o[which + 1]].tobytes(), res["summary"][which].tobytes()

    alone = run([clips[0]], 0)
    assert run([clips[0]] + others, 0) == alone and run(others + [clips[0]], 32) == alone
    engine.upload([clips[0]], rate)
    first = engine.intensity(engine.whole_clip_slices(), params)
    second = engine.intensity(engine.whole_clip_slices(), params)       # the cached plan
    assert first["values"].tobytes() == second["values"].tobytes() == alone[0]


def test_other_results_stay_untouched(engine):
    rate = 16000
    clips = make_clips(rate)[:2]
    engine.upload(clips, rate)
    sl = engine.whole_clip_slices()
    pp = P.PitchParams.praat(75.0, 600.0)
    engine.pitch_run(sl, pp); engine.energy_run(sl)
    pitch_before, energy_before = engine.pitch_fetch(want_strength=True), engine.energy_fetch()
    engine.pitch_run(sl, pp); engine.energy_run(sl)
    engine.intensity_run(sl, P.IntensityParams.praat())
    res = engine.intensity_fetch()
    pitch_after, energy_after = engine.pitch_fetch(want_strength=True), engine.energy_fetch()
    assert energy_after.tobytes() == energy_before.tobytes()
    for k in ("f0", "strength", "summary", "frame_offsets"):
        assert pitch_after[k].tobytes() == pitch_before[k].tobytes(), k
    check_against_restatement(res, clips, sl, rate, 100.0, 0.0, True)


def test_window_beyond_the_kernel_is_refused(engine):
    rate = 16000
    engine.upload([np.ones(2 * rate, dtype=np.int16)], rate)
    sl = engine.whole_clip_slices()
    engine.intensity(sl, P.IntensityParams.praat(16.7))                 # 6 133 taps: inside
    with pytest.raises(P.PceError, match="status -5"):                  # PCE_E_LIMIT
        engine.intensity(sl, P.IntensityParams.praat(10.0))             # 10 241 taps
    with pytest.raises(P.PceError, match="status -4"):                  # no numbers left behind by the refused run
        engine.intensity_fetch()


# ---------------------------------------------------------------- the module end to end
def write_wav(path, pcm, rate):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def test_module_end_to_end(engine, tmp_path, capsys):
    z = np.load(os.path.join(G, "demo_excerpts.npz"))
    seg = lambda k: z[f"segment_ph{k}"]
    # lea: 44.1 kHz pairs; max_EP02: the same kind of material at 22.05 kHz (every other sample); ph6 has no partner, ph5 is unreadable
    for k, partner in ((2, 3), (4, 5), (10, 11)):
        write_wav(tmp_path / "lea" / "audio" / f"segment_ph{k}.wav", seg(k), 44100)
        write_wav(tmp_path / "lea_microsoft" / "audio" / f"segment_ph{k}.wav", seg(partner), 44100)
    write_wav(tmp_path / "lea" / "audio" / "segment_ph6.wav", seg(6), 44100)
    for k, partner in ((7, 8), (9, 2)):
        write_wav(tmp_path / "max_EP02" / "audio" / f"segment_ph{k}.wav", seg(k)[::2], 22050)
        write_wav(tmp_path / "max_EP02_microsoft" / "audio" / f"segment_ph{k}.wav", seg(partner)[::2], 22050)
    write_wav(tmp_path / "max_EP02" / "audio" / "segment_ph5.wav", seg(5)[::2], 22050)
    (tmp_path / "max_EP02_microsoft" / "audio" / "segment_ph5.wav").write_bytes(b"RIFF")
    by_entry = {"lea": [("lea", f"lea_ph{k}", "lea", k) for k in (10, 2, 4)],
                "max_EP02": [("max", f"max_EP02_ph{k}", "max_EP02", k) for k in (7, 9)]}
    order = [x for e in os.listdir(tmp_path) for x in by_entry.get(e, [])]
    per_file = {"pitch": lambda p: M.extract_pitch_mean(p, engine=engine), "volume": lambda p: M.extract_mean_volume(p, engine=engine),
                "rate": lambda p: 1.0 / M.extract_duration(p)}
    for feature in ("pitch", "volume", "rate"):
        nat, syn, spk, ids = M.extract_and_cache_feature(str(tmp_path), feature, engine=engine)
        assert capsys.readouterr().out.count("Erreur avec ") == 1
        assert spk == [o[0] for o in order] and ids == [o[1] for o in order]
        for (_, _, entry, k), n_val, s_val in zip(order, nat, syn):
            assert n_val == per_file[feature](str(tmp_path / entry / "audio" / f"segment_ph{k}.wav"))
            assert s_val == per_file[feature](str(tmp_path / (entry + "_microsoft") / "audio" / f"segment_ph{k}.wav"))
        assert all(math.isfinite(v) and v > 0 for v in nat + syn)
        M.save_feature_only(str(tmp_path / f"{feature}_data.npz"), nat, syn, spk, ids)
        assert M.load_feature_only(str(tmp_path / f"{feature}_data.npz")) == (nat, syn, spk, ids)
    # the volume number is the restatement's, the curve functions return the analysis' own frames
    p = str(tmp_path / "max_EP02" / "audio" / "segment_ph7.wav")
    want = R.intensity(seg(7)[::2], 22050)[0]
    assert abs(M.extract_mean_volume(p, engine=engine) - R.mean_positive(want)) <= 1e-9
    raw = M.raw_feature(p, str(tmp_path / "lea" / "audio" / "segment_ph2.wav"), "volume", engine=engine)
    assert len(raw[0]) == np.sum(want > 0) and np.max(np.abs(raw[0] - want[want > 0])) <= 1e-9
    f0 = M.raw_feature(p, p, "pitch", engine=engine)[0]
    assert len(f0) and M.raw_feature(p, p, "rate", engine=engine)[0][0] == 1.0 / (len(seg(7)[::2]) / 22050)
