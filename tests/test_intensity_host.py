"""CPU tests of the Praat-intensity host rules (tap table, frame rule), of the float64 restatement the GPU tests check the kernel with
(known answers: Praat itself is absent, parity is unpinned), and of the corpus walk of visualisation/Compare_speech_noenhanced.py
against a stub engine."""
import math
import os
import wave

import numpy as np
import pytest

import intensity_restatement as R
from prosody_control_french_tts_amd import hostrules as H
from prosody_control_french_tts_amd.visualisation import Compare_speech_noenhanced as M

RATES = (16000, 44100)


def sine(rate, seconds=0.5, amp=0.25, freq=1000.0):
    t = np.arange(int(round(seconds * rate))) / rate
    return np.round(amp * 32768.0 * np.sin(2 * np.pi * freq * t)).astype(np.int16)


@pytest.mark.parametrize("rate", RATES)
def test_sine_gives_its_analytic_level(rate):
    values, _, status = R.intensity(sine(rate), rate)
    want = 10 * math.log10(0.25 ** 2 / 2 / 4e-10)                  # 78.9276 dB
    assert status == 0 and len(values) > 10
    assert np.max(np.abs(values - want)) < 1e-3


@pytest.mark.parametrize("rate", RATES)
def test_silence_and_constants(rate):
    n = rate // 4
    assert np.all(R.intensity(np.zeros(n, np.int16), rate)[0] == -300.0)
    c = 1234
    const = np.full(n, c, np.int16)
    assert np.all(R.intensity(const, rate)[0] == -300.0)             # exact integer mean: exactly zero remains
    off = R.intensity(const, rate, subtract_mean=False)[0]
    assert np.max(np.abs(off - 10 * math.log10((c / 32768.0) ** 2 / 4e-10))) < 1e-9


def test_window_geometry():
    for rate, hs in ((16000, 512), (44100, 1411)):
        got, taps = H.intensity_window(rate, 100.0)
        assert got == hs and len(taps) == 2 * hs + 1
        assert np.array_equal(taps, taps[::-1]) and np.argmax(taps) == hs and np.all(np.diff(taps[:hs + 1]) > 0)
        assert taps[hs] == H.bessel_i0_f(2 * math.pi ** 2 + 0.5)
    assert H.intensity_window(16000, 100.0)[1][0] == 1.0             # k dx = half exactly: I0f(0)
    assert H.intensity_window(48000, 50.0)[0] == 3072                # the widest window the kernel documents: 6 145 taps


def test_frame_rule():
    nf, t1, dt = H.intensity_frames(8000, 16000, 0.5 / 16000)        # 0.5 s
    assert (nf, dt) == (55, 0.008) and abs(t1 - 0.034) < 1e-15
    values, t1_r, status = R.intensity(np.zeros(8000, np.int16), 16000)
    assert len(values) == 55 and t1_r == t1 and status == 0
    for rate in RATES:
        n_min = math.ceil(0.064 * rate)                              # the first length that holds one window
        assert H.intensity_frames(n_min, rate, 0.5 / rate)[0] == 1
        assert H.intensity_frames(n_min - 1, rate, 0.5 / rate)[0] == 0
        assert R.intensity(np.zeros(n_min - 1, np.int16), rate)[2] == R.TOO_SHORT
        assert R.intensity(np.zeros(n_min, np.int16), rate)[2] == 0
    assert R.intensity(np.zeros(0, np.int16), 16000)[2] == R.EMPTY
    assert H.intensity_frames(16000, 16000, 0.0, 100.0, 0.01)[0] == 94   # floor(0.936 / 0.01) + 1


def test_i0f_polynomials():
    lo, hi = H.bessel_i0_f(np.array([np.nextafter(3.75, 0.0), 3.75]))
    assert abs(hi - lo) / lo < 2e-7                                  # the two polynomials meet to their stated accuracy
    x = np.array([0.0, 0.5, 2.0, 3.7, 3.75, 5.0, 12.0, 20.2])
    assert np.max(np.abs(H.bessel_i0_f(x) / np.i0(x) - 1.0)) < 2e-7
    assert np.array_equal(H.bessel_i0_f(-x), H.bessel_i0_f(x))


# ---------------------------------------------------------------- the module's corpus walk against a stub engine
class StubEngine:
    """Stands in for ProsodyEngine: 'pitch' is 100 Hz + the clip's first sample where that is positive, 'volume' the restatement."""

    def __init__(self):
        self.uploads = []

    def upload(self, clips, rate):
        self.clips, self.rate = [np.asarray(c) for c in clips], rate
        self.uploads.append((rate, len(clips)))

    def whole_clip_slices(self):
        return list(range(len(self.clips)))

    def _pack(self, arrays, status):
        from prosody_control_french_tts_amd.engine import INTENSITY_SUMMARY_DTYPE
        off = np.zeros(len(arrays) + 1, dtype=np.int64); np.cumsum([len(a) for a in arrays], out=off[1:])
        summ = np.zeros(len(arrays), dtype=INTENSITY_SUMMARY_DTYPE)
        summ["status"] = status
        for i, a in enumerate(arrays):
            summ["n_frames"][i] = len(a); summ["n_positive"][i] = int(np.sum(a > 0)); summ["mean_positive"][i] = R.mean_positive(a)
        return np.concatenate(arrays + [np.zeros(0)]), off, summ

    def pitch(self, slices, params):
        assert (params.pitch_floor, params.pitch_ceiling) == (75.0, 600.0)
        arrays = [np.array([0.0, 100.0 + c[0], 0.0]) if len(c) >= 100 and c[0] > 0 else np.zeros(3 if len(c) >= 100 else 0) for c in self.clips]
        f0, off, summ = self._pack(arrays, [0 if len(c) >= 100 else 1 for c in self.clips])
        return {"f0": f0, "frame_offsets": off, "summary": summ}

    def intensity(self, slices, params, want_contour=True):
        res = [R.intensity(c.astype(np.int16), self.rate) for c in self.clips]
        vals, off, summ = self._pack([r[0] for r in res], [r[2] for r in res])
        return {"values": vals if want_contour else None, "frame_offsets": off, "summary": summ}


def write_wav(path, pcm, rate):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


@pytest.fixture()
def tree(tmp_path):
    """alice (16 kHz): ph1, ph2 (synthesis unvoiced -> NaN pair), ph3 (no partner), ph10 (sorts before ph2), ph4 (unreadable natural),
    ph5 (natural shorter than any window); bob_EP03 (44.1 kHz): ph7; carol: no synthesis folder; a stray file and an entry without audio."""
    rng = np.random.default_rng(5)
    def clip(first, n=4000):
        x = (rng.standard_normal(n) * 2000).astype(np.int16); x[0] = first
        return x
    a, am = tmp_path / "alice" / "audio", tmp_path / "alice_microsoft" / "audio"
    write_wav(a / "segment_ph1.wav", clip(11), 16000); write_wav(am / "segment_ph1.wav", clip(21), 16000)
    write_wav(a / "segment_ph2.wav", clip(12), 16000); write_wav(am / "segment_ph2.wav", clip(-5), 16000)
    write_wav(a / "segment_ph3.wav", clip(13), 16000)
    write_wav(a / "segment_ph10.wav", clip(14), 16000); write_wav(am / "segment_ph10.wav", clip(24), 16000)
    (a / "segment_ph4.wav").write_bytes(b"not a wav file"); write_wav(am / "segment_ph4.wav", clip(25), 16000)
    write_wav(a / "segment_ph5.wav", clip(15, n=50), 16000); write_wav(am / "segment_ph5.wav", clip(26), 16000)
    write_wav(a / "other.wav", clip(1), 16000); write_wav(am / "other.wav", clip(1), 16000)
    b, bm = tmp_path / "bob_EP03" / "audio", tmp_path / "bob_EP03_microsoft" / "audio"
    write_wav(b / "segment_ph7.wav", clip(17, n=9000), 44100); write_wav(bm / "segment_ph7.wav", clip(27, n=9000), 44100)
    write_wav(tmp_path / "carol" / "audio" / "segment_ph1.wav", clip(1), 16000)
    os.makedirs(tmp_path / "dave")
    (tmp_path / "pitch_data.npz").write_bytes(b"")
    return tmp_path


def in_listdir_order(root, by_entry):
    return [x for e in os.listdir(root) for x in by_entry.get(e, [])]


def test_walk_ids_order_nan_and_errors(tree, capsys):
    eng = StubEngine()
    nat, syn, spk, ids = M.extract_and_cache_feature(str(tree), "pitch", engine=eng)
    out = capsys.readouterr().out
    assert ids == in_listdir_order(tree, {"alice": ["alice_ph1", "alice_ph10"], "bob_EP03": ["bob_EP03_ph7"]})
    assert spk == in_listdir_order(tree, {"alice": ["alice", "alice"], "bob_EP03": ["bob"]})
    want = {"alice_ph1": (111.0, 121.0), "alice_ph10": (114.0, 124.0), "bob_EP03_ph7": (117.0, 127.0)}
    assert [(n, s) for n, s in zip(nat, syn)] == [want[i] for i in ids]
    lines = [ln for ln in out.splitlines() if ln.startswith("Erreur avec ")]
    assert len(lines) == 2 and "segment_ph4.wav" in lines[0] and "segment_ph5.wav" in lines[1]
    assert str(tree / "alice_microsoft" / "audio" / "segment_ph4.wav") in lines[0]
    assert sorted(eng.uploads) == [(16000, 9), (44100, 2)]           # one upload per sample rate, not one per file

    eng = StubEngine()
    small = M.extract_and_cache_feature(str(tree), "pitch", engine=eng, max_batch_bytes=16000)
    assert small == (nat, syn, spk, ids) and len(eng.uploads) > 3    # bounded batches, same lists
    capsys.readouterr()


def test_volume_rate_and_unknown_feature(tree, capsys):
    eng = StubEngine()
    nat, syn, spk, ids = M.extract_and_cache_feature(str(tree), "volume", engine=eng)
    assert ids == in_listdir_order(tree, {"alice": ["alice_ph1", "alice_ph10", "alice_ph2"], "bob_EP03": ["bob_EP03_ph7"]})
    p = tree / "alice" / "audio" / "segment_ph10.wav"
    rate, pcm = H.decode_wav(p)
    assert nat[ids.index("alice_ph10")] == R.mean_positive(R.intensity(pcm, rate)[0]) == M.extract_mean_volume(str(p), engine=eng)
    assert capsys.readouterr().out.count("Erreur avec ") == 2        # unreadable, and shorter than the window

    eng = StubEngine()
    nat, syn, spk, ids = M.extract_and_cache_feature(str(tree), "rate", engine=eng)
    assert eng.uploads == []                                         # 'rate' never touches the device
    assert ids == in_listdir_order(tree, {"alice": ["alice_ph1", "alice_ph10", "alice_ph2", "alice_ph5"], "bob_EP03": ["bob_EP03_ph7"]})
    assert nat[ids.index("alice_ph5")] == 1.0 / (50 / 16000) and syn[ids.index("bob_EP03_ph7")] == 1.0 / (9000 / 44100)
    assert M.extract_duration(str(p)) == 0.25
    assert capsys.readouterr().out.count("Erreur avec ") == 1
    assert M.extract_and_cache_feature(str(tree), "jitter", engine=eng) == ([], [], [], [])


def test_per_file_functions_and_curves(tree, capsys):
    eng = StubEngine()
    a = tree / "alice" / "audio"
    assert M.extract_pitch_mean(str(a / "segment_ph1.wav"), engine=eng) == 111.0
    assert math.isnan(M.extract_pitch_mean(str(tree / "alice_microsoft" / "audio" / "segment_ph2.wav"), engine=eng))
    with pytest.raises(H.PraatError):
        M.extract_mean_volume(str(a / "segment_ph5.wav"), engine=eng)
    with pytest.raises(H.CouldntDecodeError):
        M.extract_pitch_mean(str(a / "segment_ph4.wav"), engine=eng)
    nat, syn, labels = M.compare_pitch(str(a), str(tree / "alice_microsoft" / "audio"), engine=eng)
    assert labels == ["other.wav", "segment_ph1.wav", "segment_ph10.wav"] and nat == [101.0, 111.0, 114.0] and syn == [101.0, 121.0, 124.0]
    assert capsys.readouterr().out.count("Erreur avec segment_ph") == 2

    n1, s1 = str(a / "segment_ph1.wav"), str(tree / "bob_EP03_microsoft" / "audio" / "segment_ph7.wav")
    raw = M.raw_feature(n1, s1, "volume", engine=eng)
    for path, got in zip((n1, s1), raw):
        rate, pcm = H.decode_wav(path)
        v = R.intensity(pcm, rate)[0]
        assert np.array_equal(got, v[v > 0]) and len(got) > 1
    z = M.zscore_feature(n1, s1, "volume", engine=eng)
    assert all(abs(np.mean(x)) < 1e-12 and abs(np.std(x) - 1) < 1e-12 for x in z)
    assert [x.tolist() for x in M.raw_feature(n1, s1, "pitch", engine=eng)] == [[111.0], [127.0]]
    r = M.raw_feature(n1, s1, "rate", engine=eng)
    assert r[0].tolist() == [4.0] * 3 and r[1].tolist() == [1.0 / (9000 / 44100)] * 3
    assert M.raw_feature(n1, s1, "jitter", engine=eng) is None and M.zscore_feature(n1, s1, "jitter", engine=eng) is None


def test_cache_round_trip_and_quartiles(tmp_path, capsys):
    data = ([101.5, 99.25], [88.0, 91.0], ["alice", "bob"], ["alice_ph1", "bob_EP03_ph7"])
    M.save_feature_only(str(tmp_path / "pitch_data.npz"), *data)
    assert M.load_feature_only(str(tmp_path / "pitch_data.npz")) == data
    M.print_quartiles([100.0, 200.0, 300.0, 400.0], [10.0, 20.0])
    assert capsys.readouterr().out.splitlines() == ["Voix naturelle :", "  Q1 (25%)   : 175.00 Hz", "  Médiane    : 250.00 Hz", "  Q3 (75%)   : 325.00 Hz",
                                                    "Voix synthèse :", "  Q1 (25%)   : 12.50 Hz", "  Médiane    : 15.00 Hz", "  Q3 (75%)   : 17.50 Hz"]
