"""pce_w2v_* on the device: the three new stages against their float64 restatements (tests/w2v_restatement.py), the whole forward pass against
the installed ``transformers`` ``Wav2Vec2ForCTC`` on random weights (tests/w2v_models.py: no trained checkpoint ships), bit-for-bit independence
of chunk size and batch composition, the chain into ``ctc_align`` / ``CTCFA.process_files``, and the errors.

Shapes.  Positional convolution: T = 1, 63, 64, 65, 129, 300 (one frame; around the 64-frame share of a wave; more than one 256-frame workgroup
at 300) x 16, 48, 64 columns per group, two windows with different values (a halo that read the neighbour would show).  Waveform layer: windows
of 700 frames (ends inside every tile) and 1025 (one past the 1024-frame statistics partial and the fourth 256-frame tile), a clip of 2.3
windows (the last window's last two thirds are zeros), samples at both int16 extremes, 640 channels for the group form (its channel loop runs
twice) and 320 for the layer form (twice, the second time with 64 of 256 threads); a window shorter than the ten taps gives no frames.
End to end: (2 s, 0.5 s) windows of 149 frames -> 100 kept; for B also one 31 s clip at (30 s, 2 s): two windows of 1 699 keys."""
import copy
import functools
import os
import sys
import wave

import numpy as np
import pytest
import torch  # noqa: F401  (before the session's engine loads libpce.so: torch brings its own copy of the HIP runtime, and the one loaded first serves both)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_models as M
import w2v_restatement as R
from prosody_control_french_tts_amd import w2v_weights as WW
from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE
from prosody_control_french_tts_amd.engine import PceError, DeviceEmissions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "r19", "w2v_parity.txt")
SHORT = (2, 0.5)                      # window, context in seconds


def _speechlike(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 7000 * np.sin(2 * np.pi * 140.0 * t * (1 + 0.1 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 2500 * np.sin(2 * np.pi * 910.0 * t) + 1200 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


CLIPS = {"short": [_speechlike(4800, 1), _speechlike(32000, 2), _speechlike(75200, 3)], "long": [_speechlike(31 * 16000, 4)]}
PLAN = {"short": SHORT, "long": (30, 2)}


def rel_l2(a, b):
    a, b = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in a]), np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in b])
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _rows(em, n_frames):
    return [em[i, :n_frames[i]].numpy() for i in range(len(n_frames))]


@functools.lru_cache(maxsize=None)
def reference(form, which):
    """hf_emissions on the CPU in fp32: one list of [n_frames][V + 1] arrays per (model, clip set), computed once and shared."""
    em, n_frames = CE.hf_emissions(M.model(form), CLIPS[which], "cpu", *PLAN[which])
    return _rows(em, n_frames)


@functools.lru_cache(maxsize=None)
def d_half(form, which, bf16):
    """transformers' own forward with the model in the 16-bit type, on the CPU, against its fp32 forward: relative L2 distance of the emissions."""
    half = copy.deepcopy(M.model(form)).to(torch.bfloat16 if bf16 else torch.float16)
    em, n_frames = CE.hf_emissions(half, CLIPS[which], "cpu", *PLAN[which])
    return rel_l2(_rows(em, n_frames), reference(form, which))


def emissions(engine, form, which, windows_per_chunk=None, clips=None):
    engine.w2v_load(M.model(form))
    engine.upload(CLIPS[which] if clips is None else clips, 16000)
    return engine.w2v_emissions(*PLAN[which], windows_per_chunk=windows_per_chunk)


# ------------------------------------------------------------------------------------------------------------ 1. the stages against float64
def _ratio(got, want, bound, bf16=False):
    allowed = R.stored_step(bf16) * np.abs(want) + bound
    return float((np.abs(got - want) / allowed).max()) if want.size else 0.0


OPERANDS = ["fp16", "bf16"]                # the two compiled builds of the new kernels


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("cg", [16, 48, 64])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 300])
def test_positional_convolution_against_float64(engine, T, cg, operands):
    """Per element: the fp32 accumulation of K = 128 cg products, K 2^-23 sum(|a| |w|), and the rounding of acc + bias, carried through GELU
    (slope <= 1.13, the device's erf approximation 2e-7 (1 + |x|)), plus the rounding of the fp32 sum x + GELU (the output is fp32: no 16-bit step)."""
    engine.whisper_set_operands(operands)
    bf16 = operands == "bf16"
    rng = np.random.default_rng(1000 * cg + T)
    groups, n_win = 2, 2
    d = groups * cg
    x = R.r16(rng.standard_normal((n_win, T, d)), bf16)
    w = R.r16(rng.standard_normal((d, 128, cg)) * (2.0 / np.sqrt(128 * cg)), bf16)
    bias = rng.standard_normal(d).astype(np.float32) * 0.3
    got = engine.selftest_w2v_posconv(x.astype(np.float32), R.to_bits(w, bf16), bias, groups).astype(np.float64)
    want, bound = R.pos_conv(x, w, bias, groups)
    worst = float((np.abs(got - want) / bound).max())
    print(f"w2v posconv T {T} cg {cg} {operands}: worst error / bound = {worst:.3f}")
    assert got.shape == (n_win, T, d) and np.abs(want - x).max() > 0.05
    assert worst <= 1.0


WAVE_CASES = {   # (window, context, clip samples): frames per window = (window + 2 context - 10) / 5 + 1
    "inside-a-tile": (2705, 400, 6222),               # 700 frames; 2.3 windows: the third window holds 0.3 windows of audio, then zeros
    "one-past-a-tile": (4330, 400, 9959),             # 1025 frames
}


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("case", sorted(WAVE_CASES))
@pytest.mark.parametrize("feat_norm", [0, 1])
def test_waveform_layer_against_float64(engine, feat_norm, case, operands):
    """Per stored element 2^-11 |y| (2^-8 under bf16 operands) plus the restatement's bound: the ten products' fp32 accumulation through the normalisation (group form: the
    statistics count every frame of the window, the zeros of the padding included) and GELU."""
    engine.whisper_set_operands(operands)
    bf16 = operands == "bf16"
    window, context, n = WAVE_CASES[case]
    rng = np.random.default_rng(n + feat_norm)
    ch = 640 if feat_norm == 0 else 320
    pcm = _speechlike(n, n)
    pcm[:4] = [-32768, 32767, -32768, 32767]
    pcm[-3:] = [32767, -32768, 32767]
    w = (rng.standard_normal((ch, 10)) * 0.4).astype(np.float32)
    gamma = (1.0 + 0.2 * rng.standard_normal(ch)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(ch)).astype(np.float32)
    bias = None if feat_norm == 0 else (0.1 * rng.standard_normal(ch)).astype(np.float32)
    got = R.from_bits(engine.selftest_w2v_wave(pcm, window, context, feat_norm, w, gamma, beta, bias), bf16)
    want, bound = R.wave_layer(pcm, window, context, feat_norm, w, bias, gamma, beta)
    t0 = (window + 2 * context - 10) // 5 + 1
    assert got.shape == want.shape == (3, t0, ch) and t0 == {"inside-a-tile": 700, "one-past-a-tile": 1025}[case]
    tail = R.windows(pcm, window, context)[2]
    assert np.all(tail[len(tail) // 2:] == 0) and np.any(tail[:len(tail) // 3] != 0)
    worst = _ratio(got, want, bound, bf16)
    print(f"w2v waveform layer {'group' if feat_norm == 0 else 'layer'} {case} {operands}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_waveform_layer_shorter_than_its_taps(engine):
    w = np.ones((64, 10), np.float32)
    for feat_norm in (0, 1):
        out = engine.selftest_w2v_wave(np.full(20, 1000, np.int16), 8, 0, feat_norm, w, np.ones(64, np.float32), np.zeros(64, np.float32))
        assert out.shape == (3, 0, 64)
    one = engine.selftest_w2v_wave(np.full(20, 1000, np.int16), 10, 0, 1, w, np.ones(64, np.float32), np.zeros(64, np.float32))
    assert one.shape == (2, 1, 64)                                   # exactly one tap window: one frame per window


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("ch", [128, 512])
def test_layernorm_gelu_against_float64(engine, ch, operands):
    engine.whisper_set_operands(operands)
    bf16 = operands == "bf16"
    rng = np.random.default_rng(ch)
    x = R.r16(rng.standard_normal((9, ch)) * 3.0 + 0.5, bf16)
    w = (1.0 + 0.2 * rng.standard_normal(ch)).astype(np.float32)
    b = (0.2 * rng.standard_normal(ch)).astype(np.float32)
    for with_gelu in (True, False):
        got = R.from_bits(engine.selftest_w2v_lngelu(R.to_bits(x, bf16), w, b, 1e-5, with_gelu), bf16)
        want, bound = R.ln_gelu(x, w, b, 1e-5, with_gelu)
        worst = _ratio(got, want, bound, bf16)
        print(f"w2v layernorm{' + gelu' if with_gelu else ''} C {ch} {operands}: worst error / bound = {worst:.3f}")
        assert got.shape == (9, ch) and worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ 2. end to end against transformers
def _record(key, line):
    try:
        have = open(PARITY_FILE, encoding="utf-8").read() if os.path.exists(PARITY_FILE) else ""
        if f"{key}:" not in have:
            os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
            with open(PARITY_FILE, "a", encoding="utf-8") as fh:
                if not have:
                    fh.write("# tests/test_gpu_w2v.py::test_emissions_against_transformers, random weights (tests/w2v_models.py): relative L2 distances of the\n"
                             "# emissions to transformers' fp32 forward on the CPU; d_half = transformers' own forward in the 16-bit type, on the CPU\n")
                fh.write(line + "\n")
    except OSError:
        pass                                                        # (a read-only checkout: the figures are printed)


@pytest.mark.parametrize("form,which,operands", [("A", "short", "fp16"), ("B", "short", "fp16"), ("B", "long", "fp16"), ("B", "short", "bf16")])
def test_emissions_against_transformers(engine, form, which, operands):
    """The reference is hf_emissions(model, pcm, "cpu") in fp32; frame counts and shapes must be equal.  The bound is measured, not chosen:
    d_half = the distance of transformers' own forward in the context's 16-bit type from its fp32 forward, on the same input; the device may be
    4 x as far (other rounding points and summation orders).  Both distances go to profiles/r19/w2v_parity.txt on the first GPU run."""
    engine.whisper_set_operands(operands)
    ref = reference(form, which)
    de = emissions(engine, form, which, windows_per_chunk=1 if which == "long" else None)
    got = de.numpy()
    assert isinstance(de, DeviceEmissions) and de.n_cols == ref[0].shape[1] == M.FORMS[form]["vocab_size"] + 1
    assert [g.shape for g in got] == [r.shape for r in ref] and de.n_frames.tolist() == [len(r) for r in ref]
    assert de.n_frames.tolist() == ([15, 100, 235] if which == "short" else [1550])
    assert de.row_start.tolist() == np.concatenate([[0], np.cumsum(de.n_frames)[:-1]]).tolist()
    assert all(np.all(g[:, -1] == 0) and np.all(np.isfinite(g)) for g in got)
    dh, dd = d_half(form, which, operands == "bf16"), rel_l2(got, ref)
    key = f"{form} {which} {operands}"
    line = f"{key}: frames {sum(len(r) for r in ref)}  d_half {dh:.6e}  d_device {dd:.6e}  bound 4 d_half {4 * dh:.6e}"
    print("w2v emissions", line)
    _record(key, line)
    assert 0 < dh < 0.02
    assert dd <= 4 * dh


# ------------------------------------------------------------------------------------------------------------ 3. independence, bit for bit
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("form", ["A", "B"])
def test_chunk_size_and_batch_do_not_change_a_bit(engine, form):
    whole = emissions(engine, form, "short").numpy()                  # 1 + 1 + 3 windows in one chunk
    single = emissions(engine, form, "short", windows_per_chunk=1).numpy()
    pairs = emissions(engine, form, "short", windows_per_chunk=2).numpy()      # a chunk boundary inside the third clip
    assert all(_same_bits(a, b) and _same_bits(a, c) for a, b, c in zip(whole, single, pairs))
    alone = emissions(engine, form, "short", clips=[CLIPS["short"][2]]).numpy()
    five = emissions(engine, form, "short", clips=[CLIPS["short"][i] for i in (1, 0, 2, 1, 0)]).numpy()
    assert _same_bits(alone[0], whole[2]) and _same_bits(five[2], whole[2]) and _same_bits(five[0], whole[1]) and _same_bits(five[4], whole[0])


# ------------------------------------------------------------------------------------------------------------ 4. the chain
def _targets(rng, n_frames, vocab):
    return [rng.integers(1, vocab, size=max(1, int(t) // 5)).astype(np.int32) for t in n_frames]


def test_ctc_align_reads_device_emissions_in_place(engine):
    de = emissions(engine, "A", "short")
    fetched = de.numpy()
    tg = _targets(np.random.default_rng(5), de.n_frames, 32)
    on_device, on_host = engine.ctc_align(de, tg), engine.ctc_align(fetched, tg)
    assert len(on_device) == len(on_host) == 3
    for a, b in zip(on_device, on_host):
        assert a["status"] == b["status"] == 0 and sorted(a) == sorted(b)
        for k in ("path", "frame_score", "tok_first", "tok_last"):
            assert np.array_equal(a[k], b[k]), k
        assert np.float32(a["score"]).view(np.uint32) == np.float32(b["score"]).view(np.uint32)
    again = de.numpy()
    assert all(_same_bits(x, y) for x, y in zip(fetched, again))     # read in place, not written
    with pytest.raises(ValueError):
        engine.ctc_align(de, tg, n_frames=de.n_frames)
    # a later run (or load) may free or overwrite what `de` points to: it is refused, not read
    newer = emissions(engine, "A", "short", windows_per_chunk=2)
    with pytest.raises(ValueError, match="stale"):
        engine.ctc_align(de, tg)
    with pytest.raises(ValueError, match="stale"):
        de.numpy()
    assert [a["status"] for a in engine.ctc_align(newer, tg)] == [0, 0, 0]


def test_engine_emissions_loads_when_the_engine_holds_another_model(engine):
    """engine_emissions asks the engine which model it holds: a direct w2v_load of another model in between is seen, and so is another operand build."""
    a, b = M.model("A"), M.model("B")
    clips = CLIPS["short"][:2]
    first = CE.engine_emissions(engine, a, clips, *SHORT).numpy()
    assert engine.w2v_holds(a) and not engine.w2v_holds(b)
    engine.w2v_load(b)
    assert engine.w2v_holds(b) and not engine.w2v_holds(a)
    again = CE.engine_emissions(engine, a, clips, *SHORT)
    assert again.n_cols == 33 and all(_same_bits(x, y) for x, y in zip(first, again.numpy()))
    engine.w2v_load(WW.dims(a.config), WW.pack(a.state_dict(), WW.dims(a.config)))          # a blob names no model object
    assert not engine.w2v_holds(a)
    engine.whisper_set_operands("bf16")
    assert not engine.w2v_holds(a)
    assert CE.engine_emissions(engine, a, clips, *SHORT).n_frames.tolist() == [15, 100] and engine.w2v_holds(a)
    engine.whisper_set_operands("fp16")
    assert not engine.w2v_holds(a)                                 # (the marker names the build of the latest load)


def test_process_files_on_the_engine(engine, tmp_path):
    from prosody_control_french_tts_amd import synth
    from prosody_control_french_tts_amd.Aligners import CTCFA, ctc_segments
    model = M.model("A")
    vocab = {ch: i + 1 for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz'")}
    texts = {"c0": "Bonjour, le monde!", "c1": "la (petite) maison: bleue", "c2": "il arrive — demain"}
    audio, trans = tmp_path / "audio", tmp_path / "txt"
    audio.mkdir(); trans.mkdir()
    names, clips = sorted(texts), []
    for k, name in enumerate(names):
        clips.append(synth.synth_clip(k, seconds=2.0 + 0.5 * k))
        with wave.open(str(audio / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(clips[-1].tobytes())
        (trans / f"{name}.txt").write_text(texts[name], encoding="utf-8")

    def files(directory, suffix):
        return {n: open(os.path.join(directory, n), encoding="utf-8").read() for n in sorted(os.listdir(directory)) if n.endswith(suffix)}
    rows = CTCFA.process_files(str(audio), str(trans), str(tmp_path / "tg"), "fra", "segment", False, engine=engine, model=model, vocab=vocab, acoustic="engine")
    words_engine, grids_engine = files(str(audio), ".txt"), files(str(tmp_path / "tg"), ".TextGrid")
    de = CE.engine_emissions(engine, model, clips)
    fetched = de.numpy()
    assert de.n_frames.tolist() == [100, 125, 150] and de.n_cols == 33
    padded = torch.zeros((3, 150, 33), dtype=torch.float32)
    for i, e in enumerate(fetched):
        padded[i, :len(e)] = torch.from_numpy(e)
    rows2 = CTCFA.process_files(str(audio), str(trans), str(tmp_path / "tg2"), "fra", "segment", False, engine=engine, vocab=vocab,
                                emissions=(padded, de.n_frames))
    words_host, grids_host = files(str(audio), ".txt"), files(str(tmp_path / "tg2"), ".TextGrid")
    assert sorted(grids_engine) == [f"{n}.TextGrid" for n in names] and sorted(words_engine) == [f"{n}.txt" for n in names]
    assert grids_engine == grids_host and words_engine == words_host and repr(rows) == repr(rows2)      # (repr: a word without characters has a NaN confidence)
    assert all([r["text"] for r in rows[f"{n}.wav"]] == ctc_segments.preprocess_text(texts[n].lower()).split() for n in names)
    with pytest.raises(ValueError):
        CTCFA.process_files(str(audio), str(trans), str(tmp_path / "tg3"), "fra", "segment", False, engine=engine, model=model, vocab=vocab, acoustic="hip")


# ------------------------------------------------------------------------------------------------------------ 5. errors
def test_errors(engine):
    import prosody_control_french_tts_amd as P
    with P.ProsodyEngine(0) as fresh:
        fresh.upload([CLIPS["short"][0]], 16000)
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_emissions(*SHORT)                               # run before load
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_fetch(0)                                        # fetch before run
        dims = WW.dims(M.config("A"))
        blob = WW.pack(M.model("A").state_dict(), dims)
        with pytest.raises(PceError, match="status -1"):
            fresh.w2v_load(dims, blob[:-1])                           # a blob of the wrong size
        with pytest.raises(PceError, match="status -5"):
            fresh.w2v_load(dict(dims, pos_taps=64), blob)
        with pytest.raises(PceError, match="status -5"):
            fresh.w2v_load(dict(dims, n_head=3), blob)
        fresh.w2v_load(dims, blob)
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_fetch(0)                                        # loaded, still no run
        fresh.upload([_speechlike(4410, 9)], 44100)
        with pytest.raises(PceError, match="status -1.*16000 Hz"):
            fresh.w2v_emissions(*SHORT)
        fresh.upload([CLIPS["short"][0]], 16000)
        with pytest.raises(PceError, match="status -1.*frames per window"):
            fresh.w2v_emissions(2, 0.51)                              # 150 frames, 101 kept behind a cut of 25: not the window's 100
        assert fresh.w2v_emissions(*SHORT).n_frames.tolist() == [15]
