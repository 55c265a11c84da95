"""pce_w2v_run_segments on the device: whisperX's emissions, the wav2vec2 forward pass over segments of unequal length, each alone and unpadded.

1. The two stages that take per-item frame counts, bit for bit against the uniform stages run on each item alone (whose float64 bounds
   tests/test_gpu_w2v.py holds): waveform items of 123 and 400 samples (79 frames, the shorter one zero-padded), 5 125 and 5 130 samples (1 024 and
   1 025 frames: on and one past the statistics partial) and 3 200 frames with both int16 extremes, at different offsets of one clip; positional
   convolution windows of 1, 63, 64, 65, 129 and 300 frames in slots of 300 rows whose rows behind the frames hold other values.
2. The whole forward pass against pce_w2v_run on clips of exactly 12 000 and 34 000 samples, bit for bit.
3. Parity with transformers on random weights (tests/w2v_models.py): segment_emissions on the CPU in fp32 is the reference, the same call in
   the 16-bit type gives d_half, and the device may be 4 x as far, pooled over all segments and over those of at most 2 frames.
4. Independence of batch, order, chunk size and history, bit for bit.
5. The chain into wx_align / whisperX.align / process_files.   6. The errors.

Frames of the standard stack: 400 and 719 samples -> 1, 720 -> 2, 5 200 -> 16, 5 520 -> 17, 20 240 / 20 560 / 20 880 -> 63 / 64 / 65 (around the
64-frame share of a wave and the 16-row padding), 82 320 -> 257 (one past a 256-frame workgroup), 479 999 -> 1 499."""
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
from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE
from prosody_control_french_tts_amd.engine import DeviceEmissions, PceError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "r21", "w2v_segments_parity.txt")
OPERANDS = ["fp16", "bf16"]                # the two compiled builds of the new kernels


def _speechlike(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 7000 * np.sin(2 * np.pi * 140.0 * t * (1 + 0.1 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 2500 * np.sin(2 * np.pi * 910.0 * t) + 1200 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 1. the stages, bit for bit
WAVE_ITEMS = [(7, 130), (1000, 1400), (2000, 7125), (9001, 14131), (15000, 31005)]      # samples [begin, end) of one clip
WAVE_FRAMES = [79, 79, 1024, 1025, 3200]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("feat_norm", [0, 1])
def test_ragged_waveform_layer_equals_each_item_alone(engine, feat_norm, operands):
    engine.whisper_set_operands(operands)
    rng = np.random.default_rng(77 + feat_norm)
    ch = 640 if feat_norm == 0 else 320
    pcm = _speechlike(31005, 31)
    pcm[15000:15004] = [-32768, 32767, -32768, 32767]
    pcm[31002:31005] = [32767, -32768, 32767]
    w = (rng.standard_normal((ch, 10)) * 0.4).astype(np.float32)
    gamma = (1.0 + 0.2 * rng.standard_normal(ch)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(ch)).astype(np.float32)
    bias = None if feat_norm == 0 else (0.1 * rng.standard_normal(ch)).astype(np.float32)
    got, frames = engine.selftest_w2v_wave_segments(pcm, WAVE_ITEMS, feat_norm, w, gamma, beta, bias)
    assert frames == WAVE_FRAMES and got.shape == (5, 3200, ch)
    for i, (b, e) in enumerate(WAVE_ITEMS):
        alone = engine.selftest_w2v_wave(pcm[b:e], max(e - b, 400), 0, feat_norm, w, gamma, beta, bias)       # one window, no context; zeros behind the clip
        assert alone.shape == (1, frames[i], ch) and np.any(alone != 0)
        assert np.array_equal(got[i, :frames[i]], alone[0]), (i, b, e)
        assert not got[i, frames[i]:].any()                          # nothing is written behind an item's own frames
    assert not np.array_equal(got[0, :79], got[1, :79])


POS_LENS = [1, 63, 64, 65, 129, 300]


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("cg", [16, 48, 64])
def test_ragged_positional_convolution_equals_each_window_alone(engine, cg, operands):
    engine.whisper_set_operands(operands)
    bf16 = operands == "bf16"
    rng = np.random.default_rng(500 + cg)
    groups, T = 2, 300
    d = groups * cg
    x = R.r16(rng.standard_normal((len(POS_LENS), T, d)), bf16).astype(np.float32)         # rows behind a window's frames hold values too
    w = R.to_bits(R.r16(rng.standard_normal((d, 128, cg)) * (2.0 / np.sqrt(128 * cg)), bf16), bf16)
    bias = rng.standard_normal(d).astype(np.float32) * 0.3
    got = engine.selftest_w2v_posconv_segments(x, POS_LENS, w, bias, groups)
    assert got.shape == x.shape
    for i, n in enumerate(POS_LENS):
        alone = engine.selftest_w2v_posconv(x[i:i + 1, :n], w, bias, groups)
        assert alone.shape == (1, n, d) and np.abs(alone[0] - x[i, :n]).max() > 0.05
        assert _same_bits(got[i, :n], alone[0]), (i, n)
        assert _same_bits(got[i, n:], x[i, n:])                      # a row behind the frames: the input, as every pad row
    uniform = engine.selftest_w2v_posconv(x, w, bias, groups)
    assert _same_bits(got[-1], uniform[-1]) and not _same_bits(got[0, :1], uniform[0, :1])      # (a halo over the rows behind would give this)


# ------------------------------------------------------------------------------------------------------------ 2. against the uniform run
@pytest.mark.parametrize("form,operands", [("A", "fp16"), ("B", "fp16"), ("B", "bf16")])
def test_whole_clip_segments_equal_the_uniform_run(engine, form, operands):
    """At 12 000 and 34 000 samples the model's frame count is int(seconds * 50) (37, 106), so pce_w2v_run takes the clip as one window with
    no context: the same model on the same samples.  The 20 000-sample segment shares the longer clip's chunk (63 of 112 slot rows)."""
    engine.whisper_set_operands(operands)
    model = M.model(form)
    lengths = model._get_feat_extract_output_lengths
    assert [int(lengths(torch.tensor(n))) for n in (12000, 34000, 20000)] == [37, 106, 62]
    clips = [_speechlike(12000, 11), _speechlike(34000, 12)]
    engine.w2v_load(model)
    uniform = []
    for clip, seconds in zip(clips, (0.75, 2.125)):
        engine.upload([clip], 16000)
        uniform.append(engine.w2v_emissions(seconds, 0, star=False).numpy()[0])
    engine.upload(clips, 16000)
    de = engine.w2v_segment_emissions([(0, 0, 12000), (1, 0, 34000), (1, 3000, 23000)])
    got = de.numpy()
    assert de.n_frames.tolist() == [37, 106, 62] and de.row_start.tolist() == [0, 37, 143] and de.n_cols == M.FORMS[form]["vocab_size"]
    assert _same_bits(got[0], uniform[0]) and _same_bits(got[1], uniform[1])
    assert np.all(np.isfinite(got[2])) and not _same_bits(got[2][:37], got[0])


# ------------------------------------------------------------------------------------------------------------ 3. parity with transformers
CLIP_SAMPLES = (90000, 40000, 480000)
SEGMENTS = [   # (clip, begin, end)
    (0, 1000, 1000), (0, 2000, 2123),                                      # empty and 123 samples: padded to 400
    (0, 300, 700), (0, 5000, 5719), (1, 100, 820),                        # 400, 719, 720 samples: 1, 1, 2 frames
    (1, 1000, 6200), (1, 3000, 8520),                                      # 16, 17 frames
    (0, 10000, 30240), (1, 5000, 25560), (0, 40000, 60880),               # 63, 64, 65
    (0, 0, 82320),                                                         # 257
    (1, 15000, 27000), (1, 21000, 36000),                                  # overlapping, mid-clip
    (1, 30000, 40000),                                                     # ends at the clip's last sample
]
FRAMES = [1, 1, 1, 1, 2, 16, 17, 63, 64, 65, 257, 37, 46, 31]
LONG = (2, 1, 480000)                                                      # 479 999 samples: 1 499 frames


@functools.lru_cache(maxsize=None)
def clips():
    return [_speechlike(n, 40 + i) for i, n in enumerate(CLIP_SAMPLES)]


def segments_of(form):
    return SEGMENTS + [LONG] if form == "A" else list(SEGMENTS)


def _torch_rows(model, segs):
    """segment_emissions on the CPU, per clip, back in the order of segs: one [frames][V] array per segment."""
    out = [None] * len(segs)
    for q in sorted({s[0] for s in segs}):
        mine = [k for k, s in enumerate(segs) if s[0] == q]
        # (+ 0.5: int(t * 16000) of such a time is the sample, whichever way the product rounds)
        em, n_frames = CE.segment_emissions(model, clips()[q], [{"start": (segs[k][1] + 0.5) / 16000, "end": (segs[k][2] + 0.5) / 16000} for k in mine], "cpu")
        for r, k in enumerate(mine):
            out[k] = em[r, :n_frames[r]].numpy()
    return out


@functools.lru_cache(maxsize=None)
def reference(form):
    return _torch_rows(M.model(form), segments_of(form))


@functools.lru_cache(maxsize=None)
def half_rows(form, bf16):
    return _torch_rows(copy.deepcopy(M.model(form)).to(torch.bfloat16 if bf16 else torch.float16), segments_of(form))


def rel_l2(a, b):
    a, b = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in a]), np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in b])
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run(engine, form, segs, **kw):
    if not engine.w2v_holds(M.model(form)):
        engine.w2v_load(M.model(form))
    engine.upload(clips(), 16000)
    return engine.w2v_segment_emissions(segs, **kw)


def _record(key, line):
    try:
        have = open(PARITY_FILE, encoding="utf-8").read() if os.path.exists(PARITY_FILE) else ""
        if f"{key}:" not in have:
            os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
            with open(PARITY_FILE, "a", encoding="utf-8") as fh:
                if not have:
                    fh.write("# tests/test_gpu_w2v_segments.py::test_segment_emissions_against_transformers, random weights (tests/w2v_models.py): relative L2\n"
                             "# distances of the emissions to segment_emissions in fp32 on the CPU; d_half = the same call with the model in the 16-bit type, on the\n"
                             "# CPU; all = pooled over every segment, short = over the segments of at most 2 frames\n")
                fh.write(line + "\n")
    except OSError:
        pass                                                        # (a read-only checkout: the figures are printed)


@pytest.mark.parametrize("form,operands", [("A", "fp16"), ("B", "fp16"), ("B", "bf16")])
def test_segment_emissions_against_transformers(engine, form, operands):
    """The project's rule: d_half is measured, not chosen, and the device may be 4 x as far (other rounding points and summation orders).  Both
    pools' distances go to profiles/r21/w2v_segments_parity.txt on the first GPU run."""
    engine.whisper_set_operands(operands)
    segs, ref, half = segments_of(form), reference(form), half_rows(form, operands == "bf16")
    lengths = M.model(form)._get_feat_extract_output_lengths
    want_frames = FRAMES + [1499] if form == "A" else FRAMES
    assert [int(lengths(torch.tensor(max(e - b, 400)))) for _, b, e in segs] == want_frames == [len(r) for r in ref]
    de = run(engine, form, segs)
    got = de.numpy()
    assert isinstance(de, DeviceEmissions) and de.n_cols == M.FORMS[form]["vocab_size"] and de.n_frames.tolist() == want_frames
    assert de.row_start.tolist() == np.concatenate([[0], np.cumsum(de.n_frames)[:-1]]).tolist()
    assert [g.shape for g in got] == [r.shape for r in ref] and all(np.all(np.isfinite(g)) for g in got)
    short = [k for k, f in enumerate(want_frames) if f <= 2]
    assert len(short) == 5
    pick = lambda rows, ks: [rows[k] for k in ks]
    dh, dd = rel_l2(half, ref), rel_l2(got, ref)
    dhs, dds = rel_l2(pick(half, short), pick(ref, short)), rel_l2(pick(got, short), pick(ref, short))
    key = f"{form} {operands}"
    line = (f"{key}: segments {len(segs)} frames {sum(want_frames)}  all: d_half {dh:.6e} d_device {dd:.6e} bound {4 * dh:.6e}  "
            f"short: d_half {dhs:.6e} d_device {dds:.6e} bound {4 * dhs:.6e}")
    print("w2v segment emissions", line)
    _record(key, line)
    assert 0 < dh < 0.02 and 0 < dhs < 0.02
    assert dd <= 4 * dh
    assert dds <= 4 * dhs


# ------------------------------------------------------------------------------------------------------------ 4. independence, bit for bit
@pytest.mark.parametrize("form", ["A", "B"])
def test_batch_order_chunks_and_history_do_not_change_a_bit(engine, form):
    segs = SEGMENTS + [LONG]
    whole = run(engine, form, segs).numpy()
    assert [len(w) for w in whole] == FRAMES + [1499]
    for k, seg in enumerate(segs):
        assert _same_bits(run(engine, form, [seg]).numpy()[0], whole[k]), ("alone", k)
    chunks, computed, valid = engine.w2v_segments_plan()          # (of the latest call: one segment of one frame in a slot of 16 rows ... 1 499 in 1 504)
    assert (chunks, computed, valid) == (1, 1504, 1499)
    back = run(engine, form, segs[::-1]).numpy()
    chunks, computed, valid = engine.w2v_segments_plan()
    assert valid == sum(FRAMES) + 1499 and valid <= computed <= 2 * (valid + 15 * len(segs)) and 2 <= chunks <= 7
    assert all(_same_bits(a, b) for a, b in zip(back[::-1], whole))
    for per_chunk in (1, 2):
        other = run(engine, form, segs, segments_per_chunk=per_chunk).numpy()
        assert all(_same_bits(a, b) for a, b in zip(other, whole)), per_chunk
    # stale rows in every reused buffer: the long segment's call, then the short ones under other slot strides
    for short in (SEGMENTS[:5], SEGMENTS):
        assert len(run(engine, form, [LONG]).numpy()[0]) == 1499
        after = run(engine, form, short).numpy()
        assert all(_same_bits(a, b) for a, b in zip(after, whole))


# ------------------------------------------------------------------------------------------------------------ 5. the chain
DICTIONARY = dict({"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, "'": 5}, **{ch: 6 + i for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz")})
METADATA = {"language": "fr", "dictionary": DICTIONARY, "type": "huggingface"}


def test_wx_align_reads_segment_emissions_in_place(engine):
    de = run(engine, "A", SEGMENTS[5:])
    fetched = de.numpy()
    rng = np.random.default_rng(8)
    tokens = [rng.integers(1, 32, size=max(1, int(t) // 5)).astype(np.int32) for t in de.n_frames]
    on_device, on_host = engine.wx_align(de, tokens), engine.wx_align(fetched, tokens)
    assert len(on_device) == len(on_host) == 9
    for a, b in zip(on_device, on_host):
        assert a["status"] == b["status"] == 0 and sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert all(_same_bits(x, y) for x, y in zip(fetched, de.numpy()))      # read in place, not written
    newer = run(engine, "A", SEGMENTS[:3])
    with pytest.raises(ValueError, match="stale"):
        engine.wx_align(de, tokens)
    assert len(newer) == 3


def test_align_and_process_files_on_the_engine(engine, tmp_path, capsys):
    from prosody_control_french_tts_amd import synth
    from prosody_control_french_tts_amd.Aligners import whisperX
    model = M.model("A")
    pcm = {"c0": synth.synth_clip(0, seconds=2.0), "c1": synth.synth_clip(1, seconds=1.5)}
    segments = {"c0.wav": [{"start": 0.1, "end": 1.05, "text": " bonjour le monde"}, {"start": 1.05, "end": 1.9, "text": "la petite maison "}],
                "c1.wav": [{"start": 0.5, "end": 0.6, "text": "  "}, {"start": 0.0, "end": 1.4, "text": "il arrive demain"}, {"start": 1.5, "end": 1.6, "text": "trop tard"}]}
    alignable = {"c0.wav": segments["c0.wav"], "c1.wav": segments["c1.wav"][1:2]}
    # align: the engine's forward, against the same emissions fetched to host arrays and handed in
    got = whisperX.align(segments["c0.wav"], model, METADATA, pcm["c0"], engine, acoustic="engine")
    held = CE.engine_segment_emissions(engine, model, [(pcm["c0"], alignable["c0.wav"])]).numpy()
    assert [len(e) for e in held] == [(int(s["end"] * 16000) - int(s["start"] * 16000) - 400) // 320 + 1 for s in alignable["c0.wav"]]
    assert got == whisperX.align(segments["c0.wav"], None, METADATA, pcm["c0"], engine, emissions=held)
    assert [w["word"] for w in got["word_segments"]] == "bonjour le monde la petite maison".split()
    # process_files: every alignable segment of both files in one forward call and one wx_align
    audio, trans = tmp_path / "audio", tmp_path / "txt"
    audio.mkdir(); trans.mkdir()
    for name, x in pcm.items():
        with wave.open(str(audio / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(x.tobytes())
        (trans / f"{name}.txt").write_text("", encoding="utf-8")
    words = whisperX.process_files(str(audio), str(trans), str(tmp_path / "tg"), engine=engine, align_model=model, metadata=METADATA, segments=segments,
                                   acoustic="engine")
    assert capsys.readouterr().out.count("Processed file : ") == 2
    both = CE.engine_segment_emissions(engine, model, [(pcm[n[:2]], alignable[n]) for n in sorted(alignable)]).numpy()
    words2 = whisperX.process_files(str(audio), str(trans), str(tmp_path / "tg2"), engine=engine, align_model=None, metadata=METADATA, segments=segments,
                                    emissions={"c0.wav": both[:2], "c1.wav": both[2:]})
    read = lambda d: {n: open(os.path.join(str(tmp_path / d), n), encoding="utf-8").read() for n in sorted(os.listdir(str(tmp_path / d)))}
    assert words == words2 and words["c0.wav"] == got["word_segments"] and [w["word"] for w in words["c1.wav"]] == "il arrive demain".split()
    assert read("tg") == read("tg2") and sorted(read("tg")) == ["c0.TextGrid", "c1.TextGrid"] and all("Mots" in t for t in read("tg").values())
    # acoustic="torch" is the default and is untouched: the caller's model under torch, close to the engine's words
    on_torch = copy.deepcopy(model).to("cuda:0")
    default = whisperX.align(segments["c0.wav"], on_torch, METADATA, pcm["c0"], engine)
    assert default == whisperX.align(segments["c0.wav"], on_torch, METADATA, pcm["c0"], engine, acoustic="torch")
    assert [w["word"] for w in default["word_segments"]] == [w["word"] for w in got["word_segments"]]
    with pytest.raises(ValueError, match="acoustic"):
        whisperX.align(segments["c0.wav"], model, METADATA, pcm["c0"], engine, acoustic="hip")


# ------------------------------------------------------------------------------------------------------------ 6. errors
def test_errors(engine):
    import prosody_control_french_tts_amd as P
    with P.ProsodyEngine(0) as fresh:
        fresh.upload([clips()[1]], 16000)
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_segment_emissions([(0, 0, 400)])                # run before load
        fresh.w2v_load(M.model("A"))
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_fetch(0)                                        # loaded, still no run
        for bad in [(1, 0, 400), (-1, 0, 400), (0, -1, 400), (0, 500, 400), (0, 0, 40001)]:
            with pytest.raises(PceError, match="status -1"):          # clip out of range; 0 <= begin <= end <= length violated
                fresh.w2v_segment_emissions([(0, 0, 400), bad])
        with pytest.raises(PceError, match="status -1.*no frame"):
            fresh.w2v_segment_emissions([(0, 0, 100)], min_samples=0)
        fresh.upload([_speechlike(4410, 9)], 44100)
        with pytest.raises(PceError, match="status -1.*16000 Hz"):
            fresh.w2v_segment_emissions([(0, 0, 400)])
        fresh.upload([np.zeros((1 << 26) + 1, np.int16)], 16000)
        with pytest.raises(PceError, match="status -5"):              # the longest segment is beyond pce_w2v_run's 2^26 samples (refused before any launch)
            fresh.w2v_segment_emissions([(0, 0, 400), (0, 0, (1 << 26) + 1)])
        fresh.upload([clips()[1]], 16000)
        with pytest.raises(PceError, match="status -4"):
            fresh.w2v_fetch(0)                                        # a refused run leaves nothing to fetch
        de = fresh.w2v_segment_emissions([(0, 0, 40000), (0, 0, 0)], star=True)
        assert de.n_frames.tolist() == [124, 1] and de.n_cols == 33 and np.all(de.numpy()[1][:, -1] == 0)
        assert fresh.w2v_segment_emissions([]).n_frames.tolist() == []
        with pytest.raises(ValueError, match="stale"):
            de.numpy()                                                # from before a later run: refused, not read
        with pytest.raises(PceError, match="status -1"):
            fresh.w2v_fetch(0)                                        # the later run held no segment
