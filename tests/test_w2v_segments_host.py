"""Host side of the wav2vec2 forward pass over segments of unequal length (no GPU): the declarations of ``pce_w2v_run_segments`` /
``pce_w2v_segment_frames``, the frame arithmetic against ``transformers``' own length function, the chunk plan (csrc/pce_w2v_seg_plan.h) alone
under AddressSanitizer and UndefinedBehaviorSanitizer (tests/host/w2v_seg_plan_main.cpp, a child process: nothing is loaded into this
interpreter), and the sample arithmetic of ``ctc_emissions.engine_segment_emissions`` against ``segment_emissions``' slicing."""
import ctypes
import fnmatch
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_models as M
from prosody_control_french_tts_amd import engine as E
from prosody_control_french_tts_amd import w2v_weights as WW
from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc")
SYMBOLS = {"pce_w2v_run_segments", "pce_w2v_segments_plan", "pce_w2v_segment_frames", "pce_selftest_w2v_wave_segments", "pce_selftest_w2v_posconv_segments"}
# sample count -> frames of the standard seven-layer stack (receptive field 400, stride 320)
TABLE = {400: 1, 719: 1, 720: 2, 5200: 16, 5520: 17, 12000: 37, 20240: 63, 20560: 64, 20880: 65, 34000: 106, 82320: 257, 479999: 1499}


def test_header_library_table_and_map_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pce.h"), encoding="utf-8").read()
    declared = set(re.findall(r"^\s*(?:int|const char \*|void)\s+\*?(pce_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert SYMBOLS <= declared and SYMBOLS <= set(E.EXPORTS)
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 21
    assert re.search(r"typedef struct pce_w2v_segment \{ int32_t clip; int32_t reserved; int64_t begin, end; \} pce_w2v_segment;", header)
    assert re.search(r"typedef struct pce_w2v_seg_plan \{ int32_t min_samples[^;]*, segments_per_chunk[^;]*, star; \} pce_w2v_seg_plan;", header)
    assert ctypes.sizeof(E.W2vSegment) == 24 and ctypes.sizeof(E.W2vSegPlan) == 12
    # no kernel id came with them: the positions the other host tests pin are where they were
    ids = header[header.index("enum pce_kernel_id"):]
    ids = [x for x in re.findall(r"\bPCE_K_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", ids, flags=re.S)) if x != "PCE_K_COUNT"]
    assert len(ids) == len(E.KERNEL_IDS) and not any("SEG" in x for x in ids)
    lib = E.load_library()
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 21 and all(hasattr(lib, s) for s in SYMBOLS)
    # both operand builds: a line of the entries table (declared in both namespaces, forwarded once), or written out in the dispatch file
    table = set(re.findall(r"^\s*X\((pce_[a-z0-9_]+),", open(os.path.join(CSRC, "pce_whisper_entries.h"), encoding="utf-8").read(), flags=re.M))
    dispatch = open(os.path.join(CSRC, "pce_whisper_dispatch.hip"), encoding="utf-8").read()
    assert SYMBOLS - {"pce_w2v_segment_frames"} <= table
    assert re.search(r"^int pce_w2v_segment_frames\(", dispatch, flags=re.M) and "pce_w2v_segment_frames" not in table
    # the version script exports them
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "libpce.map"), encoding="utf-8").read(), flags=re.S)
    exported = re.search(r"global:(.*?)local:", script, flags=re.S).group(1).replace(";", " ").split()
    assert all(any(fnmatch.fnmatchcase(s, pattern) for pattern in exported) for s in SYMBOLS)


def _configs():
    import transformers
    stride4 = transformers.Wav2Vec2Config(conv_dim=(128,) * 7, conv_stride=(4, 5, 2, 2, 2, 2, 1), conv_kernel=(10, 5, 3, 3, 3, 2, 2), num_hidden_layers=1,
                                          hidden_size=128, num_attention_heads=2, intermediate_size=128)
    assert int(np.prod(stride4.conv_stride)) == 320
    return {"A": M.config("A"), "B": M.config("B"), "stride-4": stride4}


@pytest.mark.parametrize("which", ["A", "B", "stride-4"])
def test_segment_frames_equal_transformers_lengths(which):
    import torch
    import transformers
    config = _configs()[which]
    lengths = transformers.Wav2Vec2Model(config)._get_feat_extract_output_lengths if which == "stride-4" else M.model(which)._get_feat_extract_output_lengths
    dims = WW.dims(config)
    lib = E.load_library()
    counts = list(range(0, 2001)) + sorted(TABLE)
    want = lengths(torch.tensor(counts, dtype=torch.long)).tolist()
    got = [E.w2v_segment_frames(dims, n, 0, lib) for n in counts]
    assert got == [max(0, w) for w in want]                      # (below the receptive field the formula goes to zero or below: no frame)
    if which != "stride-4":
        assert {n: E.w2v_segment_frames(dims, n, 400, lib) for n in TABLE} == TABLE
        assert {n: int(lengths(torch.tensor(n))) for n in TABLE} == TABLE
    # fewer than min_samples: the frames of min_samples; begin == end included
    field = E.w2v_segment_frames(dims, 400, 0, lib)
    assert [E.w2v_segment_frames(dims, n, 400, lib) for n in (0, 1, 123, 399, 400)] == [field] * 5 and field == (0 if which == "stride-4" else 1)
    nf = ctypes.c_int64()
    assert lib.pce_w2v_segment_frames(None, 400, 400, ctypes.byref(nf)) == -1
    assert lib.pce_w2v_segment_frames(ctypes.byref(E.W2vDims.of(dims)), -1, 400, ctypes.byref(nf)) == -1
    assert lib.pce_w2v_segment_frames(ctypes.byref(E.W2vDims.of(dims)), 400, -1, ctypes.byref(nf)) == -1


def test_chunk_plan_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "w2v_seg_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "w2v_seg_plan_main.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr}"
    assert "one long among 300 short" in r.stdout


class _Recorder:
    """Stands in for the engine: records what engine_segment_emissions uploads and asks for."""

    def __init__(self):
        self.loaded = self.clips = self.rate = self.segments = self.args = None

    def w2v_holds(self, model):
        return self.loaded is model

    def w2v_load(self, model):
        self.loaded = model

    def upload(self, clips, rate):
        self.clips, self.rate = clips, rate

    def w2v_segment_emissions(self, segments, min_samples=400, segments_per_chunk=None, star=False):
        self.segments, self.args = list(segments), (min_samples, segments_per_chunk, star)
        return "emissions"


def test_engine_segment_emissions_takes_the_samples_segment_emissions_slices():
    rng = np.random.default_rng(3)
    files = [rng.integers(-3000, 3000, 40000).astype(np.int16), rng.integers(-3000, 3000, 8000).astype(np.int16)]
    cases = [   # fractional times whose products round either way, an end beyond the clip, start == end, a start beyond the clip, end < start
        {"start": 0.0, "end": 0.3333}, {"start": 0.10003, "end": 1.29999}, {"start": 1.1, "end": 2.2}, {"start": 0.7, "end": 0.7},
        {"start": 2.0, "end": 9.75}, {"start": 2.49995, "end": 2.5}, {"start": 0.29, "end": 0.57}, {"start": 0.4, "end": 0.1},
    ]
    jobs = [(files[0], cases), (files[1], [{"start": 0.25, "end": 0.5}, {"start": 0.49999, "end": 0.6}, {"start": 0.7, "end": 0.2}])]
    eng, model = _Recorder(), object()
    assert CE.engine_segment_emissions(eng, model, jobs) == "emissions"
    assert eng.loaded is model and eng.rate == 16000 and eng.args == (CE.MIN_SEGMENT_SAMPLES, None, False) == (400, None, False)
    assert len(eng.clips) == 2 and all(c.dtype == np.int16 and np.array_equal(c, f) for c, f in zip(eng.clips, files))
    k = 0
    for clip, (pcm, segments) in enumerate(jobs):
        for seg in segments:
            piece = pcm[int(seg["start"] * 16000):int(seg["end"] * 16000)]           # segment_emissions' slice
            q, begin, end = eng.segments[k]
            assert q == clip and 0 <= begin <= end <= len(pcm) and np.array_equal(pcm[begin:end], piece), seg
            assert CE.segment_samples(seg, len(pcm)) == (begin, end)
            k += 1
    assert k == len(eng.segments) == 11
    assert eng.segments[4] == (0, 32000, 40000) and eng.segments[3][1] == eng.segments[3][2] and eng.segments[2] == (0, 17600, 35200)
    eng.w2v_load = None                                              # the engine holds the model: no second load
    assert CE.engine_segment_emissions(eng, model, jobs[:1]) == "emissions" and len(eng.segments) == 8
    with pytest.raises(ValueError, match="negative"):
        CE.engine_segment_emissions(eng, model, [(files[0], [{"start": -0.1, "end": 1.0}])])
    with pytest.raises(ValueError, match="int16"):
        CE.engine_segment_emissions(eng, model, [(files[0].astype(np.float32), cases)])


def test_acoustic_is_torch_or_engine():
    from prosody_control_french_tts_amd.Aligners import whisperX
    with pytest.raises(ValueError, match="acoustic"):
        whisperX.align([], None, {"dictionary": {}, "language": "fr"}, np.zeros(16, np.int16), None, acoustic="hip")
    out = whisperX.align([], None, {"dictionary": {}, "language": "fr"}, np.zeros(16, np.int16), None, acoustic="engine")
    assert out == {"segments": [], "word_segments": []}
