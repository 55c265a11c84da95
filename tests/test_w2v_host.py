"""Host side of the wav2vec2 / MMS forward pass (no GPU): the packer and its weight-norm fold, the blob's size, the limits the loader states,
the window plan of the new path against ``ctc_emissions.window_plan``, and the library's declarations."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import w2v_models as M
from prosody_control_french_tts_amd import engine as E
from prosody_control_french_tts_amd import w2v_weights as WW
from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"pce_w2v_check", "pce_w2v_load", "pce_w2v_run", "pce_w2v_shape", "pce_w2v_fetch", "pce_w2v_device", "pce_w2v_window_plan", "pce_selftest_w2v_wave",
           "pce_selftest_w2v_lngelu", "pce_selftest_w2v_posconv"}


def _pos_weight_in_blob(blob, dims):
    off = 0
    for name, shape in WW.tensor_order(dims):
        n = int(np.prod(shape))
        if name == WW.POS_W:
            return blob[off:off + n].reshape(shape)
        off += n
    raise AssertionError("no positional convolution in tensor_order")


@pytest.mark.parametrize("form", ["A", "B"])
@pytest.mark.parametrize("spelling", ["parametrizations", "weight_g_v"])
def test_pack_folds_the_weight_norm(form, spelling):
    """pack, then the blob's [out][tap][in] back as [out][in][tap], reproduces pos_conv_embed.conv.weight (what the module's forward multiplies
    by) to 1e-6, from either spelling of the weight norm's parameters; masked_spec_embed is dropped, the wav2vec2. prefix optional."""
    model = M.model(form)
    dims = WW.dims(model.config)
    sd = dict(model.state_dict())
    assert any(k.endswith("masked_spec_embed") for k in sd)
    if spelling == "weight_g_v":                                       # the spelling of checkpoints saved before torch's parametrizations
        pre = "wav2vec2.encoder.pos_conv_embed.conv."
        sd[pre + "weight_g"] = sd.pop(pre + "parametrizations.weight.original0")
        sd[pre + "weight_v"] = sd.pop(pre + "parametrizations.weight.original1")
        sd = {k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k: v for k, v in sd.items()}      # ... and a body without the prefix
    blob = WW.pack(sd, dims)
    assert blob.dtype == np.float32 and blob.size == WW.n_floats(dims)
    want = model.wav2vec2.encoder.pos_conv_embed.conv.weight.detach().numpy()
    got = WW.unfold_pos_conv(_pos_weight_in_blob(blob, dims))
    assert got.shape == want.shape == (dims["n_state"], dims["n_state"] // dims["pos_groups"], 128)
    assert np.max(np.abs(got - want)) <= 1e-6
    # the norm is per tap, over dimensions 0 and 1
    g = model.state_dict()["wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0"].numpy()
    assert g.shape == (1, 1, 128) and np.allclose(np.sqrt((got.astype(np.float64) ** 2).sum(axis=(0, 1))), g.reshape(-1), rtol=1e-5)


def test_blob_size_and_dims():
    a, b = WW.dims(M.config("A")), WW.dims(M.config("B"))
    assert (a["feat_norm"], a["conv_bias"], a["stable_ln"], a["pos_groups"], a["n_head"]) == (0, 0, 0, 8, 6)
    assert (b["feat_norm"], b["conv_bias"], b["stable_ln"], b["pos_groups"], b["n_head"]) == (1, 1, 1, 4, 4)
    for form, dims in (("A", a), ("B", b)):
        params = sum(p.numel() for n, p in M.model(form).named_parameters() if "masked_spec_embed" not in n)
        d = dims["n_state"]
        assert d % dims["pos_groups"] == 0 and WW.n_floats(dims) == params - 128       # the weight norm's 128 gains leave, v becomes the weight
        with pytest.raises(ValueError):
            WW.pack({k: v for k, v in M.model(form).state_dict().items() if "lm_head.bias" not in k} | {"lm_head.bias": torch.zeros(3)}, dims)
    s = E.W2vDims.of(a)
    assert list(s.conv_kernel)[:7] == [10, 3, 3, 3, 3, 2, 2] and list(s.conv_stride)[:7] == [5, 2, 2, 2, 2, 2, 2] and s.n_conv == 7
    assert ctypes.sizeof(E.W2vDims) == 4 * (1 + 24 + 10) + 4 and ctypes.sizeof(E.W2vPlan) == 16


LIMITS = [   # (what changes, the message names)
    (dict(n_conv=6, conv_dim=(128,) * 6, conv_kernel=(10, 3, 3, 3, 3, 2), conv_stride=(5, 2, 2, 2, 2, 2)), "feature-encoder layers"),
    (dict(conv_kernel=(8, 3, 3, 3, 3, 2, 2)), "taps at stride"),
    (dict(conv_stride=(9, 2, 2, 2, 2, 2, 2)), "taps at stride"),
    (dict(conv_dim=(128, 128, 96, 128, 128, 128, 128)), "channels"),
    (dict(conv_dim=(1088,) + (128,) * 6), "channels"),
    (dict(conv_dim=(64, 128, 128, 128, 128, 128, 128), conv_kernel=(10, 1, 3, 3, 3, 2, 3)), None),          # K = 1 x 64 and 3 x 128: whole K steps, both fit
    (dict(n_state=320, n_head=5), "n_state"),
    (dict(n_head=3), "head size 64"),
    (dict(n_state=2176, n_head=34, pos_groups=34), "LayerNorm"),
    (dict(n_inter=576), "n_inter"),
    (dict(pos_taps=64), "taps"),
    (dict(pos_groups=2), "columns per group"),
    (dict(pos_groups=16), "columns per group"),
]


@pytest.mark.parametrize("change,names", LIMITS)
def test_each_limit_is_refused_at_load(change, names):
    """pce_w2v_check is pce_w2v_load's own condition list (the loader calls it first): PCE_E_LIMIT with a message per limit, PCE_E_INVALID for a
    blob of the wrong size, PCE_OK for the two test models and for the published base / large widths."""
    dims = dict(WW.dims(M.config("A")), **change)
    rc, msg = E.w2v_check(dims, WW.n_floats(dims))
    if names is None:
        assert (rc, msg) == (0, "")
    else:
        assert rc == -5 and names in msg, (rc, msg)


def test_blob_size_and_published_widths():
    for form in "AB":
        dims = WW.dims(M.config(form))
        assert E.w2v_check(dims, WW.n_floats(dims)) == (0, "")
        rc, msg = E.w2v_check(dims, WW.n_floats(dims) - 1)
        assert rc == -1 and "floats, expected" in msg
    import transformers
    base = WW.dims(transformers.Wav2Vec2Config(vocab_size=32))
    large = WW.dims(transformers.Wav2Vec2Config(vocab_size=32, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                                                feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True))
    for dims in (base, large):
        assert E.w2v_check(dims, WW.n_floats(dims)) == (0, "")
    assert (base["n_state"] // base["pos_groups"], large["n_state"] // large["pos_groups"]) == (48, 64)


@pytest.mark.parametrize("window_s,context_s", [(2, 0.5), (30, 2)])
def test_window_plan_equals_the_torch_path(window_s, context_s):
    window = int(window_s * 16000)
    for n in (1, window, window + 1, int(4.7 * window)):
        n_win, _, keep = CE.window_plan(n, window_s, context_s)
        assert E.w2v_window_plan(n, window_s, context_s) == (n_win, keep), n
    assert E.w2v_window_plan(1, window_s, context_s)[0] == 1 and E.w2v_window_plan(int(4.7 * window), window_s, context_s)[0] == 5


def test_header_and_library_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "pce.h"), encoding="utf-8").read()
    declared = set(re.findall(r"^\s*(?:int|const char \*|void)\s+\*?(pce_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert SYMBOLS <= declared and SYMBOLS <= set(E.EXPORTS)
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 16
    assert "PCE_W2V_IMAGE_BUDGET" in header and re.search(r"typedef struct pce_w2v_dims", header) and re.search(r"typedef struct pce_w2v_plan", header)
    ids = header[header.index("enum pce_kernel_id"):]
    ids = [x for x in re.findall(r"\bPCE_K_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", ids, flags=re.S)) if x != "PCE_K_COUNT"]
    new = ["PCE_K_W2V", "PCE_K_W2V_WAVE", "PCE_K_W2V_POSCONV", "PCE_K_W2V_TAIL"]
    assert [E.KERNEL_IDS[ids.index(x)] for x in new] == ["w2v_forward", "k_w2v_wave", "k_w2v_posconv", "k_w2v_tail"]
    assert ids.index("PCE_K_CREPE_VITERBI") < ids.index(new[0]) and ids.index(new[-1]) < ids.index("PCE_K_CTC") and len(ids) == len(E.KERNEL_IDS)
    lib = E.load_library()
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 16 and all(hasattr(lib, s) for s in SYMBOLS)
    assert [lib.pce_kernel_name(i).decode() for i in range(len(E.KERNEL_IDS))] == E.KERNEL_IDS
    # every symbol is wired into both operand builds: a line of the table that both builds' declarations and the exported forwarders are generated
    # from, or a function the dispatch file writes out
    csrc = os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc")
    table = set(re.findall(r"^\s*X\((pce_[a-z0-9_]+),", open(os.path.join(csrc, "pce_whisper_entries.h"), encoding="utf-8").read(), flags=re.M))
    dispatch = open(os.path.join(csrc, "pce_whisper_dispatch.hip"), encoding="utf-8").read()
    assert dispatch.count("PCE_WHISPER_ENTRIES(PCE_DECLARE)") == 2 and dispatch.count("PCE_WHISPER_ENTRIES(PCE_FORWARD)") == 1
    assert "PCE_WHISPER_ENTRIES(PCE_DECLARE)" in open(os.path.join(csrc, "pce_whisper_impl.inc"), encoding="utf-8").read()
    for s in SYMBOLS - {"pce_w2v_window_plan"}:
        assert s in table or re.search(r"^int %s\(" % s, dispatch, flags=re.M), s
