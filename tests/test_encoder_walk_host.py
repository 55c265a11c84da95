"""CPU tests of tests/encoder_walk_restatement.py, the checker of the shared encoder layer walk (tests/test_gpu_encoder_walk.py runs it on the device):

  * its float64 layer, composed without any rounding, is the layer transformers' own modules compute (BertLayer, Wav2Vec2EncoderLayer,
    Wav2Vec2EncoderLayerStableLayerNorm, WhisperEncoderLayer in float64, the attention mask built from the lengths), to 1e-10 relative per element;
  * every check bites: the stand-in for the device (the restatement with each stage output rounded to the type the device stores) passes every stage
    check on the GPU test's own inputs, and each of nine wrong walks leaves the bound at the stage it belongs to and at no earlier one."""
import functools

import numpy as np
import pytest
import torch

from tests import encoder_walk_restatement as R
from tests.conftest import OPERANDS

torch.set_num_threads(min(16, torch.get_num_threads()))
SEED = 20

# ---------------------------------------------------------------------------------------------------------------
# the pin to transformers
# ---------------------------------------------------------------------------------------------------------------
PIN = dict(d=128, heads=2, inner=512, rows=40, lens=(1, 17, 40))


def _hf_layer(kind):
    """(module in float64 with dropout off, {our tensor name: its parameter name})"""
    d, H, I = PIN["d"], PIN["heads"], PIN["inner"]
    if kind == "bert":
        from transformers import BertConfig
        from transformers.models.bert.modeling_bert import BertLayer
        cfg = BertConfig(hidden_size=d, num_attention_heads=H, intermediate_size=I, layer_norm_eps=1e-12, hidden_dropout_prob=0.0,
                         attention_probs_dropout_prob=0.0, hidden_act="gelu")
        cfg._attn_implementation = "eager"
        names = dict(q="attention.self.query", k="attention.self.key", v="attention.self.value", out="attention.output.dense",
                     ln1="attention.output.LayerNorm", fc1="intermediate.dense", fc2="output.dense", ln2="output.LayerNorm")
        return BertLayer(cfg), names
    if kind in ("w2v-post-ln", "w2v-pre-ln"):
        from transformers import Wav2Vec2Config
        from transformers.models.wav2vec2.modeling_wav2vec2 import Wav2Vec2EncoderLayer, Wav2Vec2EncoderLayerStableLayerNorm
        cfg = Wav2Vec2Config(hidden_size=d, num_attention_heads=H, intermediate_size=I, layer_norm_eps=1e-5, hidden_dropout=0.0, attention_dropout=0.0,
                             activation_dropout=0.0, hidden_act="gelu")
        cfg._attn_implementation = "eager"
        names = dict(q="attention.q_proj", k="attention.k_proj", v="attention.v_proj", out="attention.out_proj", ln1="layer_norm",
                     fc1="feed_forward.intermediate_dense", fc2="feed_forward.output_dense", ln2="final_layer_norm")
        return (Wav2Vec2EncoderLayer if kind == "w2v-post-ln" else Wav2Vec2EncoderLayerStableLayerNorm)(cfg), names
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoderLayer
    cfg = WhisperConfig(d_model=d, encoder_attention_heads=H, encoder_ffn_dim=I, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                        activation_function="gelu")
    cfg._attn_implementation = "eager"
    names = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", out="self_attn.out_proj", ln1="self_attn_layer_norm", fc1="fc1", fc2="fc2",
                 ln2="final_layer_norm")
    return WhisperEncoderLayer(cfg), names


@pytest.mark.parametrize("kind", ["bert", "w2v-post-ln", "w2v-pre-ln", "whisper-tiled"])
def test_float64_layer_is_transformers_layer(kind):
    base = R.FORMS["bert" if kind == "bert" else kind]
    form = dict(base, d=PIN["d"], heads=PIN["heads"], inner=PIN["inner"], rows=PIN["rows"], lens=PIN["lens"])
    W = R.draw_weights(form, 1, seed=3)[0]
    module, names = _hf_layer(kind)
    module = module.double().eval()
    params = dict(module.named_parameters())
    with torch.no_grad():
        for ours, theirs in names.items():
            params[theirs + ".weight"].copy_(torch.from_numpy(W[ours + "_w"].astype(np.float64)))
            if W[ours + "_b"] is None:
                assert theirs + ".bias" not in params, theirs
            else:
                params[theirs + ".bias"].copy_(torch.from_numpy(W[ours + "_b"].astype(np.float64)))
    assert len(params) == 16 - (0 if form["key_bias"] else 1)          # nothing of the module keeps its random initialisation
    lens, rows = form["lens"], form["rows"]
    x = np.random.default_rng(4).standard_normal((len(lens) * rows, form["d"]))
    got = R.layer_float64(form, W, x, lens, rows)
    keys = torch.arange(rows)[None, :] < torch.tensor(lens)[:, None]
    mask = torch.zeros(len(lens), 1, 1, rows, dtype=torch.float64).masked_fill(~keys[:, None, None, :], torch.finfo(torch.float64).min)
    with torch.no_grad():
        want = module(torch.from_numpy(x).reshape(len(lens), rows, -1), attention_mask=mask.expand(-1, 1, rows, -1))
    want = (want[0] if isinstance(want, tuple) else want).reshape(-1, form["d"]).numpy()
    ok = R.valid_mask(lens, rows)
    rel = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    assert rel.max() <= 1e-10, (kind, float(rel.max()))


def test_blob_order_follows_the_loaders():
    """openai-whisper's order for the Whisper form (LayerNorm first), transformers' for the others; k.b only where the form has one"""
    for name, form in R.FORMS.items():
        small = dict(form, d=128, heads=2, inner=128)
        W = R.draw_weights(small, 2, seed=1)
        b = R.blob(W, small)
        d, I = 128, 128
        assert b.size == 2 * (4 * d * d + (4 if form["key_bias"] else 3) * d + 2 * d * I + I + d + 4 * d), name
        first = W[0]["ln1_w"] if name == "whisper-tiled" else W[0]["q_w"].ravel()
        assert np.array_equal(b[:first.size], first), name
        assert np.array_equal(b[b.size // 2:][:first.size], (W[1]["ln1_w"] if name == "whisper-tiled" else W[1]["q_w"].ravel())), name


# ---------------------------------------------------------------------------------------------------------------
# every check bites
# ---------------------------------------------------------------------------------------------------------------
def _ops(name):
    return dict(OPERANDS[name], name=name)


@functools.lru_cache(maxsize=None)
def _problem(form_name):
    form = R.FORMS[form_name]
    W = R.draw_weights(form, 2, SEED)
    x = R.draw_stream(form, SEED)
    return form, W, x


def _run(form_name, ops_name, mut=None):
    form, W, x = _problem(form_name)
    ops = _ops(ops_name)
    ln_in = None if form["pre_ln"] else R.bits(x, ops)
    st = R.standin(form, W, x, ln_in, ops, mut)
    return form, st, R.check_stages(form, W, x, ln_in, st, ops), ops


LAUNCH = {"ln_b_x": "ln_b", "ln_c_x": "ln_c", "vt": "qk"}          # a capture -> the launch that wrote it


def _first_failure(ratios):
    for layer, stage, r in ratios:
        if not r <= 1.0:
            return layer, stage
    return None


@pytest.mark.parametrize("ops_name", ["fp16", "bf16"])
@pytest.mark.parametrize("form_name", sorted(R.FORMS))
def test_standin_passes_every_stage(form_name, ops_name):
    form, st, ratios, ops = _run(form_name, ops_name)
    for layer, stage, r in ratios:
        print(f"standin-ratio {form_name} {ops_name} layer {layer} {stage}: {r:.4f}")
    assert [s for _, s, _ in ratios] == list(R.stage_names(form)) * 2
    assert _first_failure(ratios) is None, ratios
    assert R.structure_failures(form, st, ops) == []
    for a in st.values():                                           # the +-60000 pad rows stay finite through every stage, in fp16 too
        written = a[~np.isnan(a)] if a.dtype == np.float32 else R.val(a[a != R.SENTINEL16], ops)
        assert np.isfinite(written).all()


# mutation -> (the forms it is applied to, the layer and launch whose check must be the first to fail: pre-LN / post-LN)
CASES = {
    "eps": (("bert", "bert-full-slot"), (0, "ln_b")),
    "key_bias": (("whisper-tiled",), (0, "qk")),
    "mask_long": (("bert", "w2v-pre-ln"), (0, "attn")),
    "mask_short": (("bert", "bert-full-slot", "w2v-pre-ln"), (0, "attn")),
    "ln_before_add": (("bert", "w2v-post-ln"), (0, "ln_b")),
    "tanh_gelu": (("bert", "w2v-pre-ln"), (0, "hidden")),
    "layer1_weights": (("bert", "w2v-pre-ln"), None),
    "vt_pitch": (("bert", "w2v-pre-ln"), (0, "qk")),
    "ln_not_written_back": (("bert", "w2v-post-ln"), (0, "ln_b")),
}


@pytest.mark.filterwarnings("ignore:invalid value encountered")      # (behind its failing stage a wrong walk may overflow fp16: inf - inf in the checker's products)
@pytest.mark.parametrize("ops_name", ["fp16", "bf16"])
@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_fails_at_its_stage(mut, ops_name):
    forms, where = CASES[mut]
    for form_name in forms:
        form, st, ratios, ops = _run(form_name, ops_name, mut)
        want = where if where is not None else (1, "ln_a" if form["pre_ln"] else "qk")
        got = _first_failure(ratios)
        assert got is not None, (mut, form_name, ops_name, "inside every bound", ratios)
        assert (got[0], LAUNCH.get(got[1], got[1])) == want, (mut, form_name, ops_name, got, ratios)
