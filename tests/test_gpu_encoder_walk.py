"""The shared encoder layer walk (csrc/pce_encoder.inc: encoder_walk) stage by stage against float64, through pce_selftest_encoder_walk: the product's
own weight packer, run description and walk instantiation, with the buffer behind every launch copied out.  Five forms -- Whisper's audio encoder on the
tiled kernels, BERT at ragged lengths and with a full 512-token slot, wav2vec2 post-LN and pre-LN -- each with two layers of different weights.

Every element of every stage is checked against tests/encoder_walk_restatement.py's stage on the buffer THE DEVICE left in front of it, so each bound is one
kernel's (the single-kernel tests' own bounds: tests/test_gpu_kernels.py, tests/test_gpu_attention.py); tests/test_encoder_walk_host.py pins that
restatement to transformers' modules and shows on the CPU that every one of these checks fails for a walk that is wrong in the way it guards against.

Beside the bounds: the K half of Whisper's projection carries exactly no bias; attention rows at and behind an item's length keep the sentinel and V^T
columns at and behind rows_per_item their zeros; a post-LN LayerNorm's 16-bit image is its written-back fp32 stream rounded once, bit for bit; the valid
rows of every stage do not change by one bit when the pad rows hold zeros instead of +-60000, nor when an item runs alone in a slot of its own size.

Worst |got - want| / bound per (form, stage) over both layers, as measured on an MI355X (fp16-resid16 = fp16: the same kernels, the same figures).  A
16-bit stage behind a product or a LayerNorm sits just under 1 by construction: the bound is little more than the half ulp of the stored value, and some of
a million elements land next to a rounding boundary.  ln_b_x / ln_c_x: the fp32 stream a post-LN LayerNorm writes back.  No stage of any form leaves its
bound; the walk's choices (LayerNorm order and write-back, eps, key bias, row tables, V^T pitch, kernel rule, weight offsets) are the callers'.
    stage    whisper-tiled    bert             bert-full-slot   w2v-post-ln      w2v-pre-ln
             fp16   bf16      fp16   bf16      fp16   bf16      fp16   bf16      fp16   bf16
    ln_a     0.996  0.996     -                -                -                0.993  0.996
    qk       0.948  0.980     0.972  0.991     0.987  0.994     0.986  0.987     0.975  0.992
    vt       0.962  0.991     0.979  0.982     0.976  0.993     0.976  0.994     0.943  0.979
    attn     0.077  0.400     0.175  0.500     0.134  0.544     0.171  0.514     0.171  0.412
    x1       0.270  0.269     0.354  0.553     0.340  0.562     0.345  0.535     0.351  0.246
    ln_b     0.996  0.996     0.994  0.995     0.995  0.996     0.991  0.996     0.995  0.996
    ln_b_x   -                0.185  0.204     0.219  0.194     0.164  0.172     -
    hidden   0.861  0.975     0.895  0.982     0.963  0.990     0.795  0.954     0.803  0.959
    x2       0.034  0.034     0.003  0.002     0.004  0.004     0.001  0.001     0.292  0.294
    ln_c     -                0.993  0.996     0.995  0.995     0.994  0.995     -
    ln_c_x   -                0.186  0.197     0.186  0.207     0.173  0.166     -"""
import numpy as np
import pytest

from prosody_control_french_tts_amd import PceError
from tests import encoder_walk_restatement as R

pytestmark = pytest.mark.gpu

SEED = 20                       # tests/test_encoder_walk_host.py proves the checks on the same inputs
RATIOS = {}


def _device(engine, form, W, x, ops, lens=None, rows=None):
    """one call -> (the capture arrays, whether every product was launched)"""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    st = R.empty_stages(form, len(W), lens, rows)
    ln_in = None if form["pre_ln"] else R.bits(x, ops)
    fit = engine.selftest_encoder_walk(form["pre_ln"], form["rule"], form["key_bias"], form["heads"], form["inner"], len(W), rows, form["vt_sp"], lens,
                                       form["eps"], R.blob(W, form), x, st, ln_in=ln_in)
    return st, ln_in, fit


def _valid(st, lens, rows, item=None):
    """the valid rows of every stage as exact bit patterns (one item's, or all)"""
    ok = R.valid_mask(lens, rows)
    if item is not None:
        ok &= np.arange(ok.size) // rows == item
    items = range(len(lens)) if item is None else [item]
    out = dict(ln16=st["ln16"][:, :, ok], qk=st["qk"][:, ok], attn=st["attn"][:, ok], hidden=st["hidden"][:, ok], x32=st["x32"][:, :, ok].view(np.uint32))
    for i in items:
        out[f"vt{i - (item or 0)}"] = st["vt"][:, i, :, :lens[i]]
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("form_name", sorted(R.FORMS))
def test_every_stage_against_float64(engine, ops, form_name):
    form = R.FORMS[form_name]
    lens, rows = form["lens"], form["rows"]
    W = R.draw_weights(form, 2, SEED)
    x = R.draw_stream(form, SEED)
    w2v = form["rule"] == 1
    if w2v:
        engine.profile_enable(True)
        engine.profile_reset()
    st, ln_in, fit = _device(engine, form, W, x, ops)
    if w2v:                         # QKV at N = 1536 and fc1 at N = 2048 on the 128 x 256 kernel, the out-projection and fc2 on the 128 x 128 one
        prof = engine.profile()
        engine.profile_enable(False)
        assert prof["k_gemm_wide"]["launches"] == 4 and prof["k_gemm_bf16"]["launches"] == 4, {k: v["launches"] for k, v in prof.items()}
    assert fit
    ratios = R.check_stages(form, W, x, ln_in, st, ops)
    for layer, stage, r in ratios:
        key = (form_name, stage, ops["name"])
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
        print(f"walk-ratio {form_name} {ops['name']} layer {layer} {stage}: {r:.4f}")
    assert [s for _, s, _ in ratios] == list(R.stage_names(form)) * 2
    bad = [(layer, stage, r) for layer, stage, r in ratios if not r <= 1.0]
    assert not bad, (form_name, ops["name"], bad)
    assert R.structure_failures(form, st, ops) == [], (form_name, ops["name"])
    # the pad rows' contents reach no valid row of any stage
    if not all(n == rows for n in lens):
        st0, _, _ = _device(engine, form, W, R.draw_stream(form, SEED, pad="zero"), ops)
        _same(_valid(st, lens, rows), _valid(st0, lens, rows), (form_name, ops["name"], "zero pad rows"))
    # nor do the other items or the slot size: one item alone in a slot of its own
    i = min(2, len(lens) - 1)
    alone = R.pad16(lens[i])
    x1 = np.zeros((alone, form["d"]), dtype=np.float32)
    x1[:lens[i]] = R.item_rows(form, SEED, i, lens[i])
    st1, _, fit1 = _device(engine, form, W, x1, ops, lens=(lens[i],), rows=alone)
    assert fit1
    _same(_valid(st, lens, rows, item=i), _valid(st1, (lens[i],), alone), (form_name, ops["name"], f"item {i} alone in {alone} rows"))


def test_whisper_key_projection_has_exactly_no_bias(engine, ops):
    """With a zero key matrix the K half of Q | K is the key bias alone: every bit zero in the Whisper form (the packer's zero vector), the rounded bias where the
    form has one."""
    for name in ("whisper-tiled", "w2v-pre-ln"):
        form = dict(R.FORMS[name], rows=16, lens=(16, 5))
        W = R.draw_weights(form, 1, SEED)
        W[0]["k_w"][:] = 0.0
        st, _, fit = _device(engine, form, W, R.draw_stream(form, SEED), ops)
        K = st["qk"][0][:, form["d"]:]
        want = np.zeros(form["d"], np.float32) if W[0]["k_b"] is None else W[0]["k_b"]
        assert fit and np.array_equal(K & 0x7FFF if W[0]["k_b"] is None else K, np.broadcast_to(R.bits(want, ops), K.shape)), (name, ops["name"])


def test_walk_selftest_refuses_what_the_loaders_refuse(engine):
    """PCE_E_LIMIT / PCE_E_INVALID before any launch: widths and inner sizes the loaders refuse, lengths outside the slot, a slot wider than the V^T image, a
    blob of another size, capture arrays one element short."""
    base = dict(R.FORMS["bert"], d=128, heads=2, inner=128, rows=16, vt_sp=64, lens=(16, 3))
    ops = dict(torch="float16")

    def call(short=None, blob_extra=0, **kw):
        form = dict(base, **kw)
        W = R.draw_weights(form, 1, 0)
        x = np.zeros((len(form["lens"]) * form["rows"], form["d"]), np.float32)
        st = R.empty_stages(form, 1)
        if short:
            st[short] = st[short].ravel()[:-1].copy()
        blob = np.concatenate([R.blob(W, form), np.zeros(blob_extra, np.float32)])
        return engine.selftest_encoder_walk(form["pre_ln"], form["rule"], form["key_bias"], form["heads"], form["inner"], 1, form["rows"], form["vt_sp"],
                                            form["lens"], form["eps"], blob, x, st, ln_in=R.bits(x, ops), d=form["d"])

    assert call()
    for bad in (dict(d=192, heads=3), dict(heads=3), dict(d=2176, heads=34), dict(inner=192)):
        with pytest.raises(PceError, match="status -5"):
            call(**bad)
    for bad in (dict(lens=(16, 0)), dict(lens=(17, 3)), dict(rows=80, lens=(16, 3)), dict(rows=18, lens=(16, 3)), dict(blob_extra=1), dict(short="ln16"),
                dict(short="qk"), dict(short="vt"), dict(short="attn"), dict(short="hidden"), dict(short="x32")):
        with pytest.raises(PceError, match="status -1"):
            call(**bad)
