"""Float64 restatement of one transformer encoder layer, stage by stage, for the checks of the shared layer walk (csrc/pce_encoder.inc: encoder_walk)
through pce_selftest_encoder_walk.  Written from the definitions of the three models' layers (BERT, wav2vec2 in its two forms, Whisper's audio encoder), not
from the walk; tests/test_encoder_walk_host.py pins its composition to transformers' own modules.  Nothing here touches the GPU.

    pre-LN  (Whisper, wav2vec2 stable_ln):  x1 = x + Wo MHA(LN1 x) + bo;        x2 = x1 + W2 gelu(W1 LN2 x1 + b1) + b2
    post-LN (BERT, wav2vec2):               x1 = x + Wo MHA(x) + bo, s = LN1 x1; x2 = s + W2 gelu(W1 s + b1) + b2, out = LN2 x2

MHA: heads of 64, softmax(q k^T / 8) v over the first len[i] keys of item i; gelu is the exact (erf) one.

One function per stage.  Each takes the stage's INPUT AS THE DEVICE LEFT IT (the buffer the previous launch wrote, converted exactly to float64) and returns
the float64 result with the per-element bound on what the stage's own fp32 / 16-bit arithmetic may add.  Chaining on the device's buffers keeps every
bound one kernel's: no error is carried through a 16-bit rounding.  No bound is derived here.  They are the single-kernel tests' own:

  * LayerNorm: ``_ln_ref`` (tests/gemm_restatement.py, derived in tests/test_gpu_kernels.py);
  * the products: ``gemm_acc`` / ``gemm_pre`` (K 2^-24 sum |a b|, one fp32 addition for the bias), ``resid_err`` for the fp32 accumulate epilogue and
    ``_gelu_err`` for the GELU one (same files);
  * the attention: ``_reference`` of tests/test_gpu_attention.py for k_attention_lean16 as the product launches it (mode 0: P rounded to the operand
    type, the fp16 flush), with its EPS_EXP as it stands;
  * a 16-bit output: ``bound16``, an fp32 one: ``bound32`` -- what ``_check16`` / ``_check32`` accept.

``check_stages`` walks the captured stages in launch order and returns |got - want| / bound per (layer, stage).  ``standin`` is the restatement itself
with every stage output rounded to the type the device stores (and one mutation at a time): what the CPU test proves the checks on."""
import numpy as np

from tests.gemm_restatement import U, _gelu_err, _ln_ref, bits, bound16, bound32, gelu64, gemm_acc, gemm_pre, resid_err, val  # noqa: F401
from tests.test_gpu_attention import BIG, _reference as _attention_reference
from tests import attention_restatement as AR

AT_SP = 1536                     # csrc/pce_gemm_tiled.inc: the key columns of the Whisper encoder's V^T image
SENTINEL16 = np.uint16(0x7FFF)   # a NaN in both 16-bit types: no finite result rounds to it
ATTN_SENTINEL = np.uint16(0x3555)  # finite in both types: the run's attention buffer starts with it, and the out-projection multiplies its pad rows


def pad16(n):
    return -(-n // 16) * 16


# the forms of the issue's table (rows = rows_per_item)
FORMS = {
    "whisper-tiled": dict(pre_ln=1, rule=0, key_bias=0, eps=1e-5, d=384, heads=6, inner=1536, rows=1500, vt_sp=AT_SP, lens=(1500, 1500)),
    "bert": dict(pre_ln=0, rule=0, key_bias=1, eps=1e-12, d=256, heads=4, inner=1024, rows=128, vt_sp=512, lens=(1, 16, 17, 37, 128)),
    "bert-full-slot": dict(pre_ln=0, rule=0, key_bias=1, eps=1e-12, d=128, heads=2, inner=512, rows=512, vt_sp=512, lens=(512, 300)),
    "w2v-post-ln": dict(pre_ln=0, rule=1, key_bias=1, eps=1e-5, d=512, heads=8, inner=2048, rows=pad16(149), vt_sp=192, lens=(1, 63, 64, 65, 149)),
    "w2v-pre-ln": dict(pre_ln=1, rule=1, key_bias=1, eps=1e-5, d=512, heads=8, inner=2048, rows=pad16(149), vt_sp=192, lens=(1, 63, 64, 65, 149)),
}


def whisper_order(form):
    """pack_encoder_layer's ln_first: the Whisper loader's (the pre-LN stack on the product's GEMM rule); every other loader reads transformers' order"""
    return bool(form["pre_ln"]) and form["rule"] == 0


# ---------------------------------------------------------------------------------------------------------------
# weights and inputs
# ---------------------------------------------------------------------------------------------------------------
def draw_weights(form, n_layers, seed):
    """n_layers dicts of fp32 tensors in PyTorch layouts, different per layer.  The Q / K / V matrices are small (0.15 / sqrt d) so that a +-60000 pad row of
    a post-LN stream stays finite in fp16 behind the projection (6.7 sigma below 65504).  The query bias is of the size of the projected rows (0.3), so that
    the sign of a query's score against the mean-1000 row, whose key is a thousand times an ordinary one, changes from query to query: in every (item,
    head) that key takes all the weight of about half the queries, and a mask one key short (it is the item's last) cannot go unseen.  A small output
    projection keeps var(x1) near 0.03 on the 1e-4 rows of a post-LN form: there eps = 1e-5 moves the LayerNorm by 1.7e-4 relative, 100 times what the
    fp32 stream check allows."""
    rng = np.random.default_rng([seed, form["d"], form["inner"]])
    d, I = form["d"], form["inner"]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    layers = []
    for _ in range(n_layers):
        W = {}
        for n in "qkv":
            W[n + "_w"] = f(rng.standard_normal((d, d)) * 0.15 / np.sqrt(d))
        W["q_b"], W["v_b"] = f(0.3 * rng.standard_normal(d)), f(0.5 * rng.standard_normal(d))
        W["k_b"] = f(rng.standard_normal(d)) if form["key_bias"] else None
        W["out_w"], W["out_b"] = f(rng.standard_normal((d, d)) * 0.3 / np.sqrt(d)), f(0.1 * rng.standard_normal(d))
        W["fc1_w"], W["fc1_b"] = f(rng.standard_normal((I, d)) / np.sqrt(d)), f(rng.standard_normal(I))
        W["fc2_w"], W["fc2_b"] = f(rng.standard_normal((d, I)) / np.sqrt(I)), f(0.1 * rng.standard_normal(d))
        for n in ("ln1", "ln2"):
            W[n + "_w"], W[n + "_b"] = f(1.0 + 0.1 * rng.standard_normal(d)), f(0.1 * rng.standard_normal(d))
        layers.append(W)
    return layers


def blob(layers, form):
    """the layers' tensors in the order the form's loader reads them (include/pce.h: pce_selftest_encoder_walk)"""
    out = []
    for W in layers:
        att = [W["q_w"], W["q_b"], W["k_w"]] + ([W["k_b"]] if form["key_bias"] else []) + [W["v_w"], W["v_b"], W["out_w"], W["out_b"]]
        mlp = [W["fc1_w"], W["fc1_b"], W["fc2_w"], W["fc2_b"]]
        ln1, ln2 = [W["ln1_w"], W["ln1_b"]], [W["ln2_w"], W["ln2_b"]]
        out += (ln1 + att + ln2 + mlp) if whisper_order(form) else (att + ln1 + mlp + ln2)
    return np.concatenate([t.ravel() for t in out]).astype(np.float32)


def big_pattern(shape):
    """+-60000 in the fixed pattern of tests/test_gpu_attention.py's _big, as float32"""
    n = int(np.prod(shape))
    return np.where((np.arange(n) * 7 // 3) % 2 == 0, BIG, -BIG).reshape(shape).astype(np.float32)


def valid_mask(lens, rows):
    return (np.arange(rows)[None, :] < np.asarray(lens)[:, None]).ravel()


def draw_stream(form, seed, lens=None, rows=None, pad="big"):
    """The fp32 stream [items x rows][d]: seeded normal rows; in every item two rows of 1e-4 randn (the first and the middle one: where eps decides the
    LayerNorm) and, from three rows on, a last row of mean 1000 and unit spread; pad rows +-60000 (or zeros).  The valid rows of item i do not depend on
    what the other items or the slot size are."""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    d = form["d"]
    x = big_pattern((len(lens), rows, d)) if pad == "big" else np.zeros((len(lens), rows, d), dtype=np.float32)
    for i, n in enumerate(lens):
        x[i, :n] = item_rows(form, seed, i, n)
    return x.reshape(-1, d)


def item_rows(form, seed, i, n):
    rng = np.random.default_rng([seed, 77, i, n])
    v = rng.standard_normal((n, form["d"]))
    tiny = 1e-4 * rng.standard_normal((2, form["d"]))
    v[0] = tiny[0]
    if n >= 2:
        v[n // 2] = tiny[1]
    if n >= 3:
        v[n - 1] = 1000.0 + rng.standard_normal(form["d"])
    return v.astype(np.float32)


def empty_stages(form, n_layers, lens=None, rows=None):
    """the capture arrays of pce_selftest_encoder_walk filled with sentinels (the attention's a finite one: include/pce.h)"""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    M, d, L = len(lens) * rows, form["d"], n_layers
    s16 = lambda *shape: np.full(shape, SENTINEL16, dtype=np.uint16)
    return dict(ln16=s16(L, 3, M, d), qk=s16(L, M, 2 * d), vt=s16(L, len(lens), d, form["vt_sp"]), attn=np.full((L, M, d), ATTN_SENTINEL, dtype=np.uint16),
                hidden=s16(L, M, form["inner"]), x32=np.full((L, 4, M, d), np.nan, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------
# the stages: float64 values in, (float64 result, per-element bound of the stage's own arithmetic) out
# ---------------------------------------------------------------------------------------------------------------
def ln_stage(x, w, b, eps):
    """LayerNorm of the stream rows x (the values the kernel normalised)"""
    return _ln_ref(np.asarray(x), np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64), eps)


def qkv_stage(a, wq, wk, wv, bq, bk, bv):
    """[q | k | v] = a [Wq; Wk; Wv]^T + [bq | bk or 0 | bv]: a [M][d] the LayerNorm image, the matrices as the operand type holds them"""
    bias = np.concatenate([bq, np.zeros_like(bq) if bk is None else bk, bv]).astype(np.float64)
    acc, _, acc_err = gemm_acc(a, np.concatenate([wq, wk, wv]))
    return gemm_pre(acc, acc_err, bias)


def vt_image(v, n_items, rows, vt_sp):
    """V [items x rows][d] -> the image [item][d][vt_sp] the attention reads: column t of item i is row i x rows + t, the columns from `rows` on are zero"""
    d = v.shape[1]
    img = np.zeros((n_items, d, vt_sp), dtype=v.dtype)
    img[:, :, :rows] = v.reshape(n_items, rows, d).transpose(0, 2, 1)
    return img


def attention_stage(q, k, vt, lens, rows, heads, ops, key_lens=None):
    """q, k [items x rows][d], vt [items][d][vt_sp] -> (want, err) [items x rows][d] on the rows below len[i] (NaN elsewhere: no launch writes them);
    query rows and keys of item i: its first len[i] rows (key_lens: another key count, for the mutations)"""
    want = np.full(q.shape, np.nan)
    err = np.full(q.shape, np.nan)
    flush = ops["torch"] == "float16"              # launch_attention_rows runs mode 0
    for i, n in enumerate(lens):
        nk = n if key_lens is None else key_lens[i]
        r0 = i * rows
        kk, vv = k[r0:r0 + nk], vt[i, :, :nk].T
        for h in range(heads):                       # (one head at a time: the 1500 x 1500 weights of six heads at once are a gigabyte of temporaries)
            c = slice(64 * h, 64 * h + 64)
            w, e = _attention_reference(q[None, r0:r0 + n, c], kk[None, :, c], vv[None, :, c], "lean", ops, p_rounded=True, flush=flush)
            want[r0:r0 + n, c], err[r0:r0 + n, c] = w[0], e[0]
    return want, err


def resid_stage(a, w, bias, old):
    """old + a w^T + bias in fp32 (the out-projection and fc2): a the 16-bit operand's values, old the fp32 stream before the launch"""
    acc, _, acc_err = gemm_acc(a, w)
    pre, err = gemm_pre(acc, acc_err, bias)
    o = np.asarray(old, dtype=np.float64)
    return o + pre, resid_err(o, acc, err)


def gelu_stage(a, w, bias, gelu=gelu64):
    """gelu(a w^T + bias) (fc1)"""
    acc, _, acc_err = gemm_acc(a, w)
    pre, err = gemm_pre(acc, acc_err, bias)
    return gelu(pre), _gelu_err(pre, err)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


# ---------------------------------------------------------------------------------------------------------------
# the layer in float64 without any rounding (what tests/test_encoder_walk_host.py pins to transformers)
# ---------------------------------------------------------------------------------------------------------------
def layer_float64(form, W, x, lens, rows):
    """one layer on the float64 stream x [items x rows][d] -> the stream behind it (valid rows; pad rows carry whatever the arithmetic gives)"""
    f = lambda t: None if t is None else t.astype(np.float64)
    d, H, eps = form["d"], form["heads"], form["eps"]
    ops = dict(torch="float16")                                     # (only the bounds look at it; they are dropped here)
    a = ln_stage(x, W["ln1_w"], W["ln1_b"], eps)[0] if form["pre_ln"] else x
    qkv = qkv_stage(a, f(W["q_w"]), f(W["k_w"]), f(W["v_w"]), W["q_b"], W["k_b"], W["v_b"])[0]
    att = attention_stage(qkv[:, :d], qkv[:, d:2 * d], vt_image(qkv[:, 2 * d:], len(lens), rows, rows), lens, rows, H, ops)[0]
    att = np.where(np.isnan(att), 0.0, att)
    x1 = resid_stage(att, f(W["out_w"]), W["out_b"], x)[0]
    if form["pre_ln"]:
        s = x1
        a2 = ln_stage(x1, W["ln2_w"], W["ln2_b"], eps)[0]
    else:
        s = a2 = ln_stage(x1, W["ln1_w"], W["ln1_b"], eps)[0]
    hid = gelu_stage(a2, f(W["fc1_w"]), W["fc1_b"])[0]
    x2 = resid_stage(hid, f(W["fc2_w"]), W["fc2_b"], s)[0]
    return x2 if form["pre_ln"] else ln_stage(x2, W["ln2_w"], W["ln2_b"], eps)[0]


# ---------------------------------------------------------------------------------------------------------------
# the captured stages against the restatement, in launch order
# ---------------------------------------------------------------------------------------------------------------
STAGES_PRE = ("ln_a", "qk", "vt", "attn", "x1", "ln_b", "hidden", "x2")
STAGES_POST = ("qk", "vt", "attn", "x1", "ln_b", "ln_b_x", "hidden", "x2", "ln_c", "ln_c_x")


def stage_names(form):
    return STAGES_PRE if form["pre_ln"] else STAGES_POST


def _ratio16(got_bits, want, err, ops):
    """|got - want| / bound per element; infinite where the device left something that is not finite"""
    got = val(got_bits, ops)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(got), np.abs(got - want) / bound16(want, err, ops), np.inf)


def _ratio32(got, want, err):
    got = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(got), np.abs(got - want) / bound32(want, err), np.inf)


def check_stages(form, layers, x, ln_in, st, ops, lens=None, rows=None):
    """Every element of every captured stage against the restatement of that stage on the buffer the device left in front of it.
    -> [(layer, stage, worst |got - want| / bound)] in launch order.  x: the stream on entry, ln_in: the post-LN forms' opening image."""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    d, H, eps, pre = form["d"], form["heads"], form["eps"], bool(form["pre_ln"])
    n = len(lens)
    ok = valid_mask(lens, rows)
    w16 = lambda t: val(bits(t, ops), ops)                         # a matrix as upload_weights leaves it
    out = []
    stream, image = x, ln_in                                        # what the layer finds: the fp32 stream, and (post-LN) its 16-bit image
    for l, W in enumerate(layers):
        add = lambda name, r: out.append((l, name, float(np.max(r))))
        if pre:
            y, e = ln_stage(stream, W["ln1_w"], W["ln1_b"], eps)
            add("ln_a", _ratio16(st["ln16"][l, 0], y, e, ops))
            image = st["ln16"][l, 0]
        p, e = qkv_stage(val(image, ops), w16(W["q_w"]), w16(W["k_w"]), w16(W["v_w"]), W["q_b"], W["k_b"], W["v_b"])
        add("qk", _ratio16(st["qk"][l], p[:, :2 * d], e[:, :2 * d], ops))
        add("vt", _ratio16(st["vt"][l][:, :, :rows], vt_image(p[:, 2 * d:], n, rows, rows), vt_image(e[:, 2 * d:], n, rows, rows), ops))
        qk = val(st["qk"][l], ops)
        y, e = attention_stage(qk[:, :d], qk[:, d:], val(st["vt"][l], ops), lens, rows, H, ops)
        add("attn", _ratio16(st["attn"][l][ok], y[ok], e[ok], ops))
        y, e = resid_stage(val(st["attn"][l], ops), w16(W["out_w"]), W["out_b"], stream)
        add("x1", _ratio32(st["x32"][l, 0], y, e))
        x1 = st["x32"][l, 0]
        y, e = ln_stage(x1, W["ln2_w" if pre else "ln1_w"], W["ln2_b" if pre else "ln1_b"], eps)
        add("ln_b", _ratio16(st["ln16"][l, 1], y, e, ops))
        if not pre:
            add("ln_b_x", _ratio32(st["x32"][l, 1], y, e))
        mid = x1 if pre else st["x32"][l, 1]
        y, e = gelu_stage(val(st["ln16"][l, 1], ops), w16(W["fc1_w"]), W["fc1_b"])
        add("hidden", _ratio16(st["hidden"][l], y, e, ops))
        y, e = resid_stage(val(st["hidden"][l], ops), w16(W["fc2_w"]), W["fc2_b"], mid)
        add("x2", _ratio32(st["x32"][l, 2], y, e))
        stream = st["x32"][l, 2]
        if not pre:
            y, e = ln_stage(stream, W["ln2_w"], W["ln2_b"], eps)
            add("ln_c", _ratio16(st["ln16"][l, 2], y, e, ops))
            add("ln_c_x", _ratio32(st["x32"][l, 3], y, e))
            stream, image = st["x32"][l, 3], st["ln16"][l, 2]
    return out


def structure_failures(form, st, ops, lens=None, rows=None):
    """The exact properties beside the bounds -> the names of those that do not hold: attention rows at and behind len[i] keep the sentinel; V^T columns at
    and behind rows_per_item keep their zeros; in the post-LN forms the 16-bit image is the written-back fp32 stream rounded once, bit for bit; the
    slots no launch of the form writes keep their sentinels."""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    ok = valid_mask(lens, rows)
    bad = []
    for l in range(st["qk"].shape[0]):
        if not (st["attn"][l][~ok] == ATTN_SENTINEL).all():
            bad.append((l, "attention pad rows"))
        if not (st["vt"][l][:, :, rows:] == 0).all():
            bad.append((l, "V^T pad columns"))
        if form["pre_ln"]:
            if not ((st["ln16"][l, 2] == SENTINEL16).all() and np.isnan(st["x32"][l, 1]).all() and np.isnan(st["x32"][l, 3]).all()):
                bad.append((l, "unwritten slots"))
        else:
            if not (st["ln16"][l, 0] == SENTINEL16).all():
                bad.append((l, "unwritten slots"))
            for slot16, slot32, name in ((1, 1, "ln_b"), (2, 3, "ln_c")):
                if not np.array_equal(bits(st["x32"][l, slot32], ops), st["ln16"][l, slot16]):
                    bad.append((l, name + " image is not the stream rounded once"))
    return bad


# ---------------------------------------------------------------------------------------------------------------
# the stand-in for the device: the restatement with every stage output rounded to the type the device stores, and one mutation at a time
# ---------------------------------------------------------------------------------------------------------------
MUTATIONS = ("eps", "key_bias", "mask_long", "mask_short", "ln_before_add", "tanh_gelu", "layer1_weights", "vt_pitch", "ln_not_written_back")


def standin(form, layers, x, ln_in, ops, mut=None, lens=None, rows=None):
    """-> the capture arrays as a faultless device would return them (mut: one of MUTATIONS applied to every layer it can apply to)"""
    lens = form["lens"] if lens is None else lens
    rows = form["rows"] if rows is None else rows
    d, H, pre, vt_sp = form["d"], form["heads"], bool(form["pre_ln"]), form["vt_sp"]
    n = len(lens)
    eps = 1e-5 if mut == "eps" else form["eps"]
    ok = valid_mask(lens, rows)
    st = empty_stages(form, len(layers), lens, rows)
    w16 = lambda t: val(bits(t, ops), ops)
    f32 = lambda t: t.astype(np.float32)
    stream, image = x.copy(), ln_in
    attn_buf = np.full((n * rows, d), ATTN_SENTINEL, dtype=np.uint16)       # the run's buffer: rows no launch writes keep what they held
    for l, W0 in enumerate(layers):
        W = layers[0] if mut == "layer1_weights" else W0
        if pre:
            image = st["ln16"][l, 0] = bits(ln_stage(stream, W["ln1_w"], W["ln1_b"], eps)[0], ops)
        kb = W["k_b"]
        if mut == "key_bias" and kb is None:
            kb = np.random.default_rng(5).standard_normal(d).astype(np.float32)
        p = f32(qkv_stage(val(image, ops), w16(W["q_w"]), w16(W["k_w"]), w16(W["v_w"]), W["q_b"], kb, W["v_b"])[0])
        st["qk"][l] = bits(p[:, :2 * d], ops)
        vbits = bits(p[:, 2 * d:], ops)
        if mut == "vt_pitch":                                       # item i's image starts i x d x rows elements in, its columns rows apart
            flat = np.zeros(n * d * vt_sp, dtype=np.uint16)
            flat[:n * d * rows] = vt_image(vbits, n, rows, rows).ravel()
            st["vt"][l] = flat.reshape(n, d, vt_sp)
        else:
            st["vt"][l] = vt_image(vbits, n, rows, vt_sp)
        key_lens = None
        if mut in ("mask_long", "mask_short"):
            key_lens = [min(k + 1, rows) if mut == "mask_long" else max(k - 1, 1) for k in lens]
        qk = val(st["qk"][l], ops)
        a = attention_stage(qk[:, :d], qk[:, d:], val(st["vt"][l], ops), lens, rows, H, ops, key_lens)[0]
        attn_buf[ok] = bits(a[ok], ops)
        st["attn"][l] = attn_buf
        x1 = st["x32"][l, 0] = f32(resid_stage(val(attn_buf, ops), w16(W["out_w"]), W["out_b"], stream)[0])
        lw, lb = (W["ln2_w"], W["ln2_b"]) if pre else (W["ln1_w"], W["ln1_b"])
        if mut == "ln_before_add" and not pre:                      # s = x + LN(branch) in place of LN(x + branch)
            y = f32(stream.astype(np.float64) + ln_stage(x1.astype(np.float64) - stream, lw, lb, eps)[0])
        else:
            y = f32(ln_stage(x1, lw, lb, eps)[0])
        st["ln16"][l, 1] = bits(y, ops)
        if pre:
            mid = x1
        else:
            mid = st["x32"][l, 1] = x1 if mut == "ln_not_written_back" else y
        hid = st["hidden"][l] = bits(gelu_stage(val(st["ln16"][l, 1], ops), w16(W["fc1_w"]), W["fc1_b"], gelu_tanh if mut == "tanh_gelu" else gelu64)[0], ops)
        stream = st["x32"][l, 2] = f32(resid_stage(val(hid, ops), w16(W["fc2_w"]), W["fc2_b"], mid)[0])
        if not pre:
            y = f32(ln_stage(stream, W["ln2_w"], W["ln2_b"], eps)[0])
            image = st["ln16"][l, 2] = bits(y, ops)
            st["x32"][l, 3] = stream if mut == "ln_not_written_back" else y
            stream = st["x32"][l, 3]
    return st
