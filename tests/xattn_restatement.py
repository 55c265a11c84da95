"""Float64 restatement, stage by stage, of the encoder-output cross-attention of an incremental decoding step (csrc/pce_xattn.inc:
k_xq_fused -> k_xattn_absorbed -> k_uv_absorb), the error each kernel's fp32 / 16-bit arithmetic allows per element, the operand classes the tests
run, and a float32 / 16-bit numpy emulation of the kernels' arithmetic with switchable defects (for tests/test_xattn_host.py: the bounds must hold
for the faithful arithmetic and must NOT hold for the defects).  numpy only; nothing here touches the GPU.

Every stage is restated FROM THE PREVIOUS STAGE'S OUTPUT AS THE DEVICE RETURNED IT (pce_selftest_xattn_stages), so an error is pinned to the kernel that made
it.  With u16 the half-ulp of the operand type (2^-11 fp16, 2^-8 bf16), U = 2^-24 (fp32) and EPS_EXP2 the relative error of the hardware 2^x:

stage 1 (k_xq_fused)   ln = r16(LayerNorm(resid)), q = r16(Wq ln + bq), Q'_h = scale (q_h Wk_h), scale = fp32(0.125f * log2 e), out as hi + lo.
  * LayerNorm: the bound of tests/test_gpu_kernels.py::_ln_ref (k_layernorm's arithmetic, operation for operation).  Rounding is monotonic, so the device's
    ln lies between r16(y - e) and r16(y + e): the distance of those from r16(y) -- zero for most elements, one 16-bit step for a few -- is carried on;
  * q: d / 4 products on a wave's MFMA chain + 3 additions through LDS + the bias: (d / 4 + 4) U (sum |Wq ln| + |bq|), plus |Wq| times ln's distance;
    then the same interval argument for the rounding of q;
  * Q': 64 products on the chain + the multiplication by scale: 65 U scale sum |q Wk|, plus scale |Wk| times q's distance;
  * the split v -> hi = r16(v), lo = r16(v - hi): hi + lo = v to u16^2 |v| (2^-22 fp16, 2^-16 bf16: from the formats, lo is at most half a step of hi
    and is rounded to the same number of bits) or, fp16, to half its subnormal step 2^-25 where lo falls below 2^-14.

stage 2 (k_xattn_absorbed)   per (clip, head, node), from Q' = hi + lo as returned and the node's reference m as returned (a node's (m, l, U) is defined
  only up to that choice): s_t = Q' . E[t], l = sum_t 2^(s_t - m), U = sum_t 2^(s_t - m) E[t] over the node's frames t < k_len.
  * a score: wave w sums d / WV products for hi and as many for lo on its MFMA chain, then WV partials are added through LDS:
    delta_t = (2 d / WV + WV) U sum_e |Q'_e E_te| (WV = 4 waves, 8 at d = 1280).  m must be the largest score to delta; a weight moves by
    p (e^(2 delta ln 2) - 1), delta the largest of the node, as tests/test_gpu_attention.py takes it;
  * the exponent s_t - m reaches the weight through one subtraction per tile that rescales: the differences telescope, U |s_t - m| in all;
  * one 2^x per weight and one per rescale, and a rescale multiplies: (1 + EPS_EXP2)^(1 + r) (1 + U)^r, r = tiles of the node - 1 (+ 1 for a pair node,
    whose two leaves are merged by one more 2^x and one fma);
  * l: 4 additions per tile on a lane + 2 shuffle levels (+ 2 for the pair merge): (4 tiles + 4) U l;
  * P enters its MFMA as hi + lo: u16^2 p, or (fp16) 2^-25 where a part is subnormal; 16 + 16 products per tile on the chain: 32 tiles U sum p |E|;
  * what 2^x returns below 2^-126 is left open: 2^-126 per weight.

stage 3 (k_uv_absorb)   from u_part / ml_part as returned: the tree (L0 + L1) + (L2 + L3), U / l, out = Wv_h U_h + bv.
  * a node's weight is at most two 2^x of an fp32 difference: 2 EPS_EXP2 + U |m_s - m| ln 2; its products and fmas: 5 roundings for U, 4 for l, the
    reciprocal within 2 ulp (4 U);
  * U is split as in stage 1; a wave sums d / 4 products for hi and d / 4 for lo, 3 additions through LDS and the bias:
    (d / 2 + 4) U (sum |Wv U| + |bv|);
  * one rounding of the 16-bit output: err + u16 (|want| + err) + 2^-24, as tests/test_gpu_attention.py::_check.

Nothing is fitted.  EPS_EXP2 is the one constant the code does not give: measured on the MI355X by tests/test_gpu_xattn.py::probe_exp2_error."""
import numpy as np

U = 2.0 ** -24
SCALE = float(np.float32(0.125) * np.float32(1.4426950408889634))      # what xattn_launch_d hands k_xq_fused
EXACT_SCALE = float(np.log2(np.e)) / 8.0
M_EMPTY = float(np.float32(-1e30))                                     # the reference of a node without frames, as fp32 holds it
TF, LEAVES = 16, 4
BIG = 60000.0                                                          # finite in both 16-bit types: what must never be read
WIDTHS = (128, 256, 384, 512, 768, 1024, 1280)
K_LENS = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 97, 129, 144, 145, 160)
SUBSET = (1, 16, 17, 33, 49, 65, 81, 97, 129, 145, 160)               # one length per leaf pattern (tiles 1, 1, 2, 3, 4, 5, 6, 7, 9, 10, 10)
FULL_WIDTHS = (128, 768, 1280)                                         # the widths that take all of K_LENS; the others take SUBSET
PEAK_LENS = (160,) * 5 + (97,) * 4 + (17, 1)                           # the peak at the first frame of every leaf and on the last valid frame
PEAK_AT = (0, 48, 96, 144, 159, 0, 32, 64, 96, 16, 0)
MONOTONE_LENS = (160, 145, 97, 33, 16)
# EPS_EXP2_MEASURED: worst |device 2^x / float64 2^x - 1| of __builtin_amdgcn_exp2f seen by tests/test_gpu_xattn.py::probe_exp2_error on an MI355X
# (2026-10-20): 5.84e-8 over 1773 arguments (531 distinct) in [-125.51, -0.36], quartiles -30.3 / -9.9 / -3.2, each the fp32 number -k Q' with k in
# {0.5, 1, 2, 4} and Q' = fp32(scale q) for 480 seven-bit q between 4 and 508.  The bounds use 4 x it, the margin the project gave EPS_EXP, because the
# probe does not see every argument.
EPS_EXP2_MEASURED = 5.84e-8
EPS_EXP2 = 4 * EPS_EXP2_MEASURED


# ---------------------------------------------------------------------------------------------------------------
# the two 16-bit formats
# ---------------------------------------------------------------------------------------------------------------
def half_ulp(fmt):
    return 2.0 ** -8 if fmt == "bf16" else 2.0 ** -11


def split_rel(fmt):
    """hi + lo against the value, relative: lo <= u16 |v| is rounded to u16 of itself"""
    return half_ulp(fmt) ** 2


def split_floor(fmt):
    """... and absolute, where a part is subnormal: half the smallest step of the type"""
    return 2.0 ** -25 if fmt == "fp16" else 2.0 ** -134


def r16(x, fmt):
    """float64 (or float32) -> the value of the 16-bit type nearest to it (ties to even, ONE rounding), as float64"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        if fmt == "fp16":
            return x.astype(np.float16).astype(np.float64)
        e = np.frexp(x)[1] - 1
        q = np.ldexp(1.0, np.maximum(e, -126) - 7)
        v = np.round(x / q) * q                                     # np.round: half to even; x / q exact
        return np.where(np.abs(v) > (2.0 - 2.0 ** -7) * 2.0 ** 127, np.copysign(np.inf, x), v)


def to_bits(v, fmt):
    """values ON the type's grid -> uint16 bit patterns"""
    if fmt == "fp16":
        return np.asarray(v).astype(np.float16).view(np.uint16)
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b, fmt):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if fmt == "fp16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split(v, fmt):
    """fp32 value -> (hi, lo) as the kernels form them: hi = (op_t)v, lo = (op_t)(v - (float)hi)"""
    v = np.asarray(v, dtype=np.float32)
    hi = r16(v, fmt).astype(np.float32)
    with np.errstate(invalid="ignore"):
        lo = r16(v - hi, fmt).astype(np.float32)
    return hi, lo


def flip(y, e, fmt):
    """how far r16 of something within e of y can lie from r16(y) (rounding is monotonic)"""
    c = r16(y, fmt)
    return np.maximum(np.abs(r16(y + e, fmt) - c), np.abs(c - r16(y - e, fmt)))


# ---------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------
def xa_rows(heads):
    return 16 * ((heads + 15) // 16)


def waves(d):
    return 8 if d > 1024 else 4


def nodes_of(d, wpc):
    """what the launch writes: the two pair nodes where the width has the pair form (d <= 768) and a workgroup owns both leaves of a pair"""
    return 2 if d <= 768 and wpc in (1, 2) else 4                   # (0: what the batch size selects -- 4 below 256 clips)


def leaf_tiles(k_len):
    """the four leaves of a clip as (first tile, end tile) of its ceil(k_len / 16) 16-frame tiles"""
    nt_all = -(-k_len // TF)
    per = -(-nt_all // LEAVES)
    return [(min(i * per, nt_all), min((i + 1) * per, nt_all)) for i in range(LEAVES)]


def node_frames(k_len, nodes):
    """per node: (first frame, end frame, tiles); a pair node spans its two leaves"""
    lt = leaf_tiles(k_len)
    if nodes == 2:
        lt = [(lt[0][0], lt[1][1]), (lt[2][0], lt[3][1])]
    return [(a * TF, min(b * TF, k_len), b - a) for a, b in lt]


# ---------------------------------------------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------------------------------------------
def layernorm(x, w, b, eps=1e-5):
    """two-pass LayerNorm in float64 and the error of the fp32 kernel (tests/test_gpu_kernels.py::_ln_ref)"""
    v = np.asarray(x, dtype=np.float64)
    w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = v.shape[1]
    terms = 4 * -(-d // 256) + 6
    m = v.mean(axis=1, keepdims=True)
    xc = v - m
    q = (xc ** 2).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(q / d + eps)
    y = xc * inv * w + b
    dm = terms * U * np.abs(v).sum(axis=1, keepdims=True) / d + U * np.abs(m)
    rel_inv = 0.5 * ((terms + 3) * U + d * dm ** 2 / (q + d * eps)) + 3 * U
    err = np.abs(w) * inv * (np.abs(xc) * (rel_inv + 3 * U) + dm) + 2 * U * (np.abs(y) + np.abs(b))
    return y, err


def query(case, fmt):
    """-> (ln, q, q_pre, q_pre_err, q_flip): the rounded LayerNorm and query in float64, the unrounded query with its error, and how far the device's
    rounded q may lie from q"""
    d = case["d"]
    y, y_err = layernorm(case["resid"], case["ln_w"], case["ln_b"])
    ln, ln_flip = r16(y, fmt), flip(y, y_err, fmt)
    wq, bq = case["wq"], np.asarray(case["bq"], dtype=np.float64)
    q_pre = ln @ wq.T + bq
    q_err = ln_flip @ np.abs(wq).T + (d // 4 + 4) * U * (np.abs(ln) @ np.abs(wq).T + np.abs(bq))
    return ln, r16(q_pre, fmt), q_pre, q_err, flip(q_pre, q_err, fmt)


def qprime(q, q_flip, wk, heads, fmt, scale=SCALE):
    """Q' [n][heads][d] from the rounded query (float64) and its error, the split included"""
    n, d = q.shape
    qh = q.reshape(n, heads, 64)
    wkh = wk.reshape(heads, 64, d)
    want = scale * np.einsum("nhk,hkj->nhj", qh, wkh)
    mag = scale * np.einsum("nhk,hkj->nhj", np.abs(qh), np.abs(wkh))
    err = scale * np.einsum("nhk,hkj->nhj", q_flip.reshape(n, heads, 64), np.abs(wkh)) + 65 * U * mag
    return want, err + np.maximum(split_rel(fmt) * (np.abs(want) + err), split_floor(fmt))


def stage1(case, fmt, scale=SCALE):
    """scale: the kernel's fp32 constant; EXACT_SCALE where the chain is compared with the plain formula"""
    ln, q, q_pre, q_err, q_flip = query(case, fmt)
    want, err = qprime(q, q_flip, case["wk"], case["heads"], fmt, scale)
    return dict(ln=ln, q=q, q_pre=q_pre, q_err=q_err, q_flip=q_flip, qp=want, qp_err=err)


# ---------------------------------------------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------------------------------------------
def stage2(qp, E, k_len, m_ref, nodes, fmt, eps2=EPS_EXP2):
    """One clip.  qp [heads][d] (hi + lo), E [>= k_len][d], m_ref [nodes][heads]: the reference of every node (None: the largest score, what exact
    arithmetic would choose).  -> dict of [nodes][heads] (m, m_err, l, l_err) and [nodes][heads][d] (U, U_err)."""
    heads, d = qp.shape
    Ev = E[:k_len]
    S = qp @ Ev.T                                                  # [heads][frames]
    delta_t = (2 * d // waves(d) + waves(d)) * U * (np.abs(qp) @ np.abs(Ev).T)
    out = {k: np.zeros((nodes, heads)) for k in ("m", "m_err", "l", "l_err")}
    out["U"], out["U_err"] = np.zeros((nodes, heads, d)), np.zeros((nodes, heads, d))
    out["m"][:] = M_EMPTY
    for s, (f0, f1, tiles) in enumerate(node_frames(k_len, nodes)):
        if f1 <= f0:
            continue                                               # an empty node is exactly m = -1e30, l = 0, U = 0
        sc, e = S[:, f0:f1], Ev[f0:f1]
        delta = delta_t[:, f0:f1].max(axis=1, keepdims=True)
        m_true = sc.max(axis=1, keepdims=True)
        m = m_true if m_ref is None else np.asarray(m_ref[s], dtype=np.float64)[:, None]
        r = tiles - 1 + (1 if nodes == 2 else 0)
        with np.errstate(over="ignore"):
            p = np.exp2(sc - m)
            rel = np.exp((2 * delta + U * np.abs(sc - m)) * np.log(2.0)) * (1 + eps2) ** (1 + r) * (1 + U) ** r - 1
        dp = p * rel + 2.0 ** -126
        pe = dp + np.maximum(split_rel(fmt) * p, split_floor(fmt))
        l, A = p.sum(axis=1), p @ np.abs(e)
        out["m"][s], out["m_err"][s] = m_true[:, 0], delta[:, 0]
        out["l"][s], out["l_err"][s] = l, dp.sum(axis=1) + (4 * tiles + 4) * U * l
        out["U"][s], out["U_err"][s] = p @ e, pe @ np.abs(e) + (32 * tiles + 2) * U * A
    return out


# ---------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------
def tree(m, flat=False):
    """the weights of the nodes at the root of (L0 + L1) + (L2 + L3) (or of the two pairs), exactly: m [nodes][heads] -> (w [nodes][heads], the
    largest |difference| a weight's 2^x saw)"""
    m = np.asarray(m, dtype=np.float64)
    top = m.max(axis=0)
    with np.errstate(under="ignore"):
        return np.exp2(m - top), np.abs(m - top)


def stage3(u_part, ml_part, wv, bv, fmt, eps2=EPS_EXP2):
    """One clip.  u_part [nodes][heads][d], ml_part [nodes][heads][2], wv [d][d], bv [d] -> (want [d], err [d] before the output's rounding, U [heads][d])"""
    u_part, ml_part = np.asarray(u_part, dtype=np.float64), np.asarray(ml_part, dtype=np.float64)
    nodes, heads, d = u_part.shape
    w, diff = tree(ml_part[..., 0])                               # exact arithmetic: the tree's weights multiply out to 2^(m_s - m_root)
    rel = 2 * eps2 + U * diff * np.log(2.0) * 2
    lw = ml_part[..., 1] * w
    l = lw.sum(axis=0)
    num = (u_part * w[..., None]).sum(axis=0)
    v = num / l[:, None]
    num_err = (np.abs(u_part) * (w * (rel + 5 * U))[..., None]).sum(axis=0)
    l_err = (lw * (rel + 4 * U)).sum(axis=0) + 4 * U * l
    v_err = num_err / l[:, None] + np.abs(v) * (l_err / l)[:, None] + U * np.abs(v)
    v_err = v_err + np.maximum(split_rel(fmt) * (np.abs(v) + v_err), split_floor(fmt))
    wvh = wv.reshape(heads, 64, d)
    bv = np.asarray(bv, dtype=np.float64)
    want = np.einsum("hij,hj->hi", wvh, v).reshape(d) + bv
    mag = np.einsum("hij,hj->hi", np.abs(wvh), np.abs(v)).reshape(d)
    err = np.einsum("hij,hj->hi", np.abs(wvh), v_err).reshape(d) + (d // 2 + 4) * U * (mag + np.abs(bv))
    return want, err, v


def out_bound(want, err, fmt):
    """one rounding of the 16-bit output on top of err (tests/test_gpu_attention.py::_check)"""
    return err + half_ulp(fmt) * (np.abs(want) + err) + 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------
# the whole chain, and the formula it must equal
# ---------------------------------------------------------------------------------------------------------------
def composed(case, fmt, nodes=4):
    """stage 1 -> 2 -> 3 in float64 with nothing rounded between the stages (every node's reference: its largest score; the scale exact) -> out [n][d]"""
    s1 = stage1(case, fmt, EXACT_SCALE)
    out = np.zeros((case["n"], case["d"]))
    for c in range(case["n"]):
        s2 = stage2(s1["qp"][c], case["E"][c], int(case["k_len"][c]), None, nodes, fmt)
        ml = np.stack([s2["m"], s2["l"]], axis=-1)
        out[c] = stage3(s2["U"], ml, case["wv"], case["bv"], fmt)[0]
    return out


def plain(case, fmt):
    """softmax(q K^T / 8) V with K = E Wk^T, V = E Wv^T + bv, per head, on the same rounded ln and q"""
    q = query(case, fmt)[1]
    n, d, heads = case["n"], case["d"], case["heads"]
    out = np.zeros((n, d))
    for c in range(n):
        Ec = case["E"][c, :int(case["k_len"][c])]
        K, V = Ec @ case["wk"].T, Ec @ case["wv"].T + np.asarray(case["bv"], dtype=np.float64)
        for h in range(heads):
            sl = slice(64 * h, 64 * h + 64)
            s = K[:, sl] @ q[c, sl] / 8.0
            p = np.exp(s - s.max())
            out[c, sl] = (p / p.sum()) @ V[:, sl]
    return out


# ---------------------------------------------------------------------------------------------------------------
# checking a set of stage outputs (the device's, or the emulation's) against the three restatements
# ---------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    """worst |got - want| / bound; where the bound is zero the value must be met exactly"""
    diff = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
    r = np.where(np.isfinite(np.asarray(got, dtype=np.float64)), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


def stage_ratios(case, got, fmt, eps2=EPS_EXP2, clips=None, s1=None):
    """got: dict(qp_hi, qp_lo [n][R][d] values, u_part [n][nodes][R][d], ml_part [n][nodes][R][2], out [n][d] values).  Every element of every
    stage output of the clips listed (default: all) against its restatement -> {"qp", "m", "l", "U", "out"}: worst |got - want| / bound."""
    heads, d, n = case["heads"], case["d"], case["n"]
    nodes = got["u_part"].shape[1]
    s1 = stage1(case, fmt) if s1 is None else s1
    clips = range(n) if clips is None else clips
    rat = dict(qp=0.0, m=0.0, l=0.0, U=0.0, out=0.0)
    for c in clips:
        qp = np.asarray(got["qp_hi"][c, :heads], dtype=np.float64) + np.asarray(got["qp_lo"][c, :heads], dtype=np.float64)
        rat["qp"] = max(rat["qp"], _ratio(qp, s1["qp"][c], s1["qp_err"][c]))
        ml = np.asarray(got["ml_part"][c, :, :heads], dtype=np.float64)
        s2 = stage2(qp, case["E"][c], int(case["k_len"][c]), ml[..., 0], nodes, fmt, eps2)
        rat["m"] = max(rat["m"], _ratio(ml[..., 0], s2["m"], s2["m_err"]))
        rat["l"] = max(rat["l"], _ratio(ml[..., 1], s2["l"], s2["l_err"]))
        rat["U"] = max(rat["U"], _ratio(got["u_part"][c, :, :heads], s2["U"], s2["U_err"]))
        want, err, _ = stage3(got["u_part"][c, :, :heads], ml, case["wv"], case["bv"], fmt, eps2)
        rat["out"] = max(rat["out"], _ratio(got["out"][c], want, out_bound(want, err, fmt)))
    return rat


def readout_ratios(case, got_ident, got, fmt):
    """class 4.  got_ident: the stage outputs with Wk = I (readout_case), got: with the case's own Wk, same resid / ln / Wq / bq.  With Wk = I, Q'_h is
    fp32(scale q_h) in the head's own 64 columns and exactly zero elsewhere, so q's bits are read off hi + lo.
      "q_split":      hi + lo against fp32(q scale), q = r16((hi + lo) / scale): to the split's accuracy (q on the operand grid is part of it: a value
                      off the grid is u16 away from fp32(q scale), 2^11 (fp16) / 2^8 (bf16) bounds)
      "q":            q against the float64 chain: the LayerNorm / projection error and one 16-bit rounding
      "qp_from_bits": Q' with the case's Wk against scale q Wk from the BITS of q: 64 products, the scale, the split"""
    heads, n, d = case["heads"], case["n"], case["d"]
    v = (np.asarray(got_ident["qp_hi"], dtype=np.float64) + got_ident["qp_lo"])[:, :heads]
    own = np.zeros((heads, d), dtype=bool)
    for h in range(heads):
        own[h, 64 * h: 64 * h + 64] = True
    vq = v[:, own].reshape(n, d)
    q_read = r16(vq / SCALE, fmt)
    v_exp = (q_read.astype(np.float32) * np.float32(SCALE)).astype(np.float64)
    rat = dict(q_split=_ratio(vq, v_exp, np.maximum(split_rel(fmt) * np.abs(v_exp), split_floor(fmt))))
    if np.any(v[:, ~own] != 0.0):
        rat["q_split"] = np.inf
    _, _, q_pre, q_err, _ = query(case, fmt)
    rat["q"] = _ratio(q_read, q_pre, q_err + half_ulp(fmt) * (np.abs(q_pre) + q_err) + 2.0 ** -24)
    want, err = qprime(q_read, np.zeros_like(q_read), case["wk"], heads, fmt)
    rat["qp_from_bits"] = _ratio((np.asarray(got["qp_hi"], dtype=np.float64) + got["qp_lo"])[:, :heads], want, err)
    return rat


# ---------------------------------------------------------------------------------------------------------------
# operand classes
# ---------------------------------------------------------------------------------------------------------------
def gaussian_case(d, k_len, fmt, seed=0, k_cap=None):
    """the recipe of tests/test_gpu_whisper.py's cross-attention test, rounded to the operand type; E rows at and beyond k_len hold +-60000"""
    rng = np.random.default_rng([d, seed, len(k_len)])
    k_len = np.asarray(k_len, dtype=np.int32)
    n, heads = len(k_len), d // 64
    k_cap = int(k_len.max()) if k_cap is None else k_cap
    sc = 1.0 / np.sqrt(d)
    case = dict(d=d, heads=heads, n=n, k_len=k_len, k_cap=k_cap)
    case["resid"] = (rng.standard_normal((n, d)) * 1.5 + 0.2).astype(np.float32)
    case["ln_w"] = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    case["ln_b"] = (0.05 * rng.standard_normal(d)).astype(np.float32)
    for name, g in (("wq", 1.6), ("wk", 1.6), ("wv", 1.0)):
        case[name] = r16(rng.standard_normal((d, d)) * sc * g, fmt)
    case["bq"], case["bv"] = (0.1 * rng.standard_normal(d)).astype(np.float32), (0.1 * rng.standard_normal(d)).astype(np.float32)
    E = rng.standard_normal((n, k_cap, d))
    E[:, :, : d // 2] += rng.standard_normal((n, 1, d // 2))
    case["E"] = pad_rows(r16(E, fmt), k_len)
    return case


def pad_rows(E, k_len):
    """+-60000 in a fixed pattern in every row at and beyond a clip's length"""
    n, k_cap, d = E.shape
    big = np.where((np.arange(k_cap * d) * 7 // 3) % 2 == 0, BIG, -BIG).reshape(k_cap, d)
    for c in range(n):
        E[c, int(k_len[c]):] = big[int(k_len[c]):]
    return E


def shaped_scores(case, qp, profile, fmt, arg=None):
    """E of the case with a multiple of the Q' directions added to the valid rows, such that every head's score at frame t moves by profile(t) log2
    units (before E is rounded again).  The direction is the combination of the heads' Q' (each restricted to its own 64 columns) on which every head
    scores 1.  profile: "peak" (arg: the frame per clip, + 64 there: at least 40 above the rest), "rising" / "falling" (3 per frame, less for long clips so that E stays finite:
    every tile rescales / none does)."""
    n, heads, d = case["n"], case["heads"], case["d"]
    E = case["E"].copy()
    for c in range(n):
        L = int(case["k_len"][c])
        t = np.arange(L, dtype=np.float64)
        if profile == "peak":
            f = np.where(t == arg[c], 64.0, 0.0)
        else:
            f = (3.0 if profile == "rising" else -3.0) * t * min(1.0, 320.0 / L)
        g = np.zeros((heads, d))
        for h in range(heads):
            g[h, 64 * h: 64 * h + 64] = qp[c, h, 64 * h: 64 * h + 64]
        a = np.linalg.solve(qp[c] @ g.T, np.ones(heads))          # (Q' g^T) a = 1
        E[c, :L] += f[:, None] * (a @ g)[None, :]
    out = dict(case)
    out["E"] = pad_rows(r16(E, fmt), case["k_len"])
    return out


def readout_case(case):
    """class 4: Wk = I, so that Q'_h returns scale q_h in the head's own columns and zeros elsewhere"""
    out = dict(case)
    out["wk"] = np.eye(case["d"])
    return out


def cancelling_case(case, fmt, nodes=4):
    """class 5: bv = -fp32(Wv U) of the FIRST clip (the float64 chain's) + 2^-10 of sum |Wv U| per element: that clip's output is small against
    the products it is summed from, and its 16-bit step fine enough to show fp32-level errors of stage 3"""
    s1 = stage1(case, fmt)
    s2 = stage2(s1["qp"][0], case["E"][0], int(case["k_len"][0]), None, nodes, fmt)
    want, _, v = stage3(s2["U"], np.stack([s2["m"], s2["l"]], axis=-1), case["wv"], np.zeros(case["d"]), fmt)
    mag = np.einsum("hij,hj->hi", np.abs(case["wv"].reshape(case["heads"], 64, case["d"])), np.abs(v)).reshape(case["d"])
    out = dict(case)
    out["bv"] = (-want.astype(np.float32).astype(np.float64) + 2.0 ** -10 * mag).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------
# float32 / 16-bit emulation of the kernels' arithmetic, with switchable defects (host tests only)
# ---------------------------------------------------------------------------------------------------------------
DEFECTS = ("q_lo", "p_lo", "u_lo", "flat_merge", "leaf_floor", "mask_off_by_one")
F32 = np.float32


def _exp2f(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(np.asarray(x, dtype=F32)).astype(F32)


def emulate(case, fmt, nodes=4, defect=None):
    """The three kernels in float32 numpy with the operand type's roundings where the kernels have them (fp32 sums in numpy's order, 2^x numpy's:
    one valid instance of what the bounds allow).  defect: one of DEFECTS.  -> the dict stage_ratios takes."""
    assert defect is None or defect in DEFECTS
    n, d, heads = case["n"], case["d"], case["heads"]
    R = xa_rows(heads)
    x = case["resid"].astype(F32)
    mean = (x.sum(axis=1, keepdims=True, dtype=F32) / F32(d)).astype(F32)
    xc = x - mean
    inv = (F32(1.0) / np.sqrt((xc * xc).sum(axis=1, keepdims=True, dtype=F32) / F32(d) + F32(1e-5))).astype(F32)
    ln = r16(xc * inv * case["ln_w"].astype(F32) + case["ln_b"].astype(F32), fmt).astype(F32)
    q = r16(ln @ case["wq"].astype(F32).T + case["bq"].astype(F32), fmt).astype(F32)
    wkh = case["wk"].astype(F32).reshape(heads, 64, d)
    v = (np.einsum("nhk,hkj->nhj", q.reshape(n, heads, 64), wkh).astype(F32) * F32(SCALE)).astype(F32)
    qh, ql = split(v, fmt)
    if defect == "q_lo":
        ql = np.zeros_like(ql)
    got = dict(qp_hi=np.full((n, R, d), 7.0), qp_lo=np.full((n, R, d), 7.0), u_part=np.full((n, nodes, R, d), 7.0, dtype=F32),
               ml_part=np.full((n, nodes, R, 2), 7.0, dtype=F32), out=np.zeros((n, d)))
    got["qp_hi"][:, :heads], got["qp_lo"][:, :heads] = qh, ql
    wv, bv = case["wv"].astype(F32).reshape(heads, 64, d), case["bv"].astype(F32)
    for c in range(n):
        L = int(case["k_len"][c])
        E = case["E"][c].astype(F32)
        nt_all = -(-L // TF)
        per = nt_all // LEAVES if defect == "leaf_floor" else -(-nt_all // LEAVES)
        leaves = []
        for i in range(LEAVES):
            t0, t1 = min(i * per, nt_all), min((i + 1) * per, nt_all)
            m = np.full(heads, -1e30, dtype=F32); l = np.zeros(heads, dtype=F32); u = np.zeros((heads, d), dtype=F32)
            for t in range(t0, t1):
                f0 = t * TF
                rows = np.arange(f0, f0 + TF)
                e = np.zeros((TF, d), dtype=F32)
                ok = rows < E.shape[0]
                e[ok] = E[rows[ok]]
                sc = (e @ qh[c].T + e @ ql[c].T).astype(F32)       # [16][heads]
                limit = L + 1 if defect == "mask_off_by_one" else L
                sc[rows >= limit] = F32(-1e30)
                mx = np.maximum(m, sc.max(axis=0))
                if (mx > m).any():
                    corr = _exp2f(m - mx)
                    l = l * corr; u = u * corr[:, None]; m = mx
                p = _exp2f(sc - m[None, :])
                l = (l + p.sum(axis=0, dtype=F32)).astype(F32)
                ph, pl = split(p, fmt)
                if defect == "p_lo":
                    pl = np.zeros_like(pl)
                u = (u + ph.T @ e + pl.T @ e).astype(F32)
            leaves.append((m, l, u))

        def merge(a, b):
            m = np.maximum(a[0], b[0]); wa, wb = _exp2f(a[0] - m), _exp2f(b[0] - m)
            return m, (b[1] * wb + a[1] * wa).astype(F32), (b[2] * wb[:, None] + a[2] * wa[:, None]).astype(F32)

        pairs = [merge(leaves[0], leaves[1]), merge(leaves[2], leaves[3])]
        for s, (m, l, u) in enumerate(pairs if nodes == 2 else leaves):
            got["u_part"][c, s, :heads], got["ml_part"][c, s, :heads, 0], got["ml_part"][c, s, :heads, 1] = u, m, l
        if defect == "flat_merge":
            m = np.max([x[0] for x in leaves], axis=0)
            l = np.zeros(heads, dtype=F32); u = np.zeros((heads, d), dtype=F32)
            for a in leaves:
                w = _exp2f(a[0] - m)
                l = (l + a[1] * w).astype(F32); u = (u + a[2] * w[:, None]).astype(F32)
        else:
            m, l, u = merge(pairs[0], pairs[1])
        vv = (u * (F32(1.0) / l)[:, None]).astype(F32)
        uh, ul = split(vv, fmt)
        if defect == "u_lo":
            ul = np.zeros_like(ul)
        o = (np.einsum("hij,hj->hi", wv, uh) + np.einsum("hij,hj->hi", wv, ul)).astype(F32).reshape(d) + bv
        got["out"][c] = r16(o, fmt)
    return got
