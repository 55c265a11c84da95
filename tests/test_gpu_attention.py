"""The attention kernels alone against float64, through the launches the product makes: the single-query kernels of an incremental decoding step
(k_self_attn1w, k_cross_attn1w with and without the append; pce_selftest_attn1) and the MFMA kernel k_attention_lean16 with per-clip lengths
(pce_selftest_attention_ragged, which goes through launch_attention: one query block takes the streaming instantiation).

The reference is tests/attention_restatement.py on the ROUNDED operands; every element of every output is checked:

    |got - want| <= err + u (|want| + err) + 2^-24,      u = 2^-8 (bf16) / 2^-11 (fp16): one rounding of the 16-bit output

err is derived per element, not fitted.  With p the float64 weights and A = sum_t p_t |v_t|:
  * an fp32 score is 64 products and 3 shuffle additions: |delta_t| <= 67 x 2^-24 x sum_e |q_e k_e| / 8; with delta the largest of a row, a
    normalised weight moves by at most p (e^(2 delta) - 1) (numerator up, denominator down);
  * the exponential itself is within EPS_EXP relative, in the numerator and in the denominator: (1 + EPS_EXP) / (1 - EPS_EXP);
  * the fp32 sums: (roundings on a lane's path + 6 tree levels) x 2^-24 of A for the weighted sum and of the denominator -- the path lengths are
    counted from the kernels in _sum_terms (the reciprocal, <= 3 ulp, and the final product are on those paths);
  * k_attention_lean16 only: P is rounded to the operand type before the second MFMA (half an ulp in the numerator and in the row sum: u A), and
    its fp16 fast path flushes weights below 2^-20 of its reference to zero (keys x 2^-20 of the row sum, against the largest |v| and the output).

EPS_EXP is the one constant the code does not give.  It was measured, not guessed (probe_exp_error below, run once on an MI355X): the first two
lengths of the cross-attention list (1 and 7 keys) in one form-0 call, the returned outputs against float64, the weight errors backed
out by least squares per (clip, head) (64 output elements for 7 weights) and taken relative to the weights of at least an average share (1 / keys):
what a 16-bit output lets one resolve.  Measured with fp16 operands (the finer output) at 6, 12 and 20 heads: 1.26e-4, 1.39e-4, 2.18e-4, so
EPS_EXP_MEASURED = 2.19e-4 and EPS_EXP = 4 x that = 8.76e-4 -- the margin covers inputs the probe did not see.  The figure is the probe's
resolution (half an fp16 ulp of the output spread over 7 weights), not the exponential's true error, which is far smaller: with EPS_EXP = 0 every
test of this file still passed (worst |got - want| / bound 0.79).  The same probe with bf16 outputs resolves 8 times less (1.81e-3, for the record
only; the exponential is the same fp32 instruction in every build).

Worst |got - want| / bound seen with these constants (fp16-resid16 = fp16: the kernels are the same build):
    kernel                       fp16     bf16
    k_self_attn1w                0.209    0.662
    k_cross_attn1w               0.206    0.666
    k_attention_lean16, mode 0   0.178    0.507
    k_attention_lean16, mode 1   0.242    0.632"""
import numpy as np
import pytest

from prosody_control_french_tts_amd import PceError
from tests import attention_restatement as AR
from tests.test_gpu_kernels import bits, val

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS_EXP_MEASURED = 2.19e-4      # worst of 6, 12 and 20 heads (1.26e-4, 1.39e-4, 2.18e-4)
EPS_EXP_MEASURED_BF16 = 1.81e-3
EPS_EXP = 4 * EPS_EXP_MEASURED
BIG = 60000.0                   # finite in both 16-bit types: what must never be read with a non-zero weight
T_CAP = 448


def _half_ulp(ops):
    return 2.0 ** -8 if ops["torch"] == "bfloat16" else 2.0 ** -11


def _big(shape, ops):
    """+-60000 in a fixed pattern, as bit patterns"""
    n = int(np.prod(shape))
    return bits(np.where((np.arange(n) * 7 // 3) % 2 == 0, BIG, -BIG).reshape(shape), ops)


def _normal(rng, shape, scale, ops):
    return bits(rng.standard_normal(shape) * scale, ops)


def _sum_terms(kernel, keys):
    """fp32 roundings on one lane's path of (the weighted sum, the denominator), tree levels apart"""
    if kernel == "self":                        # keys cached + 1: a lane sums every 8th key (then 3 shuffle levels), every 64th weight
        return -(-(keys - 1) // 8) + 2, -(-(keys - 1) // 64) + 4
    if kernel == "cross" and keys <= 128:       # lane = output dimension: all keys in sequence
        return keys + 2, 8 + 3
    if kernel == "cross":                       # a lane sums 8 keys of each 512-column piece
        return 8 * -(-keys // 512) + 2, 8 * -(-keys // 512) + 3
    return keys + 1, keys + 3                   # MFMA accumulators: every key of the row


def _reference(q, k, v, kernel, ops, n_keys=None, causal=False, p_rounded=False, flush=False):
    """q [H][Q][64], k / v [H][K][64] float64 -> (want, err) [H][Q][64]"""
    p, mag = AR.weights(q, k, n_keys, causal)
    want, A = AR.attention(q, k, v, n_keys, causal)
    keys = p.shape[-1]
    delta = (67 * U * mag * (p > 0)).max(axis=-1, keepdims=True)
    rel = np.exp(2 * delta) * (1 + EPS_EXP) / (1 - EPS_EXP) - 1
    n_num, n_den = _sum_terms(kernel, keys)
    err = A * (rel + (n_num + 6) * U + (n_den + 6) * U)
    if p_rounded:
        err = err + _half_ulp(ops) * A
    if flush:
        vmax = np.abs(v[..., :keys, :]).max(axis=-2, keepdims=True)
        err = err + keys * 2.0 ** -20 * (vmax + np.abs(want))
    return want, err


RATIOS = {}


def _check(got_bits, want, err, ops, kernel, what):
    got = val(got_bits, ops)
    assert np.isfinite(got).all(), (kernel, ops["name"], what)
    bound = err + _half_ulp(ops) * (np.abs(want) + err) + 2.0 ** -24
    ratio = float(np.max(np.abs(got - want) / bound))
    key = (kernel, ops["name"])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"attention-ratio {kernel} {ops['name']} {what}: {ratio:.4f} (worst so far {RATIOS[key]:.4f})")
    bad = np.abs(got - want) > bound
    assert not bad.any(), (kernel, ops["name"], what, int(bad.sum()), ratio, np.argwhere(bad)[:4].tolist())


def _heads(x_bits, ops, H):
    """[rows][H * 64] bit patterns -> float64 [H][rows][64]"""
    return AR.split_heads(val(x_bits, ops), H)


# ---------------------------------------------------------------------------------------------------------------
# k_self_attn1w (form 2) and k_cross_attn1w appending (form 1)
# ---------------------------------------------------------------------------------------------------------------
class Step:
    """One incremental step of n clips at positions pos: the new q | k | v, a prefix of pos[i] cached keys / values per clip, and +-60000 in every
    cache row from pos[i] on (row pos[i] is the one the launch writes)."""

    def __init__(self, ops, H, pos, seed, t_cap=T_CAP):
        rng = np.random.default_rng(seed)
        self.ops, self.H, self.pos, self.n, self.d, self.t_cap = ops, H, list(pos), len(pos), H * 64, t_cap
        n, d = self.n, self.d
        self.qkv = np.concatenate([_normal(rng, (n, 2 * d), 1.5, ops), _normal(rng, (n, d), 1.0, ops)], axis=1)
        self.ck, self.cv = _big((n, t_cap, d), ops), _big((n, t_cap, d), ops)
        for i, p in enumerate(self.pos):
            self.ck[i, :p] = _normal(rng, (p, d), 1.5, ops)
            self.cv[i, :p] = _normal(rng, (p, d), 1.0, ops)
        self.prefill = _normal(rng, (n, d), 1.0, ops)

    def reference(self, i, kernel):
        p, d = self.pos[i], self.d
        q = _heads(self.qkv[i:i + 1, :d], self.ops, self.H)
        k = _heads(np.concatenate([self.ck[i, :p], self.qkv[i:i + 1, d:2 * d]]), self.ops, self.H)
        v = _heads(np.concatenate([self.cv[i, :p], self.qkv[i:i + 1, 2 * d:]]), self.ops, self.H)
        want, err = _reference(q, k, v, kernel, self.ops)
        return AR.merge_heads(want)[0], AR.merge_heads(err)[0]

    def run(self, eng, form, skip=None):
        """-> (out, K cache, V cache [n][t_cap][d] whichever form holds it) after the call"""
        out, ck = self.prefill.copy(), self.ck.copy()
        if form == 2:
            cv = self.cv.copy()
            eng.selftest_attn1(2, self.H, self.qkv, ck, cv, self.pos, out, skip=skip, span=self.t_cap)
            return out, ck, cv
        vt = _big((self.n, self.d, 512), self.ops)                    # V^T cache, column pos[i] included: a finite value other than the new one
        vt[:, :, :self.t_cap] = self.cv.transpose(0, 2, 1)
        eng.selftest_attn1(1, self.H, self.qkv, ck, vt, self.pos, out, skip=skip, span=self.t_cap)
        assert np.array_equal(vt[:, :, self.t_cap:], _big((self.n, self.d, 512), self.ops)[:, :, self.t_cap:])
        return out, ck, np.ascontiguousarray(vt[:, :, :self.t_cap].transpose(0, 2, 1))

    def check(self, eng, form, skip=None):
        kernel = "self" if form == 2 else "cross"
        out, ck, cv = self.run(eng, form, skip)
        d = self.d
        for i, p in enumerate(self.pos):
            what = (f"form {form}", self.H, p)
            if skip is not None and skip[i]:
                assert np.array_equal(out[i], self.prefill[i]), what
                assert np.array_equal(ck[i], self.ck[i]) and np.array_equal(cv[i], self.cv[i]), what
                continue
            want, err = self.reference(i, kernel)
            _check(out[i], want, err, self.ops, kernel, what)
            assert np.array_equal(ck[i, p], self.qkv[i, d:2 * d]) and np.array_equal(cv[i, p], self.qkv[i, 2 * d:]), what      # every head's columns
            rest = np.arange(self.t_cap) != p
            assert np.array_equal(ck[i, rest], self.ck[i, rest]) and np.array_equal(cv[i, rest], self.cv[i, rest]), what
        return out


SELF_CASES = {6: (0, 64, 447), 16: (1, 63, 128), 17: (7, 65, 127), 20: (8, 128, 447), 32: (0, 1, 447)}


@pytest.mark.parametrize("H", sorted(SELF_CASES))
def test_self_attn1_against_float64(engine, ops, H):
    """k_self_attn1w: one head group (6), a full 16-wave group, 2 groups of 9 with a short last group (17), the turbo case (2 x 10), 2 x 16; the
    positions cover {0, 1, 7, 8, 63, 64, 65, 127, 128, 447}: no cached key, one, the 8-row and 64-row steps of the key walk and their neighbours,
    the last row of the cache.  Row pos of both caches is the new k / v bit for bit, nothing else in them changes, and a skipped clip keeps its
    output row and its caches."""
    s = Step(ops, H, SELF_CASES[H], seed=H)
    first = s.check(engine, 2)
    again = s.check(engine, 2, skip=[0, 1, 0])
    assert np.array_equal(again[[0, 2]], first[[0, 2]])


APPEND_CASES = [(0, 1, 126, 127), (128, 129, 447)]


@pytest.mark.parametrize("H", [6, 20])
def test_cross_attn1_append_against_float64(engine, ops, H):
    """k_cross_attn1w appending (the self-attention of a step on K rows + V^T, PCE_SELF_ROWS=0), across the 128-key branch in both directions.  The
    V^T column being written holds a finite value other than the new one before the call: the new key's weight must come from registers."""
    for ci, pos in enumerate(APPEND_CASES):
        s = Step(ops, H, pos, seed=100 + H + ci)
        s.check(engine, 1)
    s.check(engine, 1, skip=[1, 0, 0])


def test_append_forms_agree_with_the_same_float64_answer(engine, ops):
    """The two kernels on the same prefix are each within their bound of the same float64 answer (they do not promise each other's bits)."""
    s = Step(ops, 12, (3, 127, 128, 300), seed=7)
    s.check(engine, 1)
    s.check(engine, 2)


# ---------------------------------------------------------------------------------------------------------------
# k_cross_attn1w without the append (form 0)
# ---------------------------------------------------------------------------------------------------------------
class Cross:
    """n clips with k_len keys each: key rows at distinct non-zero k_row0 with +-60000 rows between and after them, the whole V^T image at pitch
    1536 with +-60000 in every column >= k_len."""

    def __init__(self, ops, H, lens, seed, vt_sp=1536):
        rng = np.random.default_rng(seed)
        self.ops, self.H, self.lens, self.n, self.d, self.vt_sp = ops, H, list(lens), len(lens), H * 64, vt_sp
        n, d = self.n, self.d
        self.row0, r = [], 3
        for L in self.lens:
            self.row0.append(r)
            r += L + 5
        self.q = _normal(rng, (n, d), 1.5, ops)
        self.k = _big((r, d), ops)
        self.vt = _big((n, d, vt_sp), ops)
        self.v = []
        for i, L in enumerate(self.lens):
            self.k[self.row0[i]:self.row0[i] + L] = _normal(rng, (L, d), 1.5, ops)
            v = _normal(rng, (L, d), 1.0, ops)
            self.vt[i, :, :L] = v.T
            self.v.append(v)
        self.prefill = _normal(rng, (n, d), 1.0, ops)

    def run(self, eng, skip=None):
        out, k, vt = self.prefill.copy(), self.k.copy(), self.vt.copy()
        eng.selftest_attn1(0, self.H, self.q, k, vt, self.lens, out, k_row0=self.row0, skip=skip, span=self.vt_sp)
        assert np.array_equal(k, self.k) and np.array_equal(vt, self.vt)
        return out

    def check(self, eng, skip=None):
        out = self.run(eng, skip)
        for i, L in enumerate(self.lens):
            if skip is not None and skip[i]:
                assert np.array_equal(out[i], self.prefill[i]), (self.H, L)
                continue
            want, err = _reference(_heads(self.q[i:i + 1], self.ops, self.H), _heads(self.k[self.row0[i]:self.row0[i] + L], self.ops, self.H),
                                   _heads(self.v[i], self.ops, self.H), "cross", self.ops)
            _check(out[i], AR.merge_heads(want)[0], AR.merge_heads(err)[0], self.ops, "cross", ("form 0", self.H, L))
        return out


CROSS_LENS = [(1, 7, 8, 64), (65, 128, 129, 511), (512, 513, 1024), (1025, 1500, 1536)]


@pytest.mark.parametrize("H", [6, 12, 20])
def test_cross_attn1_against_float64(engine, ops, H):
    """k_cross_attn1w over given keys: both sides of the 128-key branch, of the 64-row step of the key walk and of every 512-column piece of the
    V^T image (1, 2 and 3 pieces), the last key of a full image; a V^T column or a key row past k_len that got a weight would show as +-60000."""
    for ci, lens in enumerate(CROSS_LENS):
        c = Cross(ops, H, lens, seed=200 + 10 * H + ci)
        first = c.check(engine)
        if ci == 0:
            again = c.check(engine, skip=[0, 1, 0, 1])
            assert np.array_equal(again[[0, 2]], first[[0, 2]])


def test_a_clip_does_not_depend_on_its_batch(engine, ops):
    """Clip 0 alone and clip 0 inside a batch of 5 give identical bits (20 heads: two head groups per clip)."""
    c5 = Cross(ops, 20, (513, 7, 1500, 64, 129), seed=31)
    c1 = Cross(ops, 20, (513,), seed=0)
    c1.q, c1.k, c1.vt, c1.prefill, c1.row0 = c5.q[:1].copy(), c5.k, c5.vt[:1].copy(), c5.prefill[:1].copy(), c5.row0[:1]
    assert np.array_equal(c1.run(engine)[0], c5.run(engine)[0])
    s5 = Step(ops, 20, (130, 0, 447, 64, 9), seed=32)
    s1 = Step(ops, 20, (130,), seed=0)
    s1.qkv, s1.ck, s1.cv, s1.prefill = s5.qkv[:1].copy(), s5.ck[:1].copy(), s5.cv[:1].copy(), s5.prefill[:1].copy()
    assert np.array_equal(s1.run(engine, 2)[0][0], s5.run(engine, 2)[0][0])


def test_attn1_refuses_what_it_cannot_address(engine, ops):
    """PCE_E_INVALID before anything is launched: key counts outside 1 .. 1536 or past the image's pitch, a position outside the cache, a cache
    longer than 512, more than 32 heads, arrays shorter than the shape needs."""
    H, d = 2, 128
    z = lambda *s: np.zeros(s, np.uint16)
    ok = dict(q=z(2, d), k=z(40, d), v=z(2, d, 64), out=z(2, d))

    def form0(lens=(8, 16), row0=(0, 20), span=64, heads=H, **kw):
        a = dict(ok, **kw)
        engine.selftest_attn1(0, heads, a["q"], a["k"], a["v"], lens, a["out"], k_row0=row0, span=span)

    form0()
    for bad in (dict(lens=(0, 16)), dict(lens=(8, 65)), dict(lens=(8, 1537), span=1600), dict(row0=(0, 25)), dict(row0=(-1, 20)), dict(span=60),
                dict(q=z(2 * d - 1)), dict(v=z(2 * d * 64 - 1)), dict(out=z(2 * d - 1)), dict(heads=33)):
        with pytest.raises(PceError, match="status -1"):
            form0(**bad)
    for form in (1, 2):
        v_elems = 2 * d * 512 if form == 1 else 2 * 16 * d

        def step(pos=(0, 15), span=16, q=z(2, 3 * d), k=z(2, 16, d), v=None, out=z(2, d)):
            engine.selftest_attn1(form, H, q, k, z(v_elems) if v is None else v, pos, out, span=span)

        step()
        for bad in (dict(pos=(0, 16)), dict(pos=(-1, 3)), dict(span=513), dict(q=z(2 * 3 * d - 1)), dict(k=z(2 * 16 * d - 1)), dict(v=z(v_elems - 1)),
                    dict(out=z(2 * d - 1))):
            with pytest.raises(PceError, match="status -1"):
                step(**bad)


def probe_exp_error(engine, ops, H=20):
    """The measurement behind EPS_EXP (see the module docstring) -> worst relative weight error the probe resolves."""
    c = Cross(ops, H, CROSS_LENS[0][:2], seed=200 + 10 * H)
    out = val(c.run(engine), ops)
    worst = 0.0
    for i, L in enumerate(c.lens):
        q, k, v = (_heads(x, ops, H) for x in (c.q[i:i + 1], c.k[c.row0[i]:c.row0[i] + L], c.v[i]))
        p, _ = AR.weights(q, k)
        want, _ = AR.attention(q, k, v)
        diff = AR.split_heads(out[i:i + 1], H)[:, 0] - want[:, 0]                     # [H][64]
        for h in range(H):
            x = np.linalg.lstsq(v[h].T, diff[h], rcond=None)[0]                      # sum_t x_t v_t = diff: x_t = p_t e_t
            w = p[h, 0]
            live = w >= 1.0 / L
            worst = max(worst, float(np.max(np.abs(x[live]) / w[live])))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# k_attention_lean16 through launch_attention
# ---------------------------------------------------------------------------------------------------------------
def _lean(engine, ops, H, q_len, k_len, causal, mode, seed, extra_rows=3):
    """one ragged call -> checks every row of every clip against float64, the rows no query owns against the prefill"""
    rng = np.random.default_rng(seed)
    hd = H * 64
    q = _normal(rng, (sum(q_len), hd), 1.5, ops)
    k = _normal(rng, (sum(k_len), hd), 1.5, ops)
    v = _normal(rng, (sum(k_len), hd), 1.0, ops)
    prefill = _normal(rng, (sum(q_len) + extra_rows, hd), 1.0, ops)
    out = prefill.copy()
    fell_back = engine.selftest_attention_ragged(q, k, v, q_len, k_len, out, causal=causal, mode=mode)
    assert fell_back == 0
    assert np.array_equal(out[sum(q_len):], prefill[sum(q_len):])
    flush = mode == 0 and ops["torch"] == "float16"
    q0 = k0 = 0
    for ql, kl in zip(q_len, k_len):
        want, err = _reference(_heads(q[q0:q0 + ql], ops, H), _heads(k[k0:k0 + kl], ops, H), _heads(v[k0:k0 + kl], ops, H), "lean", ops,
                               causal=causal, p_rounded=True, flush=flush)
        _check(out[q0:q0 + ql], AR.merge_heads(want), AR.merge_heads(err), ops, f"lean16 mode {mode}", (H, ql, kl, causal))
        q0 += ql; k0 += kl


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H", [6, 20])
def test_lean16_streaming_launch_against_float64(engine, ops, H, mode):
    """One query block per (clip, head) -- every decoder cross-attention over the 1 500 audio positions -- takes the NT instantiation: 1, 40 and 128
    queries."""
    for q_len in (1, 40, 128):
        _lean(engine, ops, H, [q_len], [1500], False, mode, seed=300 + H + q_len)


@pytest.mark.parametrize("mode", [0, 1])
def test_lean16_ragged_causal_against_float64(engine, ops, mode):
    """Three clips of 1, 77 and 130 tokens in one causal call at 12 heads: the grid is the longest clip's (2 query blocks), the short clips' second
    block leaves at once, and a row a clip does not own belongs to the next clip or keeps the prefill."""
    _lean(engine, ops, 12, [1, 77, 130], [1, 77, 130], True, mode, seed=400)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,clips", [(6, 3), (20, 2)])
def test_lean16_both_sides_of_the_xcd_remap(engine, ops, H, clips, mode):
    """2 query blocks x 6 heads x 3 clips = 36 workgroups (not a multiple of the 8 XCDs: the remap's remainder branch) and 2 x 20 x 2 = 80 (a
    multiple), with a different key count per clip."""
    _lean(engine, ops, H, [130 + 7 * i for i in range(clips)], [200 + 65 * i for i in range(clips)], False, mode, seed=500 + H)
