"""The encoder-output cross-attention of an incremental decoding step, kernel by kernel against float64 (csrc/pce_xattn.inc: k_xq_fused ->
k_xattn_absorbed -> k_uv_absorb, through pce_selftest_xattn_stages: the product's own launch, with Q', the nodes' U and (m, l) copied out).

The reference is tests/xattn_restatement.py: each stage is restated from the DEVICE'S output of the stage before it, so an error is pinned to the kernel
that made it, and every element of every stage output is checked against a bound derived there from the kernels' operation counts and the number formats.
tests/test_xattn_host.py shows on the CPU that the bounds hold for the kernels' arithmetic and fail for its defects (a dropped lo part, a wrong leaf
rule, a mask off by one frame).

Shapes: every width (each is its own instantiation), the frame counts X.K_LENS (leaves of 1 / 0 / 0 / 0 up to 3 / 3 / 3 / 1 tiles, edge tiles masked and
not, workgroups without a tile at 2 and 4 per clip), 1, 16 and 17 clips (a second 16-clip block of k_xq_fused / k_uv_absorb with one live lane), 1 / 2 / 4
workgroups per clip (bit-identical outputs, and nodes where two settings write the same kind), 1500 and 1499 frames at both ring depths, +-60000 in every
row of E no frame owns, a recognisable fill in every buffer row no head owns, ended clips.

Operand classes: Gaussian; one score 64 log2 units above the mean (40 above the rest), in each leaf and on the last frame; scores rising / falling by 3 per frame (every
tile rescales / none does; merge weights underflow); Wk = I (Q' returns q itself: its bits, the split, then Q' from those bits with a Gaussian Wk);
bv cancelling Wv U (the 16-bit output step then shows stage 3's fp32 errors).

The exponential.  The bounds need the relative error of __builtin_amdgcn_exp2f; the project's EPS_EXP (8.76e-4, the resolution of a 16-bit probe) would hide P's
lo part again.  probe_exp2_error below (not collected) measured it on an MI355X, 2026-10-20: heads with one non-zero Q' column (a single 1 per head in Wk), powers
of two in that column of E, so that s_t - m is exact in fp32, and a one-hot marker column no score reads.  A weight that went through the P operand would come back
as hi + lo (22 bits, nothing below 2^-24 in fp16), so the marker sits on the leaf's FIRST tile, where its weight is exactly 1, and the second tile's larger
score rescales it: u_part returns the instruction's fp32 result for the argument m_old - m_new untouched.
    EPS_EXP2_MEASURED = 5.84e-8 over 1773 arguments (531 distinct) in [-125.51, -0.36], against float64 2^x; the bounds use 4 x it (the probe does not see
    every argument).  With that margin "P's lo dropped" still leaves the stage-2 bound on the host at d = 128 in fp16, and no longer at d >= 768: that is the
    worst-case score term, not the margin (tests/test_xattn_host.py has the numbers).

Worst |got - want| / bound per (stage, operand type) over this file on the MI355X, 2026-10-20 (every test prints its own as "xattn-ratio"):
    stage            fp16     bf16
    qp               0.461    0.636      k_xq_fused, Gaussian operands (the bound allows q to move by a 16-bit step)
    q_split          1.000    0.355      k_xq_fused, Wk = I: hi + lo against fp32(q scale) (1.000: half a subnormal step of fp16, exactly)
    q                0.920    0.984      k_xq_fused, Wk = I: q's bits against the float64 LayerNorm and projection (one 16-bit rounding: reaches 1)
    qp_from_bits     0.043    0.341      k_xq_fused: Q' against scale q Wk from q's bits
    m                0.023    0.021      k_xattn_absorbed: the node's reference against the largest float64 score
    l                0.008    0.011      k_xattn_absorbed
    U                0.033    0.022      k_xattn_absorbed
    out              0.943    0.956      k_uv_absorb (one rounding of the 16-bit output: reaches 1)
Before k_xq_fused's split was mended (hi and lo taken from two different roundings of the product, see the kernel) qp_from_bits was 33 to 141 in fp16 at
d >= 384: one element in 2^13 a full step of hi away."""
import numpy as np
import pytest

from prosody_control_french_tts_amd import PceError
from tests import xattn_restatement as X
from tests.test_gpu_kernels import bits, val

pytestmark = pytest.mark.gpu

FILL = dict(out=5.0, qp_hi=3.0, qp_lo=-3.0, u_part=7.0, ml_part=9.0)
RATIOS = {}


@pytest.fixture(params=["fp16", "bf16"])
def ops(request, engine):
    engine.whisper_set_operands(request.param)
    yield dict(name=request.param, torch="bfloat16" if request.param == "bf16" else "float16")
    engine.whisper_set_operands("fp16-resid16")


def _note(stage, ops, ratio, what):
    key = (stage, ops["name"])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"xattn-ratio {stage} {ops['name']} {what}: {ratio:.4f} (worst so far {RATIOS[key]:.4f})")


def run(engine, case, ops, wpc, skip=None):
    """one call -> the dict X.stage_ratios takes (values) with the raw arrays under "raw"; rows no head owns and what lies past the nodes written
    must come back as they went in"""
    n, d, heads = case["n"], case["d"], case["heads"]
    R = X.xa_rows(heads)
    b = case.setdefault("_bits", {})
    for k in ("wq", "wk", "wv", "E"):
        if k not in b or b[k][0] is not case[k]:
            b[k] = (case[k], bits(case[k], ops))
    f32 = lambda k: np.ascontiguousarray(case[k], dtype=np.float32)
    out = bits(np.full((n, d), FILL["out"]), ops)
    qh, ql = bits(np.full((n, R, d), FILL["qp_hi"]), ops), bits(np.full((n, R, d), FILL["qp_lo"]), ops)
    u = np.full((n * 4 * R * d,), FILL["u_part"], dtype=np.float32)
    ml = np.full((n * 4 * R * 2,), FILL["ml_part"], dtype=np.float32)
    nodes = engine.selftest_xattn_stages(f32("resid"), f32("ln_w"), f32("ln_b"), b["wq"][1], f32("bq"), b["wk"][1], b["wv"][1], f32("bv"), b["E"][1],
                                         case["k_len"], heads, out, qh, ql, u, ml, skip=skip, workgroups_per_clip=wpc)
    assert nodes == X.nodes_of(d, wpc), (d, wpc, nodes)
    nu, nm = n * nodes * R * d, n * nodes * R * 2
    assert np.all(u[nu:] == np.float32(FILL["u_part"])) and np.all(ml[nm:] == np.float32(FILL["ml_part"])), (d, wpc)
    u, ml = u[:nu].reshape(n, nodes, R, d), ml[:nm].reshape(n, nodes, R, 2)
    assert np.all(u[:, :, heads:] == np.float32(FILL["u_part"])) and np.all(ml[:, :, heads:] == np.float32(FILL["ml_part"])), (d, wpc)
    vh, vl = val(qh, ops), val(ql, ops)
    assert np.all(vh[:, heads:] == FILL["qp_hi"]) and np.all(vl[:, heads:] == FILL["qp_lo"]), (d, wpc)
    return dict(out=val(out, ops), qp_hi=vh, qp_lo=vl, u_part=u, ml_part=ml, raw=(out, qh, ql, u, ml))


def same(a, b, parts=(0, 1, 2, 3, 4)):
    return all(np.array_equal(a["raw"][i], b["raw"][i]) for i in parts)


def check(case, got, ops, what, clips=None, s1=None):
    rat = X.stage_ratios(case, got, ops["name"], clips=clips, s1=s1)
    for stage, r in rat.items():
        _note(stage, ops, r, what)
    assert all(r <= 1.0 for r in rat.values()), (what, ops["name"], rat)
    return rat


def run_all_wpc(engine, case, ops, what):
    """1, 2 and 4 workgroups per clip: every stage output against float64, out (and Q') bit-identical, nodes too where the kind is the same"""
    d = case["d"]
    s1 = X.stage1(case, ops["name"])
    got = {w: run(engine, case, ops, w) for w in (4, 2, 1)}
    check(case, got[4], ops, (what, "wpc 4"), s1=s1)
    for w in (2, 1):
        assert same(got[w], got[4], (0, 1, 2)), (what, w)
        if X.nodes_of(d, w) == 4 or w == 1:
            assert same(got[w], got[4] if X.nodes_of(d, w) == 4 else got[2], (3, 4)), (what, w)
    if X.nodes_of(d, 2) == 2:
        check(case, got[2], ops, (what, "wpc 2"), s1=s1)
    return got


# ---------------------------------------------------------------------------------------------------------------
# class 1: Gaussian operands at every shape
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", X.WIDTHS)
def test_every_stage_against_float64_at_every_leaf_pattern(engine, ops, d):
    lens = X.K_LENS if d in X.FULL_WIDTHS else X.SUBSET
    case = X.gaussian_case(d, lens, ops["name"], seed=1)
    got = run_all_wpc(engine, case, ops, (d, "lens"))
    # the batch: 1 and 16 clips (and 17 where the list is shorter: the second 16-clip block with one live lane) give every clip the bits it has here
    for n in (1, 16, 17):
        if n == len(lens):
            continue
        idx = np.arange(n) % len(lens)
        sub = dict(case, n=n, k_len=case["k_len"][idx], resid=case["resid"][idx], E=np.ascontiguousarray(case["E"][idx]))
        sub.pop("_bits")
        g = run(engine, sub, ops, 0)
        ref = got[4] if X.nodes_of(d, 4) == g["u_part"].shape[1] else got[2]
        for i, part in enumerate(g["raw"][:3]):
            assert np.array_equal(part, got[4]["raw"][i][idx]), (d, n, i)
        assert np.array_equal(g["u_part"], ref["u_part"][idx]) and np.array_equal(g["ml_part"], ref["ml_part"][idx]), (d, n)


@pytest.mark.parametrize("d", [128, 768])
def test_the_products_window_and_one_frame_short_of_it(engine, ops, d):
    """1500 and 1499 frames: 94 tiles, leaves of 24 / 24 / 24 / 22, at the three-slot ring (128) and the two-slot ring (768)"""
    case = X.gaussian_case(d, [1500, 1499], ops["name"], seed=2)
    run_all_wpc(engine, case, ops, (d, "1500"))


def test_ended_clips_are_left_alone(engine, ops):
    """skip: clips 0, 8 and n - 1 keep the fill in out, Q', U and (m, l); every other clip has the bits it has without the list"""
    for d in (128, 1280):
        case = X.gaussian_case(d, X.K_LENS, ops["name"], seed=1)
        n, heads = case["n"], case["heads"]
        skip = np.zeros(n, dtype=np.int32)
        skip[[0, 8, n - 1]] = 1
        live = np.flatnonzero(skip == 0)
        for wpc in (4, 1):
            full, part = run(engine, case, ops, wpc), run(engine, case, ops, wpc, skip=skip)
            for i in range(5):
                assert np.array_equal(part["raw"][i][live], full["raw"][i][live]), (d, wpc, i)
            dead = np.flatnonzero(skip)
            assert np.all(part["out"][dead] == FILL["out"]) and np.all(part["qp_hi"][dead] == FILL["qp_hi"]) and np.all(part["qp_lo"][dead] == FILL["qp_lo"])
            assert np.all(part["u_part"][dead] == np.float32(FILL["u_part"])) and np.all(part["ml_part"][dead] == np.float32(FILL["ml_part"]))
            check(case, part, ops, (d, "skip", wpc), clips=live)


# ---------------------------------------------------------------------------------------------------------------
# classes 2 and 3: peaked and monotone scores
# ---------------------------------------------------------------------------------------------------------------
def _device_qp(engine, case, ops):
    g = run(engine, case, ops, 4)
    return (g["qp_hi"] + g["qp_lo"])[:, :case["heads"]]


@pytest.mark.parametrize("d", [128, 768, 1024, 1280])
def test_one_score_far_above_the_rest(engine, ops, d):
    """the peak (64 log2 units along the device's Q') at the first frame of every leaf and on the last valid frame: the other leaves' weights underflow in
    the merge, the peak's own leaf rescales once or never"""
    case = X.gaussian_case(d, X.PEAK_LENS, ops["name"], seed=3)
    peaked = X.shaped_scores(case, _device_qp(engine, case, ops), "peak", ops["name"], X.PEAK_AT)
    run_all_wpc(engine, peaked, ops, (d, "peak"))


@pytest.mark.parametrize("profile", ["rising", "falling"])
@pytest.mark.parametrize("d", [128, 768, 1024, 1280])
def test_monotone_scores(engine, ops, d, profile):
    """scores that rise by 3 per frame rescale at every tile, scores that fall never do"""
    case = X.gaussian_case(d, X.MONOTONE_LENS, ops["name"], seed=4)
    shaped = X.shaped_scores(case, _device_qp(engine, case, ops), profile, ops["name"])
    run_all_wpc(engine, shaped, ops, (d, profile))


# ---------------------------------------------------------------------------------------------------------------
# class 4: the query read out through Wk = I
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", X.WIDTHS)
def test_query_bits_and_q_prime_from_them(engine, ops, d):
    """With Wk = I, Q'_h is scale q_h in the head's own 64 columns and zero elsewhere: q is read off hi + lo (it must lie on the operand grid and agree
    with the float64 chain to the LayerNorm / projection bound plus one 16-bit rounding), hi + lo must equal fp32(q scale) to the split's accuracy -- a
    dropped lo is 2^-12 of the value against 2^-22 (fp16) -- and then, with a Gaussian Wk, Q' is checked against the query BITS read here with the
    64-term accumulation bound (going through the float64 q would let one 16-bit step of q swamp the check)."""
    fmt = ops["name"]
    case = X.gaussian_case(d, [16] * 17, fmt, seed=5)
    rat = X.readout_ratios(case, run(engine, X.readout_case(case), ops, 4), run(engine, case, ops, 4), fmt)
    for stage, r in rat.items():
        _note(stage, ops, r, d)
    assert all(r <= 1.0 for r in rat.values()), (d, fmt, rat)


# ---------------------------------------------------------------------------------------------------------------
# class 5: cancellation at the output
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 768, 1280])
def test_output_with_bv_cancelling_the_product(engine, ops, d):
    case = X.cancelling_case(X.gaussian_case(d, [160, 97, 17], ops["name"], seed=6), ops["name"])
    got = run_all_wpc(engine, case, ops, (d, "cancel"))
    small = np.abs(got[4]["out"][0]).max() / np.abs(got[4]["out"][1]).max()
    assert small < 0.05, small                                    # (the first clip's output really is what is left of a cancellation)


def test_stage_hook_refuses_what_it_cannot_address(engine, ops):
    case = X.gaussian_case(128, [16, 5], ops["name"], seed=7)
    z16, z32 = (lambda k: np.zeros(k, dtype=np.uint16)), (lambda k: np.zeros(k, dtype=np.float32))
    f32 = lambda k: np.ascontiguousarray(case[k], dtype=np.float32)
    b = {k: bits(case[k], ops) for k in ("wq", "wk", "wv", "E")}
    R, d, n = 16, 128, 2

    def call(out=n * d, qp=n * R * d, u=n * 4 * R * d, ml=n * 4 * R * 2, k_len=(16, 5), wpc=4, E=None):
        engine.selftest_xattn_stages(f32("resid"), f32("ln_w"), f32("ln_b"), b["wq"], f32("bq"), b["wk"], b["wv"], f32("bv"), b["E"] if E is None else E,
                                     k_len, 2, z16(out), z16(qp), z16(qp), z32(u), z32(ml), workgroups_per_clip=wpc)
    call()
    for bad in (dict(out=n * d - 1), dict(qp=n * R * d - 1), dict(u=n * 4 * R * d - 1), dict(ml=n * 4 * R * 2 - 1), dict(k_len=(17, 5)), dict(k_len=(16, 0)),
                dict(wpc=3)):
        with pytest.raises(PceError, match="status -1"):
            call(**bad)


# ---------------------------------------------------------------------------------------------------------------
# the measurement behind EPS_EXP2 (not collected)
# ---------------------------------------------------------------------------------------------------------------
def probe_exp2_error(engine, d=1280, rounds=24):
    """-> (worst |device 2^x / 2^x - 1|, the sorted arguments x seen).  Per head h: Wq = 0 and bq = a value with seven significant bits, so q_h[0] is that
    value; Wk[64 h][h] = 1, so Q'_h = fp32(scale q) in column h alone, a 24-bit window as hi + lo.  One clip of 128 frames: leaf i is tiles 2 i and
    2 i + 1.  Column h of E holds 0 in the leaf's first tile and k_i (0.5, 1, 2, 4: powers of two, so s = k_i Q'_h is exact in fp32) in its second; column
    `heads`, which no Q' reads, holds 1 in the leaf's first frame.  After the first tile m = 0 and U[heads] = 1 exactly; the second tile rescales by
    2^(0 - s), so u_part[i][h][heads] IS the instruction's result for the argument -k_i Q'_h, in fp32, untouched by any 16-bit part (a weight that
    went through the P operand would come back as hi + lo: 22 bits, and nothing below 2^-24 in fp16)."""
    engine.whisper_set_operands("fp16")
    ops = dict(name="fp16", torch="float16")
    heads = d // 64
    ks = (0.5, 1.0, 2.0, 4.0)
    worst, args = 0.0, []
    for r in range(rounds):
        case = X.gaussian_case(d, [128], "fp16", seed=100 + r)
        case["wq"] = np.zeros((d, d))
        mant = 64 + (np.arange(heads) * 13 + r * 29) % 64           # 7 significant bits: on both 16-bit grids
        expo = (np.arange(heads) + 3 * r) % 7 - 4                   # q from 4 to 508: Q' from 0.7 to 92
        bq = np.zeros(d); bq[64 * np.arange(heads)] = mant * 2.0 ** expo
        case["bq"] = bq.astype(np.float32)
        wk = np.zeros((d, d)); wk[64 * np.arange(heads), np.arange(heads)] = 1.0
        case["wk"] = wk
        E = np.zeros((1, 128, d))
        for i, k in enumerate(ks):
            E[0, 32 * i + 16: 32 * i + 32, :heads] = k
            E[0, 32 * i, heads] = 1.0
        case["E"] = E
        g = run(engine, case, ops, 4)
        qp = (g["qp_hi"] + g["qp_lo"])[0, :heads]
        for h in range(heads):
            assert np.count_nonzero(qp[h]) == 1 and qp[h, h] > 0
            for i, k in enumerate(ks):
                x = -k * qp[h, h]
                assert float(np.float32(x)) == x and g["ml_part"][0, i, h, 0] == np.float32(-x)
                if x >= -126.0:
                    worst = max(worst, abs(float(g["u_part"][0, i, h, heads]) / 2.0 ** x - 1.0))
                    args.append(x)
    return worst, np.sort(np.array(args))
