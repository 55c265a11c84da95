"""The persistent 256 x 256 GEMM (k_gemm_flat, csrc/pce_gemm256.inc) through the product's launch_gemm_flat (engine.selftest_gemm: plain, GELU,
V^T and split epilogues; engine.selftest_gemm_resid: the residual epilogue in place), in exact arithmetic and against float64.

Shapes: tests/gemm_flat_cases.py, one per path of the tile walk, the K loop's wait regimes, tiles per workgroup, padding tiles and the V^T
image's store paths; tests/test_gemm_flat_host.py proves on the CPU that each shape is in the class it claims (at 256 workgroups; on a device
with another CU count the class assertions here are skipped, never the numeric checks).  The hooks zero the output first and every case but one
passes a nonzero bias, so a store from a padding tile (zero accumulators) never looks like untouched memory.

Where every bound comes from (restated in tests/gemm_restatement.py):

  * exact family: A multiples of 2^-2 in [-4, 4], B multiples of 2^-3 in [-1, 1], bias nonzero multiples of 2^-4.  Every partial sum is a multiple
    of 2^-5 of at most (4 K + |bias|) x 32 <= (12 288 + 1 300) x 32 < 2^19 units, far below 2^24 (asserted per problem from the operands drawn), so
    fp32 accumulation is exact in any order, inside the MFMA too.  Plain epilogue: the output IS rne16(A B^T + bias) computed in float64, one rounding from the exact value: np.array_equal on the bit
    patterns, no element excused, ties included.  A mismatch is a kernel or launcher bug by construction; the report names row, column, tile,
    workgroup, place in its stream and ring parity of its first K-step (flat_walk), wave, lane, store and element;
  * residual epilogue: rne16(float32(R) + float32(d)), an fp32 add of two 16-bit values and one rounding, as the kernel does it, d the exact
    branch output; R as test_gpu_resid_epilogue draws it (+-8, 1 % outliers of +-500 to 2000).  Exact as well;
  * GELU on the exact family: the input error is zero, so the accepted values are interval16(gelu(pre) -+ (0.75e-7 + 16 U) |pre|): 0.75e-7 |x| is
    half the Abramowitz-Stegun erf error (1.5e-7) times |x|, 16 U |x| the fp32 steps of gelu_exact8 (U = 2^-24) -- _gelu_err of
    tests/test_gpu_kernels.py at input error zero, gelu_exact8 being documented as gelu_exact's operation sequence;
  * Gaussian family (rounded N(0,1) and N(0,1) / sqrt K operands): err = K U sum |a b| + U |pre| (fp32 accumulation of K products in any order,
    one fp32 rounding for the bias add), through the GELU with slope <= 1.13, and interval16: got must lie between rne16(want - err) and
    rne16(want + err), which is exactly "the kernel rounded some value within err of the float64 result".  The exact family is the sharp one (the
    Gaussian interval rejects a one-ulp-off output for 14 % of fp16 elements at K = 768); the Gaussian one has full-mantissa operands;
  * V^T image and split launches: the whole image, key padding included, equals the expectation scattered through vt_index, so every position
    >= S and everything the product does not define is still zero; the split launch equals the two single launches bit for bit.

Worst figures are printed per case (run with -s): |got - want| / err of the raw 16-bit output, which includes the output's own rounding, and
"needed": how far from want, in units of err, the nearest value lies that rounds to got (<= 1 is what the interval asserts)."""
import numpy as np
import pytest
import torch

from prosody_control_french_tts_amd import PceError
from tests import gemm_flat_cases as FC
from tests import gemm_restatement as G

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

EPI = {"plain": 0, "gelu": 1}
_exact, _gauss, _heads = {}, {}, {}


def _problem(shape, bias=True):
    if (shape, bias) not in _exact:
        p = G.ExactProblem(*shape, bias=bias)
        assert p.units_bound() < 2.0 ** 24
        _exact[(shape, bias)] = p
    return _exact[(shape, bias)]


@pytest.fixture(scope="module")
def grid(engine):
    return G.flat_grid(engine.device_info()["compute_units"])


def _run(engine, ops, p, epi, r_bits=None, rows=None):
    """the kernel's output as bit patterns of the operand type (rows: the first rows of the problem alone)"""
    A = p.A if rows is None else p.A[:rows]
    if epi == "resid":
        return engine.selftest_gemm_resid(A, p.B, p.bias, r_bits if rows is None else r_bits[:rows])
    return G.bits(engine.selftest_gemm(A, p.B, p.bias, EPI[epi]), ops)


def _mismatch_report(bad, got, want, shape, grid):
    idx = np.argwhere(bad)
    first = [dict(G.locate(*shape, grid, r, c), got=hex(int(got[r, c])), want=hex(int(want[r, c]) if want is not None else 0)) for r, c in idx[:6]]
    tiles = sorted({(int(r) // 256 * 256, int(c) // 256 * 256) for r, c in idx[:100000]})
    return dict(shape=shape, count=int(bad.sum()), of=int(bad.size), tiles=tiles[:12], first=first)


def _check_exact(engine, ops, p, epi, grid, keep_head=False):
    shape = (p.M, p.N, p.K)
    r_bits = p.resid(ops) if epi == "resid" else None
    got = _run(engine, ops, p, epi, r_bits)
    assert got.shape == (p.M, p.N)
    if epi == "gelu":
        want, err, (lo, hi) = p.gelu_interval(ops)
        bad = ~G.in_interval(got, lo, hi)
        near = np.abs(p.pre) <= 16.0                                     # (beyond: gelu(x) is x or 0 to fp32 and err is the interval's whole width)
        ratio = G.needed_ratio(got[near], want[near], err[near], ops)
        print(f"{ops['name']} {shape} exact GELU: worst needed |got - want| / err = {ratio.max() if ratio.size else 0.0:.3f} over {int(near.sum())} elements")
        assert not bad.any(), _mismatch_report(bad, got, None, shape, grid)
    else:
        want = p.expect(ops, r_bits)
        bad = got != want
        print(f"{ops['name']} {shape} exact {epi}: {int(bad.sum())} of {bad.size} bit patterns differ")
        assert np.array_equal(got, want), _mismatch_report(bad, got, want, shape, grid)
    if keep_head:
        _heads[(shape, epi, ops["name"])] = got[:256].copy()
    return got


@pytest.mark.parametrize("epi", ["plain", "gelu", "resid"])
@pytest.mark.parametrize("case", FC.ROW_MAJOR, ids=FC.case_id)
def test_exact_family_row_major(engine, ops, grid, case, epi):
    """every case x the three row-major epilogues: the whole output bit for bit (GELU: every element inside its interval)"""
    shape = case["shape"]
    if grid == FC.GRID:
        FC.check_class(G.classify(*shape, grid), case["expect"], shape)
    _check_exact(engine, ops, _problem(shape), epi, grid, keep_head=shape in FC.ROW_COUNT_INDEPENDENCE)


@pytest.mark.parametrize("epi", ["plain", "gelu", "resid"])
def test_exact_family_without_a_bias(engine, ops, grid, epi):
    """bias == nullptr: the kernel fills its LDS bias row with zeros"""
    _check_exact(engine, ops, _problem(FC.NO_BIAS, bias=False), epi, grid)


@pytest.mark.parametrize("epi", ["plain", "gelu", "resid"])
@pytest.mark.parametrize("shape", FC.ROW_COUNT_INDEPENDENCE, ids=FC.case_id)
def test_rows_do_not_depend_on_the_row_count(engine, ops, grid, shape, epi):
    """rows [0, 256) of the big exact results are the bits of the same rows run alone with M = 256: the rule of
    test_persistent_256_gemm_is_deterministic_and_row_count_independent where the two runs differ in walk, tiles per workgroup and wait regime"""
    p = _problem(shape)
    key = (shape, epi, ops["name"])
    if key not in _heads:
        _check_exact(engine, ops, p, epi, grid, keep_head=True)
    r_bits = p.resid(ops) if epi == "resid" else None
    small = _run(engine, ops, p, epi, r_bits, rows=256)
    bad = small != _heads[key]
    assert not bad.any(), _mismatch_report(bad, small, _heads[key], (256,) + shape[1:], grid)


@pytest.mark.parametrize("epi", ["plain", "gelu", "resid"])
@pytest.mark.parametrize("shape", FC.GAUSSIAN, ids=FC.case_id)
def test_gaussian_family_row_major(engine, ops, grid, shape, epi):
    """full-mantissa operands: every element inside interval16(want -+ err)"""
    key = (shape, ops["torch"])
    if key not in _gauss:
        _gauss.clear()                                                   # (one problem at a time: float64 matrices of the big case)
        _gauss[key] = G.GaussProblem(ops, *shape)
    g = _gauss[key]
    r_bits = g.resid() if epi == "resid" else None
    got = engine.selftest_gemm_resid(g.A, g.B, g.bias, r_bits) if epi == "resid" else G.bits(engine.selftest_gemm(g.A, g.B, g.bias, EPI[epi]), ops)
    want, err, (lo, hi) = g.interval(epi, r_bits)
    bad = ~G.in_interval(got, lo, hi)
    if epi != "resid":
        raw = np.abs(G.val(got, ops) - want) / err
        print(f"{ops['name']} {shape} Gaussian {epi}: worst |got - want| / err = {raw.max():.2f} (with the output's rounding), needed = "
              f"{G.needed_ratio(got, want, err, ops).max():.4f}")
    print(f"{ops['name']} {shape} Gaussian {epi}: {int(bad.sum())} of {bad.size} elements outside their interval")
    assert not bad.any(), _mismatch_report(bad, got, None, shape, grid)


def _image(want, S, Nv, vt_sp):
    """the V^T image [clips][Nv][vt_sp] a [M][Nv] result belongs in, zero wherever the product defines nothing"""
    M = want.shape[0]
    img = np.zeros(M // S * Nv * vt_sp, dtype=np.uint16)
    img[G.vt_index(np.arange(M)[:, None], np.arange(Nv)[None, :], S, Nv, vt_sp).ravel()] = want.ravel()
    return img.reshape(M // S, Nv, vt_sp)


def _image_report(got, want, S, shape):
    idx = np.argwhere(got != want)
    first = [dict(clip=int(c), column=int(n), position=int(t), row_tile=(int(c) * S + int(t)) // 256 * 256, rel=S - ((int(c) * S + int(t)) // 256 * 256) % S,
                  got=hex(int(got[c, n, t])), want=hex(int(want[c, n, t]))) for c, n, t in idx[:6]]
    return dict(shape=shape, count=int(idx.shape[0]), of=int(got.size), first=first)


@pytest.mark.parametrize("case", FC.VT, ids=FC.case_id)
def test_exact_family_transposed_image_and_split(engine, ops, grid, case):
    S, clips, N, K, split, vt_sp = case["shape"]
    M = S * clips
    if grid == FC.GRID:
        FC.check_class(G.classify(M, N, K, grid, split), case["expect"], case["shape"])
    p = _problem((M, N, K))
    want = p.expect(ops)
    if not split:
        got = G.bits(engine.selftest_gemm(p.A, p.B, p.bias, 2, S, vt_sp), ops)
        img = _image(want, S, N, vt_sp)
        assert got.shape == img.shape
        assert np.array_equal(got, img), _image_report(got, img, S, case["shape"])
        return
    rm, vt = engine.selftest_gemm(p.A, p.B, p.bias, split, S, vt_sp)
    rm, vt = G.bits(rm, ops), G.bits(vt, ops)
    img = _image(want[:, split:], S, N - split, vt_sp)
    assert rm.shape == (M, split) and vt.shape == img.shape
    bad = rm != want[:, :split]
    print(f"{ops['name']} {case['shape']}: row-major part {int(bad.sum())} of {bad.size} differ, image {int((vt != img).sum())} of {img.size}")
    assert not bad.any(), _mismatch_report(bad, rm, want[:, :split], (M, N, K), grid)
    assert np.array_equal(vt, img), _image_report(vt, img, S, case["shape"])
    # ... and the two single launches write the same bits
    assert np.array_equal(rm, G.bits(engine.selftest_gemm(p.A, p.B[:split], p.bias[:split], 0), ops))
    assert np.array_equal(vt, G.bits(engine.selftest_gemm(p.A, p.B[split:], p.bias[split:], 2, S, vt_sp), ops))


def test_launcher_refuses_what_the_kernel_cannot_compute(engine):
    """PCE_E_LIMIT (-5) from launch_gemm_flat's own conditions, before anything is launched"""
    for M, N, K, epi, S, vt_sp in FC.REFUSED:
        A, B, bias = np.ones((M, K), np.float32), np.ones((N, K), np.float32), np.ones(N, np.float32)
        with pytest.raises(PceError, match="status -5"):
            engine.selftest_gemm(A, B, bias, epi, S, vt_sp)
    with pytest.raises(PceError, match="status -5"):
        engine.selftest_gemm_resid(np.ones((300, 64), np.float32), np.ones((384, 64), np.float32), np.ones(384, np.float32), np.zeros((300, 384), np.uint16))
