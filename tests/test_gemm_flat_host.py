"""Host side of the persistent 256 x 256 GEMM's tests (no GPU): the restated tile walk covers every tile once and forms no offset past 2^32, every
case of tests/gemm_flat_cases.py is in the class it claims, the exact operand family is exact, rne16 is one rounding, and the checkers of
tests/test_gpu_gemm_flat.py reject what a subtly wrong kernel would write."""
import numpy as np
import pytest
import torch

from tests import gemm_flat_cases as FC
from tests import gemm_restatement as G

torch.set_num_threads(min(16, torch.get_num_threads()))
TYPES = [dict(torch="float16", name="fp16"), dict(torch="bfloat16", name="bf16")]
HOST_ROWS = 512                                    # rows of a big case the element-wise host checks look at (whole tiles: 0-255 and 256-511)


def test_constants_follow_the_sources():
    c = G.source_constants()
    assert (c["F_T"], c["F_K"], c["F_N_MAX"]) == (G.F_T, G.F_K, G.F_N_MAX)
    assert (c["short_k"], c["short_sm"], c["sm"]) == (G.WALK_SHORT_K, G.WALK_SHORT_SM, G.WALK_SM) == (1024, 8, 16)
    assert c["sn_candidates"] == (4, 3, 2) and c["rows_pad"] == (15, 16, 16) and c["default_cus"] == FC.GRID == 256
    assert G.flat_grid(256) == 256 and G.flat_grid(0) == 256 and G.flat_grid(255) == 248


def test_walk_visits_every_real_tile_exactly_once():
    for M in list(range(1, 701, 37)) + [2100, 4097, 8448, 23040, 96000]:
        for N in range(256, G.F_N_MAX + 1, 256):
            for K in (64, 1088):
                walk = G.flat_walk(M, N, K, FC.GRID)
                real = [t for w in walk for t in w if t[0] < M]
                want = {(m0, n0) for m0 in range(0, M, 256) for n0 in range(0, N, 256)}
                assert len(real) == len(want) and set(real) == want, (M, N, K)
                assert all(0 <= n0 < N and m0 % 256 == 0 and n0 % 256 == 0 for w in walk for m0, n0 in w), (M, N, K)


@pytest.mark.parametrize("K", [768, 3072])
def test_no_offset_reaches_2_to_the_32_where_the_launcher_accepts(K):
    """up to the largest row count gemm_flat_offsets_fit lets through, for the row-major output and the V^T image: not only the tiles that can store
    (m0 < M) but every walk entry stays below 2^32, so a padding tile's offsets never wrap back into the matrices"""
    lim = 1 << 32
    top = (lim // (K * 2) // 4096) * 4096                       # the first rows_pad that is refused, or the last accepted one
    for N, ldc, S, vt_sp in [(768, 768, 0, 0), (256, 256, 0, 0), (768, 0, 1500, 1536), (256, 0, 256, 256)]:
        fit = lambda m: G.flat_offsets_fit(m, N, K, ldc, S, vt_sp)
        lo, hi = 1, top + 4096                                     # bisect the largest accepted M (acceptance is monotonic in M)
        assert fit(lo) and not fit(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fit(mid) else (lo, mid)
        for M in (lo, lo - 255, lo - 4096, lo // 2 + 1, 23040, 4097, 300, 1):
            if M < 1 or (S and M % S):
                M = max(S, M // max(S, 1) * max(S, 1))
            assert fit(M)
            worst = 0
            for w in G.flat_walk(M, N, K, FC.GRID):
                for m0, n0 in w:
                    worst = max(worst, *G.flat_tile_max_offsets(m0, n0, M, N, K, ldc, S, vt_sp))
            assert worst < lim, (M, N, K, S, worst)
        assert not fit(hi)


def test_cases_are_in_the_classes_they_claim():
    seen_counts, rules, nks = set(), set(), set()
    for case in FC.ROW_MAJOR:
        M, N, K = case["shape"]
        assert G.flat_accepts(M, N, K, N)
        c = G.classify(M, N, K, FC.GRID)
        FC.check_class(c, case["expect"], case["shape"])
        seen_counts |= set(c["tiles_per_workgroup"]); rules.add((c["rule"], c["sn"])); nks.add(min(c["nk"], 4))
    assert seen_counts == {0, 1, 2, 3} and nks == {1, 2, 3, 4}
    assert {r for r, _ in rules} == {"default", "three_short", "six"} and {sn for r, sn in rules if r == "default"} == {4, 3, 2, 1}
    # the three wait regimes that follow an epilogue: second tiles with nk >= 3 (after_stores 1, 2, 0), nk == 2 (1, 2) and nk == 1 (plain counts)
    second = {min(G.classify(*c["shape"])["nk"], 3) for c in FC.ROW_MAJOR if max(G.classify(*c["shape"])["tiles_per_workgroup"]) >= 2}
    assert second == {1, 2, 3}
    assert all(s in [c["shape"] for c in FC.ROW_MAJOR] for s in FC.GAUSSIAN + FC.ROW_COUNT_INDEPENDENCE + [FC.NO_BIAS])
    for M, N, K in FC.ROW_COUNT_INDEPENDENCE:                       # ... differ from the 256-row run in walk, tiles per workgroup and wait regime
        big, small = G.classify(M, N, K), G.classify(256, N, K)
        assert (big["sm"], max(big["tiles_per_workgroup"])) != (small["sm"], max(small["tiles_per_workgroup"])) and max(small["tiles_per_workgroup"]) == 1


def test_vt_cases_meet_every_store_path():
    all_rels = set()
    for case in FC.VT:
        S, clips, N, K, split, vt_sp = case["shape"]
        M = S * clips
        assert G.flat_accepts(M, N, K, split or 0, S, vt_sp, split or 0, "split" if split else "vt")
        if split:
            assert G.flat_accepts(M, split, K, split) and G.flat_accepts(M, N - split, K, 0, S, vt_sp, 0, "vt")     # the two single launches
        FC.check_class(G.classify(M, N, K, FC.GRID, split), case["expect"], case["shape"])
        groups = G.vt_store_groups(M, S)
        rels = {rel for _, _, rel, _ in groups if 0 < rel < 32}
        assert rels == set(case["rels"]), (case["shape"], sorted(rels))
        assert all(two == (rel in (4, 12, 20, 28)) for _, _, rel, two in groups)
        assert any(rel <= 0 for _, _, rel, _ in groups) == (S != 256)                   # wave groups wholly past the clip's end
        assert vt_sp >= S and all((m0 + 255) // S - m0 // S <= 1 for m0, _, _, _ in groups)        # a tile spans at most one clip boundary
        all_rels |= rels
    assert all_rels == {4, 8, 12, 16, 20, 24, 28}
    for M, N, K, epi, S, vt_sp in FC.REFUSED:
        form = "rm" if epi < 2 else "vt" if epi == 2 else "split"
        assert not G.flat_accepts(M, N, K, N if epi < 2 else epi, S, vt_sp, epi if epi >= 256 else 0, form), (M, N, K, epi)


def test_vt_index_is_the_image_layout():
    S, Nv, vt_sp, clips = 260, 512, 272, 3
    img = np.full(clips * Nv * vt_sp, -1, dtype=np.int64)
    m, n = np.meshgrid(np.arange(S * clips), np.arange(Nv), indexing="ij")
    idx = G.vt_index(m, n, S, Nv, vt_sp)
    assert np.unique(idx).size == idx.size
    img[idx.ravel()] = (m * Nv + n).ravel()
    img = img.reshape(clips, Nv, vt_sp)
    assert (img[:, :, S:] == -1).all() and img[2, 7, 11] == (2 * S + 11) * Nv + 7


# ---------------------------------------------------------------------------------------------------------------
# rne16 and the exact family
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ops", TYPES, ids=lambda o: o["name"])
def test_rne16_is_torchs_rounding_from_float32_and_one_rounding_from_float64(ops):
    rng = np.random.default_rng(1)
    p, emin, fmax = G._fmt(ops)
    x = np.concatenate([rng.standard_normal(200000) * np.exp2(rng.integers(-30, 17, 200000)), [0.0, -0.0, fmax, -fmax]]).astype(np.float32)
    # exact ties: odd multiples of half a spacing, in normal binades and among the subnormals; both ends of the exact-integer range
    n = rng.integers(2 ** p, 2 ** (p + 1), 20000) * 2 + 1
    ties = np.concatenate([n * np.exp2(e - p - 1) for e in (-8, 0, 3, 6, 11)] + [(np.arange(64) * 2 + 1) * np.exp2(emin - p - 1)])
    top = 2 ** (p + 1)
    ints = np.r_[np.arange(top - 8, top + 9), -np.arange(top - 8, top + 9)].astype(np.float64)
    half_top = np.exp2(np.floor(np.log2(fmax)) - p - 1)                                         # half a spacing in the top binade
    edge = np.array([fmax + half_top * (1.0 - 2.0 ** -10), fmax + half_top, -fmax - half_top, 2.0 ** -149])      # the last finite cell, overflow on the tie
    for v in (x.astype(np.float64), ties, -ties, ints, edge):
        v32 = v.astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), v)                                        # (so that torch's conversion is one rounding too)
        b, back = G.rne16(v, ops)
        assert np.array_equal(b, G.bits(v32, ops)) and np.array_equal(G.val(b, ops), back)
    b, _ = G.rne16(ties, ops)
    assert (b & 1 == 0).all()                                                                    # ties went to even
    # above a tie by less than float32 resolves: one rounding goes up, torch's two roundings (float64 -> float32 -> 16 bits) land on the even value
    y = np.array([1.0 + 2.0 ** -(p + 1) + 2.0 ** -40])
    assert G.rne16(y, ops)[1][0] == 1.0 + 2.0 ** -p and torch.from_numpy(y).to(G._dt(ops)).double().item() == 1.0
    # key16 orders bit patterns as values; an interval is closed
    s = np.sort(np.concatenate([x.astype(np.float64), -ties]))
    assert (np.diff(G.key16(G.rne16(s, ops)[0])) >= 0).all()
    lo, hi = G.interval16(np.array([1.0, -2.0]), np.array([1.0, -1.0]), ops)
    assert G.in_interval(G.bits(np.array([1.0, -1.5]), ops), lo, hi).all()
    assert not G.in_interval(G.bits(np.array([1.0 + 2.0 ** -p, -1.0 + 2.0 ** -(p + 1)]), ops), lo, hi).any()
    lo_c, hi_c = G.cell16(G.bits(np.array([1.0, -1.0, 0.0]), ops), ops)
    assert lo_c[0] == 1.0 - 2.0 ** -(p + 2) and hi_c[0] == 1.0 + 2.0 ** -(p + 1) and lo_c[1] == -hi_c[0] and hi_c[2] == -lo_c[2] > 0


_exact = {}


def _exact_head(shape, bias=True):
    """the exact problem of a case, its float64 result kept for the first HOST_ROWS rows only"""
    if (shape, bias) not in _exact:
        p = G.ExactProblem(*shape, bias=bias)
        rows = min(p.M, HOST_ROWS)
        pre = p.A[:rows].astype(np.float64) @ p.B.astype(np.float64).T + (p.bias.astype(np.float64) if bias else 0.0)
        _exact[(shape, bias)] = (p, pre)
    return _exact[(shape, bias)]


def test_exact_family_is_exact_and_rounds_in_abundance():
    shapes = [c["shape"] for c in FC.ROW_MAJOR] + [(c["shape"][0] * c["shape"][1], c["shape"][2], c["shape"][3]) for c in FC.VT]
    for shape in shapes:
        p, pre = _exact_head(shape)
        assert p.units_bound() < 2.0 ** 24, shape                                  # fp32 holds every partial sum, in any order
        assert np.array_equal(np.rint(pre * 32.0), pre * 32.0) and np.abs(pre).max() * 32.0 < 2.0 ** 24
        assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
        for t in (p.A, p.B):                                                        # operands are values of both 16-bit types (the bias is fp32)
            for ops in TYPES:
                assert np.array_equal(G.r16(t, ops), t)
        assert (p.bias != 0).all() and np.array_equal(np.rint(p.bias * 16.0), p.bias * 16.0)
        assert np.abs(p.A).max() == 4.0 and np.abs(p.B).max() == 1.0 or p.M * p.K < 4096       # full-range values occur
        for ops in TYPES:
            v = G.rne16(pre, ops)[1]
            inexact = v != pre
            spacing = np.exp2(np.floor(np.log2(np.maximum(np.abs(pre), 2.0 ** -14))) - G._fmt(ops)[0])
            tie = inexact & (np.abs(v - pre) == 0.5 * spacing)
            # half of the columns carry a bias of scale 64 or 256, and half of all sums are odd multiples of 2^-5: both kinds by the percent at least
            assert tie.mean() >= 0.01 and (inexact & ~tie).mean() >= 0.01, (shape, ops["name"], tie.mean(), (inexact & ~tie).mean())
    p, pre = _exact_head(FC.NO_BIAS, bias=False)
    assert p.bias is None and p.units_bound() < 2.0 ** 24


def test_residual_restatement_is_the_existing_tests_rule():
    """gemm_restatement.resid_expected against test_gpu_resid_epilogue's reference on that test's own inputs, fed a torch-computed branch output"""
    from tests import test_gpu_resid_epilogue as TR
    A, B, bias, R = TR._problem((300, 768, 128))
    for ops in TYPES:
        dtype = G._dt(ops)
        a, b = torch.from_numpy(A).to(dtype).float(), torch.from_numpy(B).to(dtype).float()
        delta = (a @ b.T + torch.from_numpy(bias)).to(dtype).float().numpy()
        theirs = TR._bits(TR._f32(TR._bits(R, dtype), dtype) + delta, dtype)
        mine, _ = G.resid_expected(G.bits(R, ops), delta, ops)
        assert np.array_equal(mine, theirs)
        assert (np.abs(G.val(G.bits(R, ops), ops)) > 400).mean() > 0.005            # the outliers are there


# ---------------------------------------------------------------------------------------------------------------
# checker sensitivity: what a subtly wrong kernel would write, applied on the CPU
# ---------------------------------------------------------------------------------------------------------------
def _kstep(A, B, ks):
    return A[:, ks * 64:(ks + 1) * 64].astype(np.float64) @ B[:, ks * 64:(ks + 1) * 64].astype(np.float64).T


def _ksteps_to_try(nk):
    return range(nk) if nk <= 3 else (0, nk - 1)


@pytest.mark.parametrize("ops", TYPES, ids=lambda o: o["name"])
def test_exact_checker_rejects_every_mutation(ops):
    for shape in [(300, 768, 192), (2100, 768, 768), (2100, 768, 3072), (8448, 2048, 128), (1, 256, 64), (1300, 6144, 64)]:
        p, pre = _exact_head(shape)
        rows, N, nk = pre.shape[0], p.N, p.K // 64
        want = G.rne16(pre, ops)[0]
        r_bits = p.resid(ops)[:rows]
        want_r = G.resid_expected(r_bits, G.val(want, ops), ops)[0]
        gw, ge = G._gelu(pre), G._gelu_err(pre, 0.0)
        glo, ghi = G.interval16(gw - ge, gw + ge, ops)
        assert G.in_interval(G.rne16(gw, ops)[0], glo, ghi).all()
        # one output one ulp off, either way: the plain and residual forms compare bit patterns, so every element is rejected; the GELU interval
        # rejects it wherever it is one value wide
        for d in (1, -1):
            for w in (want, want_r):
                assert ((w.astype(np.int32) + d).astype(np.uint16) != w).all()
            g_off = (G.rne16(gw, ops)[0].astype(np.int32) + d).astype(np.uint16)
            assert (~G.in_interval(g_off, glo, ghi))[glo == ghi].all() and (glo == ghi).any()
        # two 8-column pieces of a row swapped / a 16-byte piece left unwritten (zeros): rejected for EVERY piece, in the plain, residual and GELU checks
        pieces = want.reshape(rows, N // 8, 8)
        assert (pieces != 0).any(axis=2).all(), shape                                               # no expected piece is all zero bits
        assert (pieces != np.roll(pieces, 1, axis=1)).any(axis=2).all(), shape                     # no piece equals its left neighbour
        # (GELU: an unwritten piece passes only where all eight inputs are zero or so negative that gelu is zero to within its bound)
        zero_ok = G.in_interval(np.zeros_like(want), glo, ghi).reshape(rows, N // 8, 8).all(axis=2)
        assert (zero_ok <= ((pre < -4.0) | (pre == 0.0)).reshape(rows, N // 8, 8).all(axis=2)).all() and zero_ok.mean() < 0.02, (shape, zero_ok.mean())
        assert (want_r.reshape(rows, N // 8, 8) != r_bits.reshape(rows, N // 8, 8)).any(axis=2).all()      # residual form: an unwritten piece keeps R
        # the bias shifted by one column
        shifted = G.rne16(pre - p.bias.astype(np.float64) + np.roll(p.bias, 1).astype(np.float64), ops)[0]
        assert (shifted != want).mean() > 0.5
        # the store-data hazard: the first dword of a 16-byte piece left as the bits of an fp32 sum (the next row block's: 16 rows down)
        f32 = np.roll(pre, -16, axis=0).astype(np.float32).view(np.uint32).reshape(rows, N // 8, 8)[:, :, 0]
        hazard = pieces.copy()
        hazard[:, :, 0], hazard[:, :, 1] = (f32 & 0xFFFF).astype(np.uint16), (f32 >> 16).astype(np.uint16)
        assert (hazard != pieces).any(axis=2).all(), shape
        # a 64-deep K-step dropped or counted twice: >= 95 % of the elements change (its exact contribution is zero for about 2 % at K = 64)
        for ks in _ksteps_to_try(nk):
            step = _kstep(p.A[:rows], p.B, ks)
            for sign in (-1.0, 1.0):
                mut = G.rne16(pre + sign * step, ops)[0]
                frac = (mut != want).mean()
                assert frac >= 0.95, (shape, ks, sign, frac)
                # (GELU: where both inputs are positive, where the function does not flatten them to zero)
                pos = (pre > 0) & (pre + sign * step > 0)
                gfrac = 1.0 - G.in_interval(G.rne16(G._gelu(pre + sign * step), ops)[0], glo, ghi)[pos].mean()
                assert gfrac >= 0.95, (shape, ks, sign, gfrac)


@pytest.mark.parametrize("ops", TYPES, ids=lambda o: o["name"])
def test_gaussian_checker_accepts_fp32_sums_and_rejects_the_mutations(ops):
    for shape in FC.GAUSSIAN:
        M, N, K = shape
        rows = min(M, HOST_ROWS)
        g = G.GaussProblem(ops, rows, N, K)
        # a kernel's result: fp32 sums, K-step by K-step, rounded once
        acc32 = np.zeros((rows, N), dtype=np.float32)
        for ks in range(K // 64):
            acc32 += g.A[:, ks * 64:(ks + 1) * 64] @ g.B[:, ks * 64:(ks + 1) * 64].T
        out32 = acc32 + g.bias
        r_bits = g.resid()
        for epi in ("plain", "gelu", "resid"):
            want, err, (lo, hi) = g.interval(epi, r_bits)
            model = {"plain": lambda x: G.bits(x, ops), "gelu": lambda x: G.rne16(G._gelu(x.astype(np.float64)), ops)[0],
                     "resid": lambda x: G.resid_expected(r_bits, G.r16(x, ops), ops)[0]}[epi]
            got = model(out32)
            assert G.in_interval(got, lo, hi).all(), (shape, epi)
            if epi != "resid":
                assert (G.needed_ratio(got, want, err, ops) <= 1.0).all()
            for ks in _ksteps_to_try(K // 64):
                step = _kstep(g.A, g.B, ks).astype(np.float32)
                for sign in (-1.0, 1.0):
                    frac = 1.0 - G.in_interval(model(out32 + np.float32(sign) * step), lo, hi).mean()
                    if epi == "plain":
                        print(f"{ops['name']} {shape}: K-step {ks} {'dropped' if sign < 0 else 'twice'}: {100 * frac:.2f} % rejected")
                        assert frac >= 0.90, (shape, epi, ks, sign, frac)
                    else:
                        assert frac >= 0.5, (shape, epi, ks, sign, frac)             # (GELU flattens the negative half; the residual's outliers absorb the step)
            if epi != "plain":
                continue
            pieces = got.reshape(rows, N // 8, 8)
            swapped = np.roll(pieces, 1, axis=1).reshape(rows, N)
            assert not G.in_interval(swapped, lo, hi).reshape(rows, N // 8, 8).all(axis=2).any()
            assert not G.in_interval(np.zeros_like(got), lo, hi).reshape(rows, N // 8, 8).all(axis=2).any()
            assert 1.0 - G.in_interval(G.bits(acc32 + np.roll(g.bias, 1), ops), lo, hi).mean() > 0.9
            f32 = np.roll(out32, -16, axis=0).view(np.uint32).reshape(rows, N // 8, 8)[:, :, 0]
            hazard = pieces.copy()
            hazard[:, :, 0], hazard[:, :, 1] = (f32 & 0xFFFF).astype(np.uint16), (f32 >> 16).astype(np.uint16)
            assert not G.in_interval(hazard.reshape(rows, N), lo, hi).reshape(rows, N // 8, 8).all(axis=2).any()
            for d in (1, -1):
                off = (got.astype(np.int32) + d).astype(np.uint16)
                print(f"{ops['name']} {shape}: one ulp {'up' if d > 0 else 'down'} rejected for {100 * (1.0 - G.in_interval(off, lo, hi).mean()):.1f} % of the elements")
