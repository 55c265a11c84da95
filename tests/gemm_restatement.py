"""Restatements shared by the GEMM tests: 16-bit rounding in float64, the error terms of the tiled kernels' checks, and the persistent
256 x 256 GEMM's host side (csrc/pce_gemm256.inc: FSched, the V^T image, the two-store rule; csrc/pce_whisper_impl.inc: launch_gemm_flat's walk
rule and gemm_flat_offsets_fit).  Nothing here touches the GPU.

Two operand families for the persistent kernel:

  * exact (``ExactProblem``): A holds multiples of 2^-2 in [-4, 4], B multiples of 2^-3 in [-1, 1], the bias nonzero multiples of 2^-4.  Every
    product and every partial sum is a multiple of 2^-5 of magnitude <= 4 K + |bias|, under 2^24 units for every K the cases use, so fp32
    accumulation is exact in ANY order and whatever the MFMA does inside.  The expected output is rne16(A B^T + bias): one bit pattern per
    element, zero tolerance, ties included.  The bias spreads over four scales (1, 8, 64, 256) so that sums past each type's exact range (odd multiples
    of 2^-5 are exact ties from |x| >= 8 in bf16 and >= 64 in fp16, and round up or down beyond twice that) are abundant at every K;
  * Gaussian (``GaussProblem``): test_gpu_kernels.Prob's operands (rounded N(0,1) and N(0,1) / sqrt K), err = K U sum |a b| + U |pre|, accepted
    through ``interval16``.  Full-mantissa operands catch what five-bit operands cannot, but the interval is only as sharp as err: measured on the
    CPU with this scaling, it rejects a one-ulp-off output for 92 % of fp16 and 99 % of bf16 elements at K = 64 (82 % and 97 % at K = 128), but
    only 14-16 % and 72-73 % at K = 768 and 0 % and 15 % at K = 3072 (tests/test_gemm_flat_host.py prints them).  The exact family is the sharp one.

Rounding is monotonic, so "the kernel rounded SOME value within err of the float64 result" is exactly rne16(want - err) <= got <= rne16(want + err)
(``interval16`` / ``in_interval``): the sharpest statement err allows, up to twice as tight as a half_ulp |want| term."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc")

U = 2.0 ** -24


def _dt(ops):
    return getattr(torch, ops["torch"])


def _half_ulp(ops):
    return 2.0 ** -8 if ops["torch"] == "bfloat16" else 2.0 ** -11


def bits(x, ops):
    """float array -> uint16 bit patterns of the operand type (round to nearest even)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_dt(ops)).view(torch.int16).numpy().view(np.uint16)


def val(u, ops):
    """uint16 bit patterns -> float64 values"""
    return torch.from_numpy(np.ascontiguousarray(u).view(np.int16)).view(_dt(ops)).double().numpy()


def r16(x, ops):
    """fp32 values rounded to the operand type and back (what the kernels' (op_t) conversion does)"""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(_dt(ops)).float().numpy()


def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def _gelu_err(pre, pre_err):
    return 1.13 * pre_err + (0.75e-7 + 16 * U) * np.abs(pre)


# ---------------------------------------------------------------------------------------------------------------
# the per-element bounds of the tiled kernels' checks (tests/test_gpu_kernels.py, tests/encoder_walk_restatement.py): derived in the docstring of
# tests/test_gpu_kernels.py
# ---------------------------------------------------------------------------------------------------------------
def bound16(want, err, ops):
    """what a 16-bit output may differ by from a float64 value known to within err: one rounding of the output on top"""
    return err + _half_ulp(ops) * (np.abs(want) + err) + 2.0 ** -24


def bound32(want, err):
    return err + 2 * U * np.abs(want)


def _check16(got_bits, want, err, ops, what):
    """16-bit output against a float64 value known to within err: one rounding of the output on top"""
    got = val(got_bits, ops)
    bound = bound16(want, err, ops)
    bad = np.abs(got - want) > bound
    assert not bad.any(), (what, int(bad.sum()), float(np.max(np.abs(got - want) - bound)))


def _check32(got, want, err, what):
    bound = bound32(want, err)
    bad = np.abs(got.astype(np.float64) - want) > bound
    assert not bad.any(), (what, int(bad.sum()), float(np.max(np.abs(got - want) - bound)))


def gemm_acc(A, B):
    """float64 A B^T of rounded operands (A [m][K], B [N][K]) -> (product, sum |a b|, what fp32 accumulation over K may add: K 2^-24 sum |a b|)"""
    acc, mag = A @ B.T, np.abs(A) @ np.abs(B).T
    return acc, mag, A.shape[1] * U * mag


def gemm_pre(acc, acc_err, bias):
    """the epilogue's input acc + bias and its error (one fp32 addition on top of the accumulation)"""
    pre = acc + np.asarray(bias, dtype=np.float64)
    return pre, acc_err + U * np.abs(pre)


def resid_err(old, acc, err):
    """the fp32 accumulate epilogue old + pre: two more fp32 additions"""
    return err + U * (np.abs(old) + np.abs(acc))


def _ln_ref(v, w, b, eps):
    """float64 LayerNorm of the values the kernel normalised, and the error its fp32 arithmetic allows (per element)"""
    v = v.astype(np.float64)
    d = v.shape[1]
    terms = 4 * -(-d // 256) + 6                                  # sequential adds in a lane + the wave tree
    m = v.mean(axis=1, keepdims=True)
    xc = v - m
    q = (xc ** 2).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(q / d + eps)
    y = xc * inv * w + b
    dm = terms * U * np.abs(v).sum(axis=1, keepdims=True) / d + U * np.abs(m)
    rel_inv = 0.5 * ((terms + 3) * U + d * dm ** 2 / (q + d * eps)) + 3 * U
    err = np.abs(w) * inv * (np.abs(xc) * (rel_inv + 3 * U) + dm) + 2 * U * (np.abs(y) + np.abs(b))
    return y, err


def gelu64(x):
    """_gelu in float64 on all threads (torch's erf; the big cases of the persistent kernel)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * t * (1.0 + torch.special.erf(t / np.sqrt(2.0)))).numpy()


# ---------------------------------------------------------------------------------------------------------------
# one rounding from float64, and acceptance intervals in the 16-bit type's own order
# ---------------------------------------------------------------------------------------------------------------
def _fmt(ops):
    """(explicit mantissa bits, smallest normal exponent, largest finite value)"""
    return (7, -126, (2.0 - 2.0 ** -7) * 2.0 ** 127) if ops["torch"] == "bfloat16" else (10, -14, 65504.0)


def rne16(x64, ops):
    """float64 -> the 16-bit type with ONE round-to-nearest-even (torch's .to() from float64 goes through float32: two roundings).  Returns
    (uint16 bit patterns, float64 values)."""
    x = torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float64))          # (torch: the same steps as numpy's, on all threads)
    p, emin, fmax = _fmt(ops)
    a = x.abs()
    e = torch.frexp(a)[1] - 1                                     # a = 1.f x 2^e (-1 for a == 0: the subnormal quantum below)
    q = torch.ldexp(torch.ones((), dtype=torch.float64), torch.clamp(e, min=emin) - p)         # spacing of the type at a
    v = torch.round(a / q) * q                                    # a / q is exact (q a power of two); round() rounds half to even
    v = torch.where(v > fmax, torch.full((), float("inf"), dtype=torch.float64), v)            # (a carry out of the top binade: 2^(emax + 1))
    v = torch.copysign(v, x)
    b = v.float().to(_dt(ops)).view(torch.int16).numpy().view(np.uint16)                        # v is a value of the type: both conversions are exact
    return b, v.numpy()


def key16(b):
    """uint16 bit patterns -> integers in the order of the values they encode (-0 and +0 both 0; NaNs sort past the infinities)"""
    b = np.asarray(b).astype(np.int32)
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def interval16(lo64, hi64, ops):
    """the closed interval of 16-bit values a kernel may return when it rounds something in [lo64, hi64], as ``key16`` keys"""
    return key16(rne16(lo64, ops)[0]), key16(rne16(hi64, ops)[0])


def in_interval(got_bits, lo, hi):
    k = key16(got_bits)
    return (k >= lo) & (k <= hi)


def cell16(b, ops):
    """the float64 interval that rounds to each bit pattern: midpoints to the two neighbouring values (finite patterns)"""
    b = np.asarray(b, dtype=np.uint16)
    mag = (b & 0x7FFF).astype(np.int32)
    v = val((mag).astype(np.uint16), ops)
    up = val((mag + 1).astype(np.uint16), ops)                    # (past the largest finite value: infinity, cell open upwards)
    dn = np.where(mag > 0, val(np.maximum(mag - 1, 0).astype(np.uint16), ops), -val(np.ones_like(mag).astype(np.uint16), ops))
    lo, hi = 0.5 * (v + dn), 0.5 * (v + up)
    neg = (b & 0x8000) != 0
    return np.where(neg, -hi, lo), np.where(neg, -lo, hi)


def needed_ratio(got_bits, want, err, ops):
    """how far from want, in units of err, the nearest value lies that rounds to got (<= 1 exactly where in_interval holds, up to ties)"""
    lo, hi = cell16(got_bits, ops)
    d = np.maximum(0.0, np.maximum(lo - want, want - hi))
    return np.where(d > 0, d / np.maximum(err, 1e-300), 0.0)


# ---------------------------------------------------------------------------------------------------------------
# the persistent kernel's host side
# ---------------------------------------------------------------------------------------------------------------
F_T, F_K, F_N_MAX = 256, 64, 6144
WALK_SHORT_K, WALK_SHORT_SM, WALK_SM = 1024, 8, 16                # tiles_n == 3 && K <= 1024: sn = 1, sm = 8; default sm = 16


def source_constants():
    """the same constants read out of the two source files (a drift fails tests/test_gemm_flat_host.py on the CPU)"""
    kern = open(os.path.join(CSRC, "pce_gemm256.inc")).read()
    impl = open(os.path.join(CSRC, "pce_whisper_impl.inc")).read()
    m = re.search(r"constexpr int F_T = (\d+), F_K = (\d+), F_THREADS = (\d+);", kern)
    nmax = re.search(r"constexpr int F_N_MAX = (\d+);", kern)
    short = re.search(r"if \(tiles_n == 3 && K <= (\d+)\) \{ P\.sn = 1; sm_want = (\d+); \}\s*else if \(tiles_n == 6\) P\.sn = tiles_n;", impl)
    smw = re.search(r"int sm_want = (\d+);", impl)
    cands = re.search(r"for \(int cand : \{([\d, ]+)\}\) if \(tiles_n % cand == 0\)", impl)
    pad = re.search(r"rows_pad = \(\(tiles_m \+ (\d+)\) / (\d+)\) \* (\d+) \* F_T", impl)
    grid = re.search(r"const int grid = \(\(c->cu_count > 0 \? c->cu_count : (\d+)\) / 8\) \* 8;", impl)
    return dict(F_T=int(m.group(1)), F_K=int(m.group(2)), F_N_MAX=int(nmax.group(1)), short_k=int(short.group(1)), short_sm=int(short.group(2)),
                sm=int(smw.group(1)), sn_candidates=tuple(int(t) for t in cands.group(1).split(",")),
                rows_pad=tuple(int(pad.group(i)) for i in (1, 2, 3)), default_cus=int(grid.group(1)))


def flat_rule(M, N, K):
    """launch_gemm_flat's supertile: (sm, sn, which rule chose it)"""
    tiles_n, tiles_m = N // F_T, -(-M // F_T)
    sn = next((c for c in (4, 3, 2) if tiles_n % c == 0), 1)
    sm_want, rule = WALK_SM, "default"
    if tiles_n == 3 and K <= WALK_SHORT_K:
        sn, sm_want, rule = 1, WALK_SHORT_SM, "three_short"
    elif tiles_n == 6:
        sn, rule = tiles_n, "six"
    return min(tiles_m, sm_want), sn, rule


def flat_grid(compute_units):
    return ((compute_units if compute_units > 0 else 256) // 8) * 8


def flat_walk(M, N, K, grid=256):
    """FSched::init / FSched::tile under launch_gemm_flat's (sm, sn): for every workgroup the ordered list of (m0, n0) it computes.  Entries
    with m0 >= M are padding tiles (loads read zeros, stores are dropped): padding rows of the last supertile, and entries past the end of the
    list (8 per_xcd > total)."""
    sm, sn, _ = flat_rule(M, N, K)
    tiles_n, tiles_m = N // F_T, -(-M // F_T)
    tiles_m_pad = -(-tiles_m // sm) * sm
    total = tiles_m_pad * tiles_n
    per_xcd, wper = (total + 7) >> 3, grid >> 3
    per, n_sn = sm * sn, tiles_n // sn
    out = []
    for wg in range(grid):
        xcd, slot = wg & 7, wg >> 3
        my_tiles = (per_xcd - slot + wper - 1) // wper if per_xcd > slot else 0
        tiles = []
        for it in range(my_tiles):
            lin = xcd * per_xcd + slot + it * wper
            sup, r = divmod(lin, per)
            tiles.append((((sup // n_sn) * sm + r // sn) * F_T, ((sup % n_sn) * sn + r % sn) * F_T))
        out.append(tiles)
    return out


def flat_offsets_fit(M, N, K, ldc, S, vt_sp):
    """gemm_flat_offsets_fit: every byte offset stays below 2^32 (S > 0: the V^T image of N columns; else the row-major output of pitch ldc)"""
    tiles_m = -(-M // F_T)
    rows_pad, lim = ((tiles_m + 15) // 16) * 16 * F_T, 1 << 32
    if rows_pad * K * 2 >= lim or N * K * 2 >= lim:
        return False
    if S > 0:
        return (rows_pad // S + 2) * N * vt_sp * 2 < lim
    return rows_pad * ldc * 2 < lim


def flat_accepts(M, N, K, ldc, S=1, vt_sp=0, vt_n0=0, form="rm"):
    """launch_gemm_flat's conditions (form: 'rm' row-major epilogues, 'vt', 'split')"""
    has_vt, has_rm = form in ("vt", "split"), form != "vt"
    if N % F_T or K % F_K or M < 1 or N > F_N_MAX or (has_vt and (S % 4 or S < F_T)):
        return False
    if form == "split" and (vt_n0 <= 0 or vt_n0 >= N or vt_n0 % F_T):
        return False
    if has_rm and not flat_offsets_fit(M, N, K, ldc, 0, 0):
        return False
    return not has_vt or flat_offsets_fit(M, N - vt_n0, K, 0, S, vt_sp)


def flat_tile_max_offsets(m0, n0, M, N, K, ldc=0, S=0, vt_sp=0, nb0=0):
    """the largest byte offsets the kernel forms for the tile (m0, n0): (A operand, B operand, output).  Output: row-major with pitch ldc, or
    (S > 0) the V^T image of N columns, n0 counted from the first transposed column, positions past the clip's end moved on by one clip."""
    a = ((m0 + F_T - 1) * K + K - 8) * 2 + 15                   # last row of the tile, last byte of the last 16-byte chunk of the last K-step
    b = ((nb0 + n0 + F_T - 1) * K + K - 8) * 2 + 15
    if S <= 0:
        return a, b, ((m0 + F_T - 1) * ldc + n0 + F_T - 1) * 2 + 1
    clip0 = m0 // S
    t_last = m0 - clip0 * S + F_T - 1
    c = ((clip0 * N + n0 + F_T - 1) * vt_sp + min(t_last, S - 1)) * 2 + 1
    if t_last >= S:
        c = max(c, ((clip0 * N + n0 + F_T - 1) * vt_sp + t_last + N * vt_sp - S) * 2 + 1)
    return a, b, c


def classify(M, N, K, grid=256, vt_n0=None):
    """what a shape makes the kernel do: the walk rule, the K loop's wait regime, tiles per workgroup, padding tiles and where they sit in a
    workgroup's stream, and (split launches: vt_n0) neighbouring tiles of different kind"""
    sm, sn, rule = flat_rule(M, N, K)
    walk = flat_walk(M, N, K, grid)
    real = [[m0 < M for m0, _ in t] for t in walk]
    counts = {}
    for t in walk:
        counts[len(t)] = counts.get(len(t), 0) + 1
    tiles_m_pad = -(-(-(-M // F_T)) // sm) * sm
    c = dict(sm=sm, sn=sn, rule=rule, nk=K // F_K, tiles_per_workgroup=counts,
             padding_tiles=sum(r.count(False) for r in real),
             past_the_end=sum(1 for t in walk for m0, _ in t if m0 >= tiles_m_pad * F_T),
             mixed_workgroups=sum(1 for r in real if True in r and False in r),
             padding_then_real=sum(1 for r in real if any(not a and b for a, b in zip(r, r[1:]))),
             real_then_padding=sum(1 for r in real if any(a and not b for a, b in zip(r, r[1:]))))
    if vt_n0 is not None:
        kind = [[n0 >= vt_n0 for _, n0 in t] for t in walk]
        c["rm_then_vt"] = sum(1 for k in kind if any(not a and b for a, b in zip(k, k[1:])))
        c["vt_then_rm"] = sum(1 for k in kind if any(a and not b for a, b in zip(k, k[1:])))
    return c


def vt_index(m, n, S, Nv, vt_sp):
    """element (row m, column n of the transposed part) of the product in the V^T image [clips][Nv][vt_sp]"""
    m, n = np.asarray(m), np.asarray(n)
    return ((m // S) * Nv + n) * vt_sp + m % S


def vt_store_groups(M, S):
    """store_vt / store_vtT: for every row tile that can store and each of its eight 32-position wave groups, (m0, first position t_g in the
    tile's first clip, rel = S - t_g, whether the kernel takes its two-8-byte-store path).  Both forms walk the same eight groups (store_vt:
    hA, wr, g; store_vtT: hB, wc)."""
    out = []
    for m0 in range(0, M, F_T):
        t_tile = m0 - (m0 // S) * S
        for k in range(8):
            t_g = t_tile + 32 * k
            rel = S - t_g
            out.append((m0, t_g, rel, 0 < rel < 32 and (rel & 7) == 4))
    return out


def locate(M, N, K, grid, row, col):
    """where an output element is computed: tile, (workgroup, place in that workgroup's stream, ring parity of the tile's first K-step: the
    stream is one flat sequence of K-steps alternating between the ring's two halves), wave, lane, store and element of the lane's 16-byte
    piece (row-major epilogue)"""
    m0, n0 = row // F_T * F_T, col // F_T * F_T
    where = [(wg, it, (it * (K // F_K)) & 1) for wg, t in enumerate(flat_walk(M, N, K, grid)) for it, mn in enumerate(t) if mn == (m0, n0)]
    r, c = row - m0, col - n0
    hA, wr, i, fr = r // 128, r % 128 // 64, r % 64 // 16, r % 16
    hB, wc, fq, e = c // 128, c % 128 // 32, c % 32 // 8, c % 8
    return dict(row=int(row), col=int(col), tile=(m0, n0), workgroup_it_parity=where, wave=wr * 4 + wc, lane=fq * 16 + fr, store=hB * 8 + hA * 4 + i, element=e)


# ---------------------------------------------------------------------------------------------------------------
# operand families
# ---------------------------------------------------------------------------------------------------------------
def resid_values(M, N, rng):
    """the residual stream as test_gpu_resid_epilogue._problem draws it: around +-8 with 1 % outliers of +-500 to 2000 (float32)"""
    R = rng.standard_normal((M, N), dtype=np.float32) * 8.0
    out = rng.random((M, N)) < 0.01
    R[out] = (np.sign(R[out]) * rng.uniform(500.0, 2000.0, size=int(out.sum()))).astype(np.float32)
    return R


def resid_expected(r_bits, d_val, ops):
    """FEPI_RESID as the kernel computes it: (op_t)((float)R + (float)d), an fp32 add of two 16-bit values, then one rounding.  d_val: the rounded
    branch output's values.  Returns (bits, values)."""
    s = val(r_bits, ops).astype(np.float32) + np.asarray(d_val).astype(np.float32)
    return rne16(s.astype(np.float64), ops)


class ExactProblem:
    """Operands whose every partial sum fp32 holds exactly (see the module's docstring); ``pre`` = A B^T + bias in float64 (exact)."""

    def __init__(self, M, N, K, seed=0, bias=True):
        rng = np.random.default_rng([M, N, K, seed])
        self.M, self.N, self.K = M, N, K
        self.A = (np.clip(np.rint(rng.standard_normal((M, K), dtype=np.float32) * 8.0), -16, 16) / 4.0).astype(np.float32)
        self.B = (np.clip(np.rint(rng.standard_normal((N, K), dtype=np.float32) * 4.0), -8, 8) / 8.0).astype(np.float32)
        scale = rng.choice(np.array([1.0, 8.0, 64.0, 256.0]), size=N)
        b = np.rint(rng.standard_normal(N) * scale * 16.0)
        b[b == 0] = 1.0
        self.bias = (b / 16.0).astype(np.float32) if bias else None
        self.seed = seed
        self._pre = None

    def units_bound(self):
        """the largest magnitude any partial sum can reach, in units of 2^-5 (must stay below 2^24)"""
        worst = np.abs(self.A.astype(np.float64)).sum(axis=1).max() * np.abs(self.B).max()
        return 32.0 * (worst + (0.0 if self.bias is None else float(np.abs(self.bias).max())))

    @property
    def pre(self):
        """A B^T + bias in float64 (kept as float32, which holds these sums exactly: half the memory of the big cases)"""
        if self._pre is None:
            pre = self.A.astype(np.float64) @ self.B.astype(np.float64).T
            if self.bias is not None:
                pre += self.bias.astype(np.float64)
            self._pre = pre.astype(np.float32)
            assert np.array_equal(self._pre, pre)
        return self._pre.astype(np.float64)

    def resid(self, ops):
        """the residual matrix of this problem as bit patterns of the operand type"""
        return bits(resid_values(self.M, self.N, np.random.default_rng([self.M, self.N, self.K, self.seed, 1])), ops)

    def expect(self, ops, r_bits=None):
        """the one bit pattern per element: plain epilogue, or the residual epilogue on r_bits"""
        b, v = rne16(self.pre, ops)
        return b if r_bits is None else resid_expected(r_bits, v, ops)[0]

    def gelu_interval(self, ops):
        """gelu(pre) +- (0.75e-7 + 16 U) |pre|: _gelu_err at input error zero, gelu_exact8 being the tiled kernels' operation sequence"""
        want, err = gelu64(self.pre), _gelu_err(self.pre, 0.0)
        return want, err, interval16(want - err, want + err, ops)


class GaussProblem:
    """test_gpu_kernels.Prob's operands for the persistent kernel, every row kept: float64 product of the ROUNDED operands and its fp32
    accumulation bound err = K U sum |a b| + U |pre|."""

    def __init__(self, ops, M, N, K, seed=0):
        rng = np.random.default_rng([M, N, K, seed, 2])
        self.M, self.N, self.K, self.ops = M, N, K, ops
        self.a = bits(rng.standard_normal((M, K)), ops)
        self.b = bits(rng.standard_normal((N, K)) / np.sqrt(K), ops)
        self.bias = rng.standard_normal(N).astype(np.float32)
        A, B = val(self.a, ops), val(self.b, ops)
        self.A, self.B = A.astype(np.float32), B.astype(np.float32)          # (exact: 16-bit values) what the self-test hooks take
        self.acc = A @ B.T
        self.pre = self.acc + self.bias.astype(np.float64)
        self.err = K * U * (np.abs(A) @ np.abs(B).T) + U * np.abs(self.pre)
        self.seed = seed

    def resid(self):
        return bits(resid_values(self.M, self.N, np.random.default_rng([self.M, self.N, self.K, self.seed, 3])), self.ops)

    def interval(self, epi, r_bits=None):
        """(want, err, (lo, hi)) of an epilogue: 'plain', 'gelu', 'resid' (the residual rule is monotonic in the branch output, so the interval
        of the branch output maps through it endpoint by endpoint; want / err stay those of the branch output)"""
        ops = self.ops
        if epi == "gelu":
            want, err = gelu64(self.pre), _gelu_err(self.pre, self.err)
            return want, err, interval16(want - err, want + err, ops)
        lo, hi = rne16(self.pre - self.err, ops)[1], rne16(self.pre + self.err, ops)[1]
        if epi == "resid":
            return self.pre, self.err, (key16(resid_expected(r_bits, lo, ops)[0]), key16(resid_expected(r_bits, hi, ops)[0]))
        return self.pre, self.err, interval16(self.pre - self.err, self.pre + self.err, ops)
