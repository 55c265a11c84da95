"""The three kernels between the decoder's cross-attention queries and the DTW of the forced alignment -- k_align_scores, k_align_colnorm,
k_align_cost<7> / <0> -- stage by stage against float64, through the launches and the padding code of pce_whisper_align_run
(pce_selftest_align_matrix).  The reference is tests/align_restatement.py (pinned to find_alignment's torch pieces by tests/test_align_host.py); every
element of every output is checked, and each stage's reference runs on the DEVICE's previous stage, so the conditioning of a later stage (a small
std) never enters a tolerance.  U = 2^-24 below.

Stage 1, w_soft against the softmax of the rounded operands in float64: |got - want| <= want x rel + 2^-120, per element, derived and not fitted:
  * a score is 64 exact 16-bit products accumulated in fp32 by two MFMAs and one multiplication by the scale: 65 roundings against
    mag = sum_e |q_e k_e| x scale; the subtraction of the row maximum rounds once more, U |s - max| (the rescales' exponents sum to the same
    difference).  With delta = max over the row of 65 U mag + U |s - max|, a weight moves by at most e^(2 delta) (numerator up, denominator down);
  * the exponential is within EPS_EXP relative (tests/test_gpu_attention.py's figure for the same fp32 instruction): once in the numerator, and on
    the path of a term of the denominator once for itself, once per later tile of its wave (the online rescale) and once in the four-wave merge:
    tiles + 1 exponentials, tiles = ceil(F / 64) being the tiles of ANY wave's walk (s0 += 64) -- the worst case, a rescale by e^0 is exact;
  * fp32 roundings on a term's path to the denominator: 4 DPP levels and the addition into the running sum in its own tile, a multiplication and an
    addition per later tile, a multiplication and 4 additions in the merge: 2 tiles + 8;
  * the final division, correctly rounded (the library is built without fast-math): one more.
  rel = e^(2 delta) (1 + EPS_EXP) (1 + U) / ((1 - EPS_EXP)^(tiles + 1) (1 - U)^(2 tiles + 8)) - 1.  2^-120 covers exponentials and quotients below the
  smallest normal number (flushed or denormal: at most 2^-126 each, the denominator being >= 1 - rel).  A row's sum over s < F is 1 within the sum
  of its elements' bounds.  F = 1 returns exactly 1.0.

Stage 2, w_norm against float64 norm(w_soft of the device), per column of T non-negative values v with mean m, deviations a = v - m, q = sum a^2,
sd = sqrt(q / T), every operation of k_align_colnorm rounding once (no contraction: -ffp-contract=off):
  * the sequential sum of T non-negative terms and the division by T: e_m = T U m;
  * a subtraction: e_a = e_m + U (|a| + e_m);
  * T squares, their sequential sum and the division by T: e_q = sum (2 |a| e_a + e_a^2) + (T + 1) U q, then sqrtf (2 U allowed):
    r_sd = (e_q / q) (1 + e_q / q) / 2 + 2 U;
  * the subtraction again and the division: |got - want| <= (e_a + (|a| + e_a) (r_sd + U)) / (sd (1 - r_sd)).
  Both paths of the kernel (registers for T <= 64, the loop above) add in the same order, and the library is built without contraction or
  fast-math: test_colnorm_paths_share_their_bytes also holds a T = 64 and a T = 65 clip, one on each path, to the sequential fp32 restatement
  (AL.norm_f32) bit for bit.

Stage 3, cost: bit-exact against the fp32 variant of the restatement on the device's w_norm (a median is a selection; the heads are added in
ascending order in fp32, one correctly rounded fp32 division, widened and negated).

Nothing else is written: w_soft and cost go in filled with a value no result can take (-777: a weight is in [0, 1], |a normalised weight| <=
sqrt(T - 1) < 10 and so is a cost) and must keep it, bit for bit, wherever t >= T, s >= F or a cost row is outside [0, T - sot_len - 1).  w_norm is
the same device buffer after the in-place normalisation (include/pce.h says so): it goes in filled with -555 and must come back with w_soft's -777
in those positions, none of its own prefill surviving.  q rows past a clip's tokens and key rows past its frames hold +-60000 and would show in
any weight.

The F = 1 clip's single column is constant, so its normalisation is 0 / 0 in the reference too: stages 2 and 3 are checked there only for WHERE they
write.  Every other column of every case has a non-zero reference std: asserted in every check on the array stage 2's reference runs on, the
device's own w_soft.

Worst |got - want| / bound seen on an MI355X with these constants (fp16-resid16 runs the fp16 build's kernels):
    stage               fp16-resid16   fp16       bf16
    1  w_soft           1.01e-3        1.01e-3    1.25e-3
    1  w_soft, EPS_EXP = 0 (printed, not asserted)
                        0.0334         0.0334     0.0334
    1  row sums         6.2e-5         6.2e-5     5.3e-5
    2  w_norm           0.505          0.505      0.435
    2  w_norm at T = 64 and T = 65 against AL.norm_f32: identical bits
    3  cost             identical bits in every case
Stage 1 sits three orders below its bound because EPS_EXP is the attention probe's resolution, not the exponential's error (see that file).  The
tests therefore also print the ratio against the same bound with EPS_EXP = 0; a change that moves that figure from 0.03 towards 1 deserves a look
even while the asserted bound holds."""
import numpy as np
import pytest

from prosody_control_french_tts_amd import PceError
from tests import align_restatement as AL
from tests.test_gpu_attention import EPS_EXP
from tests.test_gpu_kernels import bits, val

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -120
BIG = 60000.0                   # finite in both 16-bit types: what must never be read
SENT = -777.0                   # what no launch may overwrite outside a clip's own rows and columns
SENT_NORM = -555.0              # w_norm goes in with another value: it comes back as the in-place buffer, w_soft's value where nothing is written
HEADS6, SEL4 = 6, (5, 0, 3, 3)  # non-ascending from a non-zero head, one head twice


def _big(shape, ops):
    n = int(np.prod(shape))
    return bits(np.where((np.arange(n) * 7 // 3) % 2 == 0, BIG, -BIG).reshape(shape), ops)


def _ceil(x, m):
    return -(-x // m) * m


class Batch:
    """n clips of t_len tokens and f_len frames: q [n][T_pad][d] and k [n][k_rows][d] as bit patterns, +-60000 in every query row >= T and every
    key row >= F.  q and k are drawn per clip from (seed, T, F) so that a clip can be rebuilt inside another batch."""

    def __init__(self, ops, H, t_len, f_len, heads_sel, seed, sot_len=3, width=7, qk_scale=1.0, split=0, sigma=1.0, k_rows=None):
        self.ops, self.H, self.d, self.n = ops, H, H * 64, len(t_len)
        self.t_len, self.f_len, self.heads_sel = list(t_len), list(f_len), list(heads_sel)
        self.sot_len, self.width, self.qk_scale, self.split = sot_len, width, qk_scale, split
        self.T_pad, self.F_pad, self.N_max = _ceil(max(t_len), 16), _ceil(max(f_len), 64), max(t_len) - sot_len - 1
        self.k_rows = min(max(f_len) + 2, 1500) if k_rows is None else k_rows
        self.scale = float(np.float32(0.125) * np.float32(qk_scale))          # what the kernel multiplies by
        self.q, self.k = _big((self.n, self.T_pad, self.d), ops), _big((self.n, self.k_rows, self.d), ops)
        for i, (T, F) in enumerate(zip(t_len, f_len)):
            rng = np.random.default_rng([seed, T, F])
            self.q[i, :T] = bits(rng.standard_normal((T, self.d)) * sigma, ops)
            self.k[i, :F] = bits(rng.standard_normal((F, self.d)) * sigma, ops)

    def run(self, eng):
        n_sel = len(self.heads_sel)
        w_soft = np.full((self.n, n_sel, self.T_pad, self.F_pad), SENT, np.float32)
        w_norm = np.full(w_soft.shape, SENT_NORM, np.float32)
        cost = np.full((self.n, self.N_max, self.F_pad), SENT, np.float64)
        q0, k0 = self.q.copy(), self.k.copy()
        eng.selftest_align_matrix(self.H, self.q, self.k, self.t_len, self.f_len, self.heads_sel, w_soft, w_norm, cost, split=self.split,
                                  sot_len=self.sot_len, medfilt_width=self.width, qk_scale=self.qk_scale)
        assert np.array_equal(q0, self.q) and np.array_equal(k0, self.k)
        return w_soft, w_norm, cost


RATIOS = {}


def _ratio(stage, ops, what, diff, bound, asserted=True):
    r = float(np.max(diff / bound))
    key = (stage, ops["name"])
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"align-ratio {stage} {ops['name']} {what}: {r:.3e} (worst so far {RATIOS[key]:.3e})")
    bad = diff > bound
    assert not asserted or not bad.any(), (stage, ops["name"], what, int(bad.sum()), r, np.argwhere(bad)[:4].tolist())


def _soft_rel(mag, s, F, eps_exp=EPS_EXP):
    """relative bound of a weight, [n_sel][T][1] (see the module docstring)"""
    tiles = -(-F // 64)
    delta = (65 * U * mag + U * np.abs(s - s.max(axis=-1, keepdims=True))).max(axis=-1, keepdims=True)
    return np.exp(2 * delta) * (1 + eps_exp) * (1 + U) / ((1 - eps_exp) ** (tiles + 1) * (1 - U) ** (2 * tiles + 8)) - 1


def _norm_bound(v):
    """v [n_sel][T][F] float64 (the device's w_soft) -> absolute bound of k_align_colnorm's output against AL.norm(v)"""
    T = v.shape[1]
    m = v.mean(axis=1, keepdims=True)
    a = np.abs(v - m)
    q = (a * a).sum(axis=1, keepdims=True)
    sd = np.sqrt(q / T)
    e_m = T * U * m
    e_a = e_m + U * (a + e_m)
    e_q = (2 * a * e_a + e_a * e_a).sum(axis=1, keepdims=True) + (T + 1) * U * q
    r_sd = (e_q / q) * (1 + e_q / q) / 2 + 2 * U
    return (e_a + (a + e_a) * (r_sd + U)) / (sd * (1 - r_sd))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(eng, b, what):
    """One call -> every element of the three outputs of every clip; returns the outputs."""
    ops = b.ops
    w_soft, w_norm, cost = b.run(eng)
    sent32, sent64 = np.float32(SENT), np.float64(SENT)
    for i, (T, F) in enumerate(zip(b.t_len, b.f_len)):
        N = T - b.sot_len - 1
        tag = (what, i, T, F)
        # ---- nothing else is written
        for w in (w_soft, w_norm):
            assert np.all(w[i, :, T:, :] == sent32) and np.all(w[i, :, :, F:] == sent32), tag
        assert not np.any(w_norm[i] == np.float32(SENT_NORM)), tag
        assert np.all(cost[i, N:, :] == sent64) and np.all(cost[i, :, F:] == sent64), tag
        got1, got2, got3 = w_soft[i, :, :T, :F], w_norm[i, :, :T, :F], cost[i, :N, :F]
        # ---- stage 1
        qv, kv = val(b.q[i, :T], ops), val(b.k[i, :F], ops)
        want1, mag, s = AL.soft(qv, kv, b.heads_sel, b.scale)
        assert np.isfinite(got1).all() and np.all(got1 >= 0), tag
        bound1 = want1 * _soft_rel(mag, s, F) + TINY
        _ratio("w_soft", ops, tag, np.abs(got1 - want1), bound1)
        _ratio("w_soft, EPS_EXP = 0 (printed only)", ops, tag, np.abs(got1 - want1), want1 * _soft_rel(mag, s, F, 0.0) + TINY, asserted=False)
        _ratio("row sums", ops, tag, np.abs(got1.astype(np.float64).sum(axis=-1) - 1.0), bound1.sum(axis=-1))
        if F == 1:
            assert np.all(got1 == np.float32(1.0)), tag
            # 0 / 0 in the reference as well: only where stages 2 and 3 write
            assert np.all(got2.view(np.uint32) != sent32.view(np.uint32)) and np.all(got3.view(np.uint64) != sent64.view(np.uint64)), tag
            continue
        # ---- stage 2, on the device's own w_soft
        v = got1.astype(np.float64)
        assert np.all(v.std(axis=1) > 0), tag                             # stage 2's reference input: no column but the F = 1 clip's is constant
        assert np.isfinite(got2).all(), tag
        _ratio("w_norm", ops, tag, np.abs(got2 - AL.norm(v)), _norm_bound(v))
        # ---- stage 3, on the device's own w_norm: bit for bit
        want3 = AL.cost_f32(got2, b.sot_len, b.width)
        assert _same_bits(got3, want3), (tag, int((got3 != want3).sum()), np.argwhere(got3 != want3)[:4].tolist())
    return w_soft, w_norm, cost


def _clip(outs, b, i):
    """clip i's own region of the three outputs"""
    T, F, N = b.t_len[i], b.f_len[i], b.t_len[i] - b.sot_len - 1
    return outs[0][i, :, :T, :F], outs[1][i, :, :T, :F], outs[2][i, :N, :F]


# F along the wave (16 keys each), tile (64) and column-block (256) edges, mixed so that the longest clip sizes the grid; T ragged over its own edges
F_BATCHES = [((1, 257, 16, 65), (5, 96, 17, 33)), ((3, 63, 256, 17), (64, 15, 65, 16)), ((4, 127, 15, 64), (33, 5, 96, 17)), ((129, 255, 1500), (16, 65, 20))]


@pytest.mark.parametrize("case", range(len(F_BATCHES)))
def test_frames_along_the_wave_and_tile_edges(engine, ops, case):
    """F in {1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 129, 255, 256, 257, 1500}: one wave holding keys (F <= 16), each further wave joining, the last
    64-key tile partial by 1 and by 63, the second 256-column block of colnorm / cost by one column, the full window.  6 heads, four selected from a
    non-zero head downwards with one twice, as one launch and as two (split 0, 1, 3, 4)."""
    f_len, t_len = F_BATCHES[case]
    check(engine, Batch(ops, HEADS6, t_len, f_len, SEL4, seed=10 + case, split=(0, 1, 3, 4)[case]), ("F", case))


@pytest.mark.parametrize("sot_len", [0, 1, 3])
def test_token_counts_on_both_sides_of_16_64_65(engine, ops, sot_len):
    """T in {sot_len + 2 (one cost row), 15, 16, 17, 33, 64, 65, 96}, ragged within a batch: one and two 16-row blocks, colnorm's register path up to 64
    and its loop from 65; 2 heads with one selected, and 6 heads with four."""
    check(engine, Batch(ops, 2, (sot_len + 2, 16, 65, 33), (70, 20, 130, 64), (1,), seed=20 + sot_len, sot_len=sot_len), ("T", sot_len, 0))
    check(engine, Batch(ops, HEADS6, (15, 17, 64, 96), (40, 257, 66, 9), SEL4, seed=30 + sot_len, sot_len=sot_len, split=sot_len), ("T", sot_len, 1))


def test_colnorm_paths_share_their_bytes(engine, ops):
    """A T = 64 clip alone (T_pad 64) and the same clip beside a T = 65 neighbour (T_pad 80, the neighbour on the loop path): identical bytes for
    the shared rows in all three outputs.  The T = 64 clip is on the register path both times, so the two paths are also compared through what they
    share: each clip's w_norm is the sequential fp32 restatement of its own w_soft, bit for bit."""
    solo = Batch(ops, HEADS6, (64,), (130,), SEL4, seed=40, split=1)
    pair = Batch(ops, HEADS6, (64, 65), (130, 130), SEL4, seed=40, split=1)
    assert np.array_equal(pair.q[0, :64], solo.q[0]) and np.array_equal(pair.k[0, :130], solo.k[0, :130])
    o1, o2 = check(engine, solo, "T64 solo"), check(engine, pair, "T64 + T65")
    for a, c in zip(_clip(o1, solo, 0), _clip(o2, pair, 0)):
        assert _same_bits(a, c)
    for i in (0, 1):                                     # the register path (T = 64) and the loop path (T = 65) against the same sequential fp32 sums
        w_soft, w_norm, _ = _clip(o2, pair, i)
        assert _same_bits(w_norm, AL.norm_f32(w_soft)), (i, int((w_norm != AL.norm_f32(w_soft)).sum()))


def _dominant(ops, seed):
    """T = 24 rows over F = 70 keys: row t's key DOM[t % 6] scores more than 100 above the row's other keys (its weight is 1, the rest underflow),
    the dominant key standing in the first tile of each of the four waves (3, 20, 37, 52) and in the last, partial tile (67); rows with t % 6 == 5
    are ordinary, so that no column is constant."""
    b = Batch(ops, HEADS6, (24, 17), (70, 70), SEL4, seed=seed, split=3)
    dom = (3, 20, 37, 52, 67)
    q, k = val(b.q, ops), val(b.k, ops)
    for i in range(b.n):
        k[i, :70] *= 0.25
        for h in range(b.H):
            for j, s in enumerate(dom):
                k[i, s, h * 64 + j] = 64.0
            for t in range(b.t_len[i]):
                if t % 6 != 5:
                    q[i, t, h * 64:h * 64 + 5] = 0.0
                    q[i, t, h * 64 + t % 6] = 20.0                     # 20 x 64 / 8 = 160, the other keys of the row below 30
    b.q, b.k = bits(q, ops), bits(k, ops)
    return b, dom


def test_a_key_100_above_the_rest(engine, ops):
    """Scores where all but one exponential of a row underflow, the survivor in each wave's first tile and in the last partial tile: the merge must take
    the maximum and the sum of the right wave.  The underflowed zeros and the repeated head put equal values into the median windows."""
    b, dom = _dominant(ops, seed=50)
    for i in range(b.n):
        s = AL.soft(val(b.q[i, :b.t_len[i]], ops), val(b.k[i, :70], ops), b.heads_sel, b.scale)[2]
        for t in range(b.t_len[i]):
            if t % 6 != 5:
                top = s[:, t, dom[t % 6]]
                rest = np.delete(s[:, t], dom[t % 6], axis=-1).max(axis=-1)
                assert np.all(top - rest > 100), (i, t)
    w_soft = check(engine, b, "dominant")[0]
    for t in range(24):
        if t % 6 != 5:
            assert np.all(w_soft[0, :, t, dom[t % 6]] == np.float32(1.0)) and np.all(np.delete(w_soft[0, :, t, :70], dom[t % 6], axis=-1) <= TINY)


def test_a_scale_other_than_an_eighth(engine, ops):
    """qk_scale 0.7 (the kernel multiplies by float32(0.125) * float32(0.7)) and scores of three times the spread."""
    check(engine, Batch(ops, HEADS6, (20, 33), (129, 64), SEL4, seed=60, qk_scale=0.7, split=1), "qk_scale 0.7")
    check(engine, Batch(ops, 2, (20, 33), (129, 64), (1,), seed=61, sigma=1.75), "sigma 1.75")


WIDTH_F = {1: [(2, 3, 40)], 3: [(1, 2, 5, 40)], 5: [(2, 3, 9, 40)], 7: [(3, 4, 5, 6), (7, 8, 2, 40)], 9: [(4, 5, 17, 40)], 15: [(7, 8, 29, 257)]}


@pytest.mark.parametrize("width", sorted(WIDTH_F))
def test_median_widths_on_both_sides_of_the_skip(engine, ops, width):
    """Every width's F <= width // 2 (the filter is skipped) and F just above it (every window reflects at both ends); width 7 at F = 3 (leaves the
    network), 4, 5, 6, 7 (the network's smallest rows) and 8."""
    for j, f_len in enumerate(WIDTH_F[width]):
        check(engine, Batch(ops, HEADS6, (9, 20, 5, 17)[:len(f_len)], f_len, SEL4, seed=70 + width + j, width=width, split=j), ("width", width, j))


def _ties(ops):
    b = Batch(ops, HEADS6, (12, 20), (6, 150), SEL4, seed=80, split=3)
    b.k[0, 2:5] = b.k[0, 1]                              # four equal keys in a row of six: equal weights, equal normalised weights
    for s0 in (0, 60, 140):
        b.k[1, s0 + 1:s0 + 6] = b.k[1, s0]               # six equal neighbours at the left edge, across the 64-key tile edge, near the right edge
    return b


def test_the_network_and_the_sort_agree(engine, ops, monkeypatch):
    """Width 7 on a context created with PCE_ALIGN_GENERIC_MEDIAN=1 (the insertion sort) gives the default context's cost bytes: on random rows, on
    the network's smallest rows and on windows of equal values (equal neighbouring keys, the repeated head)."""
    from prosody_control_french_tts_amd import ProsodyEngine
    ties = _ties(ops)
    cases = [ties, Batch(ops, HEADS6, (9, 20, 5, 17), (4, 5, 6, 7), SEL4, seed=81), Batch(ops, 2, (33, 16), (257, 64), (0,), seed=82)]
    outs = [check(engine, b, ("network", j)) for j, b in enumerate(cases)]
    z = outs[0][1][0, 0, 3, :6]
    assert z[1] == z[2] == z[3] == z[4]                  # the ties are there
    monkeypatch.setenv("PCE_ALIGN_GENERIC_MEDIAN", "1")
    with ProsodyEngine(0) as generic:
        generic.whisper_set_operands(ops["name"])
        monkeypatch.delenv("PCE_ALIGN_GENERIC_MEDIAN")
        for j, b in enumerate(cases):
            got = check(generic, b, ("sort", j))
            for a, c in zip(got, outs[j]):
                assert _same_bits(a, c), j


def test_a_clip_does_not_depend_on_its_batch(engine, ops):
    """Clip 1 of a batch of four and the same clip alone: identical bytes in its rows and columns of all three outputs (other paddings, other grid)."""
    t_len, f_len = (33, 17, 65, 5), (257, 70, 16, 1500)
    four = Batch(ops, HEADS6, t_len, f_len, SEL4, seed=90, split=1, k_rows=1500)
    o4 = four.run(engine)
    for i in (1, 2):
        one = Batch(ops, HEADS6, t_len[i:i + 1], f_len[i:i + 1], SEL4, seed=90, split=1)
        assert np.array_equal(one.q[0, :t_len[i]], four.q[i, :t_len[i]]) and np.array_equal(one.k[0, :f_len[i]], four.k[i, :f_len[i]])
        o1 = check(engine, one, ("alone", i))
        for a, c in zip(_clip(o1, one, 0), _clip(o4, four, i)):
            assert _same_bits(a, c), i


def test_refusals_leave_the_outputs_alone(engine, ops):
    """PCE_E_INVALID before any launch: lengths pce_whisper_align_run refuses, frames past the window or the key rows, an even or too wide filter, a head
    outside the model, a split outside 0 .. n_sel, arrays shorter than the shape needs.  The three outputs keep every byte."""
    d = 128

    def call(t_len=(5, 20), f_len=(8, 70), heads_sel=(1, 0), split=0, sot_len=3, width=7, heads=2, k_rows=72, short=None):
        n, n_sel = len(t_len), len(heads_sel)
        T_pad, F_pad, N_max = _ceil(max(t_len), 16), _ceil(max(max(f_len), 1), 64), max(max(t_len) - sot_len - 1, 1)
        size = dict(q=n * T_pad * d, k=n * k_rows * d, w_soft=n * n_sel * T_pad * F_pad, w_norm=n * n_sel * T_pad * F_pad, cost=n * N_max * F_pad)
        if short:
            size[short] -= 1
        q, k = np.zeros(size["q"], np.uint16), np.zeros(size["k"], np.uint16)
        outs = [np.full(size["w_soft"], SENT, np.float32), np.full(size["w_norm"], SENT, np.float32), np.full(size["cost"], SENT, np.float64)]
        before = [o.copy() for o in outs]
        try:
            engine.selftest_align_matrix(heads, q, k, t_len, f_len, heads_sel, *outs, split=split, sot_len=sot_len, medfilt_width=width, k_rows=k_rows)
        except PceError:
            assert all(_same_bits(o, p) for o, p in zip(outs, before))
            raise
        assert not _same_bits(outs[0], before[0]) and not _same_bits(outs[2], before[2])

    call()                                                               # the shape itself is accepted (and writes)
    call(split=2)                                                        # split == n_sel: one launch
    # (f_len = 1501 needs 1501 key rows to get past "f_len > k_rows": it is the "k_rows > 1500" check that turns it down -- no clip can hold more
    #  than 1500 frames because f_len <= k_rows <= 1500)
    for bad in (dict(t_len=(4, 20)), dict(t_len=(5, 449)), dict(f_len=(0, 70)), dict(f_len=(8, 73)), dict(f_len=(8, 1501), k_rows=1501), dict(width=6),
                dict(width=17), dict(width=0), dict(heads_sel=(1, 2)), dict(heads_sel=(-1, 0)), dict(split=3), dict(split=-1), dict(sot_len=-1), dict(heads=33),
                dict(short="q"), dict(short="k"), dict(short="w_soft"), dict(short="w_norm"), dict(short="cost")):
        with pytest.raises(PceError, match="status -1"):
            call(**bad)
