"""The float64 restatement of the forced alignment's matrix stages (tests/align_restatement.py), which tests/test_gpu_align_matrix.py compares the
kernels against, pinned to the pieces of oracle/whisper_oracle.py's find_alignment the end-to-end tests already trust: torch's softmax,
torch.std_mean(unbiased=False) and the oracle's median_filter, all in float64.

Agreement required (E = 2^-53, double-precision round-off; nothing here is fitted):
  * soft: two 64-term dot products in different orders move an exponent by at most 2 x 64 E x sum |q_e k_e| scale, the two softmaxes add a few
    roundings per term of the sum: |dw| <= w (128 E max mag + (F + 8) E);
  * norm: sums of T terms in two orders, against the column's mean and deviation: |dz| <= 4 (T + 4) E (|z| + mean / std); its sequential fp32
    variant (U = 2^-24): (4 T + 8) U (|z| + mean / std);
  * the median is a selection: identical bits; the head mean: (n_sel + 2) E x mean |median|;
  * the fp32 variant of the cost against the fp64 one: n_sel - 1 additions and one division in fp32: n_sel x 2^-24 x mean |median|."""
import numpy as np
import pytest
import torch

from oracle import whisper_oracle as WO
from tests import align_restatement as AL

E = 2.0 ** -53
U = 2.0 ** -24
WIDTHS = (1, 3, 5, 7, 15)


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("T,F,H,heads_sel,scale", [(5, 1, 2, [1], 0.125), (17, 3, 6, [5, 0, 3, 3], 0.125), (33, 70, 6, [5, 0, 3, 3], 0.0875),
                                                   (20, 257, 3, [2, 1], 0.125)])
def test_soft_agrees_with_torch_softmax(T, F, H, heads_sel, scale):
    rng = _rng(T * 1000 + F)
    q, k = rng.standard_normal((T, H * 64)) * 1.5, rng.standard_normal((F + 3, H * 64)) * 1.5
    w, mag, logits = AL.soft(q, k[:F], heads_sel, scale)
    assert w.shape == mag.shape == logits.shape == (len(heads_sel), T, F)
    tq, tk = torch.from_numpy(q).view(T, H, 64).permute(1, 0, 2), torch.from_numpy(k).view(F + 3, H, 64).permute(1, 2, 0)
    qk = (tq @ tk)[heads_sel][:, :, :F]                                   # find_alignment: the logits cut to the clip's frames, then the softmax
    want = (qk * scale).softmax(dim=-1).numpy()
    assert np.all(np.abs(w - want) <= want * (128 * E * mag.max() + (F + 8) * E))
    assert np.allclose(w.sum(axis=-1), 1.0, rtol=0, atol=(F + 8) * E)
    assert np.allclose(logits, (qk * scale).numpy(), rtol=0, atol=128 * E * mag.max())
    if F == 1:
        assert np.all(w == 1.0)


@pytest.mark.parametrize("T,F", [(2, 4), (16, 9), (65, 70)])
def test_norm_agrees_with_torch_std_mean(T, F):
    w = torch.from_numpy(_rng(T + F).standard_normal((3, T, F)) * 2.0).softmax(dim=-1)
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    want = ((w - mean) / std).numpy()
    got = AL.norm(w.numpy())
    tol = 4 * (T + 4) * E * (np.abs(want) + (mean / std).numpy())
    assert np.all(np.abs(got - want) <= tol)
    assert np.allclose(got.mean(axis=-2), 0.0, atol=1e-12) and np.allclose((got ** 2).mean(axis=-2), 1.0, atol=1e-12)
    # the fp32 variant: T additions, a mean, T squares and their sum, sqrt, one subtraction and one division in fp32 against a column whose
    # deviations are of the size of its mean (softmax columns): (4 T + 8) U (|z| + mean / std)
    w32 = w.numpy().astype(np.float32)
    got32, want32 = AL.norm_f32(w32), AL.norm(w32)
    mean, std = w32.astype(np.float64).mean(axis=-2, keepdims=True), w32.astype(np.float64).std(axis=-2, keepdims=True)
    assert got32.dtype == np.float32 and np.all(np.abs(got32 - want32) <= (4 * T + 8) * U * (np.abs(want32) + mean / std))


def test_norm_of_a_constant_column_is_nan_like_torch():
    w = np.full((1, 4, 2), 1.0); w[0, :, 1] = [0.1, 0.2, 0.3, 0.4]
    got = AL.norm(w)
    t = torch.from_numpy(w)
    std, mean = torch.std_mean(t, dim=-2, keepdim=True, unbiased=False)
    assert np.isnan(got[0, :, 0]).all() and torch.isnan(((t - mean) / std)[0, :, 0]).all() and np.isfinite(got[0, :, 1]).all()


def _median_by_index_rule(row, width):
    """reflect: index -i for i < 0, 2 (F - 1) - i for i >= F; a plain Python sort per window"""
    F, pad = len(row), width // 2
    if F <= pad:
        return list(row)
    out = []
    for s in range(F):
        win = []
        for u in range(width):
            i = s - pad + u
            i = -i if i < 0 else i
            i = 2 * (F - 1) - i if i >= F else i
            win.append(row[i])
        out.append(sorted(win)[pad])
    return out


@pytest.mark.parametrize("width", WIDTHS)
def test_median_filter_agrees_with_the_oracle_bit_for_bit(width):
    pad = width // 2
    for F in sorted({1, max(1, pad), pad + 1, pad + 2, 2 * pad + 1, 2 * pad + 2, 40}):      # F <= pad (unfiltered), just above it, one window, more
        x = _rng(100 * width + F).standard_normal((3, 6, F))
        x[0, 0, : F // 2] = 0.25                                                           # ties inside a window
        got = AL.median_filter(x, width)
        want = WO.median_filter(torch.from_numpy(x), width).numpy()
        assert got.shape == x.shape and np.array_equal(got, want), (width, F)
        assert got[1, 2].tolist() == _median_by_index_rule(x[1, 2].tolist(), width), (width, F)
        if F <= pad:
            assert np.array_equal(got, x)
        g32 = AL.median_filter(x.astype(np.float32), width)
        assert g32.dtype == np.float32 and np.array_equal(g32, AL.median_filter(x.astype(np.float32).astype(np.float64), width))


def test_median_filter_by_hand():
    assert AL.median_filter(np.array([1.0, 2.0, 3.0, 4.0]), 3).tolist() == [2.0, 2.0, 3.0, 3.0]          # windows 212 123 234 343
    # width 7 on 4 elements: both reflections inside one window: 3210123 -> 2, 2101232 -> 2, 1012321 -> 1 (sorted 0111223), 0123210 -> 1
    assert AL.median_filter(np.array([0.0, 1.0, 2.0, 3.0]), 7).tolist() == [2.0, 2.0, 1.0, 1.0]
    assert AL.median_filter(np.array([5.0, 1.0, 9.0]), 7).tolist() == [5.0, 1.0, 9.0]                    # F <= 3: unfiltered


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("sot_len", [0, 3])
def test_cost_agrees_with_find_alignment_tail(width, sot_len):
    pad = width // 2
    for F in sorted({max(1, pad), pad + 1, 33}):
        n_sel, T = 4, sot_len + 6
        z = _rng(width * 37 + F + sot_len).standard_normal((n_sel, T, F))
        z[3] = z[1]                                                                        # a head listed twice
        got = AL.cost(z, sot_len, width)
        med = WO.median_filter(torch.from_numpy(z), width)
        want = (-(med.mean(axis=0)[sot_len:-1])).numpy()                                   # find_alignment: mean over heads, [sot_len:-1], negated
        mag = med.abs().mean(axis=0)[sot_len:-1].numpy()
        assert got.shape == want.shape == (T - sot_len - 1, F)
        assert np.all(np.abs(got - want) <= (n_sel + 2) * E * mag)
        z32 = z.astype(np.float32)
        got32 = AL.cost_f32(z32, sot_len, width)
        want64 = AL.cost(z32, sot_len, width)
        mag32 = np.abs(AL.median_filter(z32.astype(np.float64), width)).mean(axis=0)[sot_len:T - 1]
        assert got32.dtype == np.float64 and np.all(np.abs(got32 - want64) <= n_sel * U * mag32 + (n_sel + 2) * E * mag32)
        assert np.array_equal(got32, got32.astype(np.float32).astype(np.float64))          # the widened fp32 quotient, nothing finer


def test_one_cost_row_and_one_head():
    z = _rng(9).standard_normal((1, 5, 12)).astype(np.float32)                             # T == sot_len + 2: one row, t = sot_len
    c = AL.cost_f32(z, 3, 7)
    assert c.shape == (1, 12) and np.array_equal(c[0], -AL.median_filter(z, 7)[0, 3].astype(np.float64))
