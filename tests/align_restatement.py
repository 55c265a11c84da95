"""Float64 NumPy restatement of the three stages between the decoder's cross-attention queries and the DTW of the forced alignment (openai-whisper
timing.py find_alignment after the attention logits), one clip at a time; the checker of k_align_scores, k_align_colnorm and k_align_cost (no test in
this file).  Each stage takes the previous stage's array, so a kernel can be checked on the device's own previous output:

    soft   w[h][t][s] = softmax over s < F of q_t . k_s * scale, per selected head (64-wide heads)
    norm   (w - mean_t) / std_t, the population std over the tokens t < T
    cost   reflect padding and the median of ``width`` along s (skipped when F <= width // 2), the mean over heads, rows [sot_len, T - 1), negated

Written from the definitions, independently of csrc/pce_align_kernels.inc: one matrix product per head, NumPy's own (pairwise) sums, np.pad's reflect
mode, a full sort per window.  ``soft`` also returns sum_e |q_e k_e| * scale per score, the magnitude an fp32 dot product's rounding is relative to,
and the scores.

``norm_f32`` is the norm stage in the kernel's arithmetic (sequential fp32 sums; the library is built without contraction or fast-math).

``cost_f32`` is the cost stage in the kernel's arithmetic: a median is a selection (exact in any type), so only the head mean rounds -- the heads added
in ascending order in np.float32, one np.float32 division, then widened and negated.
"""
import numpy as np


def soft(q, k, heads_sel, scale):
    """q [T][H * 64], k [F][H * 64] -> (w, mag, s), each [n_sel][T][F]: the weights, sum_e |q_e k_e| |scale| and the scaled logits themselves"""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    w, mag, logits = [], [], []
    for h in heads_sel:
        qh, kh = q[:, h * 64:(h + 1) * 64], k[:, h * 64:(h + 1) * 64]
        s = qh @ kh.T * scale
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        w.append(e / e.sum(axis=-1, keepdims=True))
        mag.append(np.abs(qh) @ np.abs(kh).T * abs(scale))
        logits.append(s)
    return np.stack(w), np.stack(mag), np.stack(logits)


def norm(w):
    """w [n_sel][T][F] -> (w - mean over t) / population std over t (0 / 0 where a column is constant, as torch gives it)"""
    w = np.asarray(w, dtype=np.float64)
    mean = w.mean(axis=-2, keepdims=True)
    std = np.sqrt(((w - mean) ** 2).mean(axis=-2, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (w - mean) / std


def norm_f32(w):
    """The same in k_align_colnorm's arithmetic on float32 weights: the sum over t in sequence, the mean, the squares of the deviations in sequence,
    sqrt of their mean, (w - mean) / std, every operation rounded once to np.float32 (both paths of the kernel add in this order)."""
    w = np.asarray(w)
    assert w.dtype == np.float32
    T = np.float32(w.shape[-2])
    total = np.zeros(w.shape[:-2] + w.shape[-1:], dtype=np.float32)
    for t in range(w.shape[-2]):
        total = total + w[..., t, :]
    mean = total / T
    q = np.zeros_like(total)
    for t in range(w.shape[-2]):
        a = w[..., t, :] - mean
        q = q + a * a
    std = np.sqrt(q / T)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (w - mean[..., None, :]) / std[..., None, :]
    assert out.dtype == np.float32
    return out


def median_filter(x, width):
    """median of ``width`` along the last axis with reflect padding; rows of at most width // 2 elements pass unfiltered.  Keeps x's dtype."""
    x = np.asarray(x)
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    padded = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    windows = np.lib.stride_tricks.sliding_window_view(padded, width, axis=-1)
    return np.sort(windows, axis=-1)[..., pad]


def cost(w_norm, sot_len, width):
    """w_norm [n_sel][T][F] -> float64 [T - sot_len - 1][F]"""
    w = np.asarray(w_norm, dtype=np.float64)
    return -median_filter(w, width).mean(axis=0)[sot_len:w.shape[1] - 1]


def cost_f32(w_norm, sot_len, width):
    """The same in the kernel's arithmetic on float32 weights: heads added in ascending order and divided in np.float32, widened, negated."""
    w = np.asarray(w_norm)
    assert w.dtype == np.float32
    med = median_filter(w, width)
    acc = np.zeros(med.shape[1:], dtype=np.float32)
    for h in range(med.shape[0]):
        acc = acc + med[h]
    assert acc.dtype == np.float32
    return -((acc / np.float32(med.shape[0])).astype(np.float64))[sot_len:w.shape[1] - 1]
