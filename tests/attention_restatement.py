"""Float64 NumPy restatement of scaled dot-product attention over 64-wide heads (the checker of the attention kernels; no test in this file).

Per (clip, head): out = softmax(q k^T / 8) v over the first ``n_keys`` keys, with the causal mask (key j visible to query i only if j <= i) on
request.  Written from the definition, independently of csrc/pce_attention.inc: the scores of a head are one matrix product, the softmax
subtracts the row maximum, NumPy's own (pairwise) sums.

Beside the output it returns A = sum_t p_t |v_t| per output element: every rounding of a kernel's weighted sum is relative to that magnitude, not to
the (possibly cancelling) output, so the bounds of tests/test_gpu_attention.py scale with it.  ``weights`` also returns sum_e |q_e k_e| / 8 per score,
the magnitude an fp32 dot product's rounding is relative to.
"""
import numpy as np

SCALE = 0.125           # 1 / sqrt(64)


def weights(q, k, n_keys=None, causal=False):
    """q [..., Q, 64], k [..., K, 64] -> (p [..., Q, n_keys] softmax weights, mag [..., Q, n_keys] = sum_e |q_e k_e| / 8)."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    n_keys = k.shape[-2] if n_keys is None else n_keys
    assert 1 <= n_keys <= k.shape[-2]
    k = k[..., :n_keys, :]
    s = q @ np.swapaxes(k, -1, -2) * SCALE
    mag = np.abs(q) @ np.swapaxes(np.abs(k), -1, -2) * SCALE
    if causal:
        visible = np.arange(n_keys)[None, :] <= np.arange(q.shape[-2])[:, None]
        s = np.where(visible, s, -np.inf)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True), mag


def attention(q, k, v, n_keys=None, causal=False):
    """q [..., Q, 64], k / v [..., K, 64] -> (out [..., Q, 64], A [..., Q, 64] = sum_t p_t |v_t|) over the first n_keys keys (default: all)."""
    p, _ = weights(q, k, n_keys, causal)
    v = np.asarray(v, dtype=np.float64)[..., :p.shape[-1], :]
    return p @ v, p @ np.abs(v)


def split_heads(x, heads):
    """[rows][heads * 64] -> [heads][rows][64]"""
    x = np.asarray(x)
    return x.reshape(x.shape[0], heads, 64).transpose(1, 0, 2)


def merge_heads(x):
    """[heads][rows][64] -> [rows][heads * 64]"""
    return x.transpose(1, 0, 2).reshape(x.shape[1], -1)
