"""float64 restatements of the three stages pce_w2v.inc adds -- the waveform layer with its normalisation, LayerNorm (+ GELU) over 16-bit rows, the
grouped 128-tap positional convolution -- on the operands the device takes (16-bit values where it reads 16-bit values).  Each returns its
result, not rounded, and a per-element bound on what fp32 arithmetic in any order may add to it; the caller adds the rounding of the stored value.

The bounds, derived.  A sum of K products in fp32 differs from the exact sum by at most K 2^-23 sum(|a| |w|).  A normalisation
z = (v - mean) gamma / sqrt(var + eps) + beta of values that carry the errors e_v (``norm_bound``): the mean moves by at most mean(e_v) plus, where
the statistics are summed in fp32, n 2^-24 mean(|v|); the centred value by e_v plus that plus its own rounding; the variance by
mean(2 |v - mean| e_centred) plus its summation error, and 1 / sqrt(var + eps) relatively by half of that over (var + eps), plus two ulps for the
division and the reciprocal square root; the three fp32 operations of the affine step round |z - beta| and |z| once more.  GELU has slope
at most 1.13; the device's erf (Abramowitz-Stegun 7.1.26, |error| < 1.5e-7, behind a 1-ulp reciprocal and exponential) adds at most
2e-7 (1 + |x|) to GELU(x)."""
import numpy as np
import torch

U23, U24 = 2.0 ** -23, 2.0 ** -24
GELU_SLOPE, GELU_APPROX = 1.13, 2e-7
TAPS0, POS_TAPS = 10, 128


def to_bits(x, bf16=False):
    """float array -> the uint16 bits of its fp16 (or bf16, round to nearest even) values."""
    if not bf16:
        return np.asarray(x, dtype=np.float64).astype(np.float16).view(np.uint16)
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(b, bf16=False):
    b = np.asarray(b, dtype=np.uint16)
    if not bf16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def r16(x, bf16=False):
    return from_bits(to_bits(x, bf16), bf16)


def stored_step(bf16=False):
    """Relative rounding of a stored 16-bit value: half an ulp of 11 (fp16) or 8 (bf16) significand bits."""
    return 2.0 ** -8 if bf16 else 2.0 ** -11


def gelu(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / np.sqrt(2.0))).numpy())


def gelu_bound(x, e_x):
    return GELU_SLOPE * e_x + GELU_APPROX * (1.0 + np.abs(x))


def norm_bound(v, e_v, gamma, beta, eps, axis, fp32_stats):
    """(z, bound on |z_device - z|) of the normalisation of ``v`` along ``axis`` (biased variance); gamma / beta broadcast against v."""
    n = v.shape[axis]
    mean = v.mean(axis=axis, keepdims=True)
    cen = v - mean
    var = (cen * cen).mean(axis=axis, keepdims=True)
    sig = np.sqrt(var + eps)
    z = cen / sig * gamma + beta
    s32 = n * U24 if fp32_stats else 0.0
    e_mean = e_v.mean(axis=axis, keepdims=True) + s32 * np.abs(v).mean(axis=axis, keepdims=True)
    e_cen = e_v + e_mean + U23 * np.abs(cen)
    e_var = (2.0 * np.abs(cen) * e_cen).mean(axis=axis, keepdims=True) + (s32 + U23) * var
    rel = 0.5 * e_var / (var + eps) + 2.0 * U23
    # (statistics in fp64: the device folds them into z = y scale + shift, scale and shift rounded to fp32: the mean's share of both rounds too)
    folded = 0.0 if fp32_stats else 2.0 * U23 * np.abs(mean) * np.abs(gamma) / sig
    return z, np.abs(gamma) / sig * e_cen + np.abs(z - beta) * rel + 2.0 * U23 * (np.abs(z - beta) + np.abs(z)) + folded


# ------------------------------------------------------------------------------------------------------------ the waveform layer
def windows(pcm, window, context):
    """int16 clip -> float64 [n_windows][window + 2 context]: samples / 32768, ``context`` zeros in front, zeros behind to whole windows + context."""
    x = np.asarray(pcm, dtype=np.float64).reshape(-1) / 32768.0
    n_win = max(1, -(-len(x) // window))
    padded = np.concatenate([np.zeros(context), x, np.zeros(context + n_win * window - len(x))])
    return np.stack([padded[j * window: j * window + window + 2 * context] for j in range(n_win)])


def wave_layer(pcm, window, context, feat_norm, w, bias, gamma, beta, stride=5, eps=1e-5):
    """-> (GELU(norm(conv(windows))) [n_windows][T0][C] float64, bound).  feat_norm 0: per channel over all frames of the window, the zeros of
    the padding included (statistics in fp64 on the device: no summation term); 1: per frame over the channels, with the bias (fp32 statistics)."""
    xw = windows(pcm, window, context)
    length = xw.shape[1]
    t0 = (length - TAPS0) // stride + 1 if length >= TAPS0 else 0
    w = np.asarray(w, dtype=np.float64)
    if t0 == 0:
        z = np.zeros((xw.shape[0], 0, w.shape[0]))
        return z, z
    a = np.lib.stride_tricks.sliding_window_view(xw, TAPS0, axis=1)[:, ::stride][:, :t0]          # [n_win][T0][10]
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, dtype=np.float64)
    y = a @ w.T + b
    e_y = TAPS0 * U23 * (np.abs(a) @ np.abs(w).T) + U23 * np.abs(y)
    g, be = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    z, e_z = norm_bound(y, e_y, g, be, eps, axis=1 if feat_norm == 0 else 2, fp32_stats=feat_norm != 0)
    return gelu(z), gelu_bound(z, e_z)


# ------------------------------------------------------------------------------------------------------------ LayerNorm (+ GELU) over 16-bit rows
def ln_gelu(x, w, b, eps=1e-5, with_gelu=True):
    """x [rows][C] float64 (the 16-bit values the device reads: exact) -> (LayerNorm over C, then GELU where asked; bound)."""
    x = np.asarray(x, dtype=np.float64)
    z, e_z = norm_bound(x, np.zeros_like(x), np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64), eps, axis=1, fp32_stats=True)
    return (gelu(z), gelu_bound(z, e_z)) if with_gelu else (z, e_z)


# ------------------------------------------------------------------------------------------------------------ the positional convolution
def pos_conv(x, w, bias, groups):
    """x [windows][T][d] float64 (16-bit values), w [d][128][d / groups] float64 (16-bit values; the blob's layout), bias [d] ->
    (x + GELU(conv + bias) [windows][T][d], bound): output frame t reads frames t - 64 .. t + 63 of ITS window, zeros outside [0, T)."""
    x, w, bias = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    n_win, t, d = x.shape
    cg = d // groups
    xp = np.concatenate([np.zeros((n_win, POS_TAPS // 2, d)), x, np.zeros((n_win, POS_TAPS // 2, d))], axis=1)
    acc, sab = np.zeros_like(x), np.zeros_like(x)
    for g in range(groups):
        cols = slice(g * cg, (g + 1) * cg)
        a = np.lib.stride_tricks.sliding_window_view(xp[:, :, cols], POS_TAPS, axis=1)[:, :t]          # [n_win][T][cg (in)][128]
        a = np.ascontiguousarray(np.transpose(a, (0, 1, 3, 2))).reshape(n_win, t, POS_TAPS * cg)      # K = (tap, channel)
        wm = w[cols].reshape(cg, POS_TAPS * cg)
        acc[:, :, cols] = a @ wm.T
        sab[:, :, cols] = np.abs(a) @ np.abs(wm).T
    pre = acc + bias
    e_pre = POS_TAPS * cg * U23 * sab + U23 * np.abs(pre)
    y = x + gelu(pre)
    return y, gelu_bound(pre, e_pre) + U23 * np.abs(y)
