"""float64 restatement of torchcrepe's ``predict`` (preprocess / infer / postprocess with its default ``viterbi`` decoder, no dither) as
include/pce.h, "CREPE pitch tracking", states it -- written from that description, independent of csrc/pce_crepe.hip.  torchcrepe is not
installed: parity with the package itself is unpinned.

``emulate=True`` rounds to fp16 where the device stores fp16: the conv weights, the normalised frame, and every block's pooled output (the last
one is the embedding).  The classifier's weights, BatchNorm's (scale, shift), the biases and the salience are fp32 on the device; the
restatement keeps their float32 VALUES and computes in float64.
"""
import math

import numpy as np

from prosody_control_french_tts_amd import crepe_weights as CW

TINY = np.finfo(np.float64).tiny


def r16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ framing
def frames(pcm16, hop: int):
    """int16 samples at 16 kHz -> float64 [n_frames, 1024]: x / 32768, 512 zeros on both sides, frame t = padded [t hop, t hop + 1024),
    minus its mean, over max(1e-10, unbiased std)."""
    x = np.asarray(pcm16, dtype=np.float64) / 32768.0
    n = CW.n_frames(len(x), hop)
    pad = np.concatenate([np.zeros(512), x, np.zeros(512 + CW.WINDOW_SIZE)])
    fr = np.stack([pad[t * hop:t * hop + CW.WINDOW_SIZE] for t in range(n)])
    fr = fr - fr.mean(axis=1, keepdims=True)
    sd = np.sqrt((fr ** 2).sum(axis=1, keepdims=True) / (CW.WINDOW_SIZE - 1))          # (the mean is removed already)
    return fr / np.maximum(1e-10, sd)


# ------------------------------------------------------------------------------------------------------------ one block
def im2row(x, block: int):
    """x [t_in, c_in] (block 1: [1024, 1]) -> the operand rows [t_conv, taps * c_in] of the zero-padded, time-major image."""
    t_in, c_in = x.shape
    if block == 1:
        pad = np.concatenate([np.zeros((254, 1)), x, np.zeros((254, 1))]); taps, stride, rows = 512, 4, 256
    else:
        pad = np.concatenate([np.zeros((31, c_in)), x, np.zeros((32, c_in))]); taps, stride, rows = 64, 1, t_in
    flat = np.ascontiguousarray(pad).reshape(-1)
    s = flat.strides[0]
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, taps * c_in), strides=(stride * c_in * s, s), writeable=False)


def block_forward(x, block: int, w, bias, scale, shift, with_bound=False):
    """One block on ONE frame: x [t_in, c_in], w [c_out, taps, c_in] -> pooled [t_conv / 2, c_out] float64 (not rounded).
    ``with_bound``: also the per-element accumulation bound K 2^-23 |scale| sum(|a| |b|), the larger of the two pooled rows'."""
    a = np.ascontiguousarray(im2row(np.asarray(x, dtype=np.float64), block))        # (a copy: BLAS does not take overlapping rows)
    wm = np.asarray(w, dtype=np.float64).reshape(w.shape[0], -1)
    acc = a @ wm.T
    y = np.maximum(acc + bias, 0.0) * scale + shift                 # ReLU, then BatchNorm; pooled after BatchNorm
    pooled = np.maximum(y[0::2], y[1::2])
    if not with_bound:
        return pooled
    k = a.shape[1]
    sab = np.abs(a) @ np.abs(wm).T
    bnd = k * 2.0 ** -23 * np.abs(scale) * sab
    return pooled, np.maximum(bnd[0::2], bnd[1::2])


# ------------------------------------------------------------------------------------------------------------ the network
def salience(frames64, c_out, flat, emulate: bool):
    """Normalised frames [n, 1024] -> salience [n, 360] float64."""
    blocks, cw, cb = CW.unfold(c_out, flat)
    ws = [(r16(w) if emulate else np.asarray(w, dtype=np.float64), *(np.asarray(v, dtype=np.float64) for v in (b, sc, sh))) for w, b, sc, sh in blocks]
    cw = np.asarray(cw, dtype=np.float64); cb = np.asarray(cb, dtype=np.float64)
    out = np.zeros((len(frames64), CW.PITCH_BINS))
    for f, fr in enumerate(frames64):
        x = (r16(fr) if emulate else fr).reshape(-1, 1)
        for i, (w, b, sc, sh) in enumerate(ws):
            x = block_forward(x, i + 1, w, b, sc, sh)
            if emulate:
                x = r16(x)
        z = cw @ x.reshape(-1) + cb                                 # time-major, then channel
        out[f] = 1.0 / (1.0 + np.exp(-z))
    return out


# ------------------------------------------------------------------------------------------------------------ decoding
def log_transition():
    """log(T + tiny), T[i, j] = max(12 - |i - j|, 0) with rows normalised to 1."""
    i = np.arange(CW.PITCH_BINS)
    t = np.maximum(12 - np.abs(i[:, None] - i[None, :]), 0).astype(np.float64)
    t = t / t.sum(axis=1, keepdims=True)
    return np.log(t + TINY)


def log_observation(sal, lo: int, hi: int, order: str = "numpy"):
    """Mask, softmax over the 360 sigmoid outputs, log(p + tiny).  ``order``: how the softmax denominator is summed (``"numpy"``: pairwise;
    ``"reversed"``: one term after the other from the last bin down) -- two float64 evaluations that differ in rounding only."""
    p = np.array(sal, dtype=np.float64)
    p[:, :lo] = -np.inf; p[:, hi:] = -np.inf
    e = np.exp(p - p.max(axis=1, keepdims=True))
    if order == "numpy":
        s = e.sum(axis=1, keepdims=True)
    else:
        s = np.zeros((len(e), 1))
        for b in range(CW.PITCH_BINS - 1, -1, -1):
            s[:, 0] = s[:, 0] + e[:, b]
    return np.log(e / s + TINY)


def viterbi(log_prob, log_trans=None):
    """``librosa.sequence.viterbi`` on log probabilities: uniform initial state, dense arg-max (first maximum), walk back."""
    lt = log_transition() if log_trans is None else log_trans
    n, s = log_prob.shape
    value = log_prob[0] + math.log(1.0 / s + TINY)
    ptr = np.zeros((n, s), dtype=np.int64)
    for t in range(1, n):
        trans_out = value[None, :] + lt.T                            # [target j, predecessor i]
        ptr[t] = np.argmax(trans_out, axis=1)
        value = log_prob[t] + trans_out[np.arange(s), ptr[t]]
    states = np.zeros(n, dtype=np.int64)
    states[-1] = int(np.argmax(value))
    for t in range(n - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def decode(sal, lo: int, hi: int, decoder: str = "viterbi", order: str = "numpy"):
    """-> (bins, f0 Hz, periodicity = sal[t, bin[t]])."""
    sal = np.asarray(sal)
    if decoder == "viterbi":
        bins = viterbi(log_observation(sal, lo, hi, order))
    else:
        p = np.array(sal, dtype=np.float64); p[:, :lo] = -np.inf; p[:, hi:] = -np.inf
        bins = np.argmax(p, axis=1)
    return bins, CW.bins_to_frequency(bins), sal[np.arange(len(sal)), bins]


def predict(pcm16, hop: int, c_out, flat, fmin: float, fmax: float, emulate: bool = False, decoder: str = "viterbi"):
    lo, hi = CW.mask_range(fmin, fmax)
    sal = salience(frames(pcm16, hop), c_out, flat, emulate)
    return (sal,) + decode(sal, lo, hi, decoder)
