"""The resampler's spec (csrc/pce_resample.hip) in long double, and the cases tests/test_resample_host.py and tests/test_gpu_resample.py share.

y[i] = sum_m h[n - m up] x[m] with n = (i + n_pre_remove) down, over 0 <= n - m up < len(h) and 0 <= m < len(x); the output is rint(y), half to even,
saturated to int16.  The kernel accumulates the K terms it uses with one fma each: K roundings, none of a partial sum above sum |h x|, so its y lies within
(K + 1) 2^-53 sum |h x| of the exact one (the + 1 covers the long double's own roundings many times over) and its output may differ from
rint(exact), by one step, only where the exact y lies that close to a half-integer (``near``)."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
RATIOS = ((44100, 16000), (48000, 16000), (24000, 16000), (22050, 16000), (8000, 16000), (16000, 22050), (16000, 44100))


def reference(x, up, down, taps, n_pre_remove):
    """-> (want int16 [n_out], near bool [n_out], y LD [n_out])."""
    x = np.asarray(x, np.int64); h = np.asarray(taps, np.float64)
    n_in, nt = len(x), len(h)
    n_out = -(-n_in * up // down)
    if n_out == 0:
        return np.zeros(0, np.int16), np.zeros(0, bool), np.zeros(0, LD)
    n = (np.arange(n_out, dtype=np.int64) + n_pre_remove) * down
    K = -(-nt // up) + 1
    m = (n // up)[:, None] - np.arange(K)[None, :]                  # from the newest input sample backwards
    t = n[:, None] - m * up
    live = (t >= 0) & (t < nt) & (m >= 0) & (m < n_in)
    hv = np.where(live, h[np.clip(t, 0, nt - 1)], 0.0).astype(LD)
    xv = np.where(live, x[np.clip(m, 0, max(n_in - 1, 0))] if n_in else 0, 0).astype(LD)
    prod = hv * xv
    y = prod.sum(1)
    window = (live.sum(1) + 1) * LD(2.0) ** -53 * np.abs(prod).sum(1)
    frac = y - np.floor(y)
    near = np.abs(frac - LD(0.5)) <= window
    want = np.clip(np.rint(y), -32768, 32767).astype(np.int16)     # np.rint of a long double: half to even
    return want, near, y


def exact(x, up, down, taps, n_pre_remove):
    """The same in rational arithmetic (dyadic taps, small inputs): every sum exact, Python's round() is half to even."""
    h = [Fraction(float(v)) for v in taps]
    n_out = -(-len(x) * up // down)
    out = []
    for i in range(n_out):
        n = (i + n_pre_remove) * down
        y = sum((h[n - m * up] * int(x[m]) for m in range(len(x)) if 0 <= n - m * up < len(h)), Fraction(0))
        out.append(min(max(round(y), -32768), 32767))
    return np.array(out, np.int16)


def clips(rate_in, rate_out, span):
    """A ragged batch: 0 samples, 1 sample, one sample less and one more than the filter's span, 0.3 s of noise, a full-scale square."""
    rng = np.random.default_rng(rate_in + 7 * rate_out)
    noise = lambda k: np.clip(np.rint(6000 * rng.standard_normal(k)), -32768, 32767).astype(np.int16)
    n = int(0.3 * rate_in) + 1
    square = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32767).astype(np.int16)
    return [np.zeros(0, np.int16), noise(1), noise(span - 1), noise(span + 1), noise(n), square]


TIES = (                                                          # (up, down, taps, n_pre_remove): dyadic taps, every sum exact
    (1, 1, [0.5, 0.5], 0),
    (1, 2, [0.25, 0.5, 0.25], 0),
    (2, 1, [0.5, 1.0, 0.5], 0),
    (1, 1, [1.5, 1.0], 0),                                        # reaches both rails and the half steps beside them
)


def tie_clip():
    rng = np.random.default_rng(5)
    small = rng.integers(-9, 10, 200)
    edge = np.array([32767, 32767, 32766, 32767, -32768, -32768, -32767, -32768, 13107, 13107, 13106, 13107, -13107, -13107, -13108, -13107, 1, 0, -1, 0, 3, 2])
    return np.concatenate([small, edge, np.arange(-40, 41)]).astype(np.int16)
