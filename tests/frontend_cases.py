"""tests/frontend_cases.py -- TEST INFRASTRUCTURE: the signals tests/test_gpu_frontend.py feeds the log-mel and STFT kernels, by name, so that
tests/test_frontend_host.py judges the very same inputs on the CPU (int16, 16 kHz)."""
import numpy as np


def silence(n):
    return np.zeros(n, dtype=np.int16)


def lsb_noise(n, seed=2):
    """+-1 LSB, no zeros: every log10 on the way is negative."""
    return (np.random.default_rng(seed).integers(0, 2, n) * 2 - 1).astype(np.int16)


def noise(n, seed=1, sigma=3000.0):
    return np.clip(np.rint(np.random.default_rng(seed).standard_normal(n) * sigma), -32768, 32767).astype(np.int16)


def square(n, half_period=36):
    """Full scale: -32768 / +32767."""
    return np.where((np.arange(n) // half_period) % 2 == 0, 32767, -32768).astype(np.int16)


def dc_min(n):
    return np.full(n, -32768, dtype=np.int16)


def tone(n, hz=220.0, amp=0.6):
    return np.round(amp * 32767 * np.sin(2 * np.pi * hz * np.arange(n) / 16000.0)).astype(np.int16)


def impulses(n, at, amp=1):
    x = np.zeros(n, dtype=np.int16)
    for i, p in enumerate(np.atleast_1d(at)):
        if 0 <= p < n:
            x[p] = np.atleast_1d(amp)[i % np.size(amp)]
    return x


def loud_then_lsb(n, loud=3200, seed=3):
    """0.2 s of the full-scale square, then +-1 LSB: the quiet part lies more than 8 decades (80 dB) below the loud part's maximum."""
    x = lsb_noise(n, seed)
    m = min(n, loud)
    x[:m] = square(m)
    return x


def content(name, n, seed=0):
    """One clip of ``n`` samples by family name."""
    if name == "silence":
        return silence(n)
    if name == "lsb":
        return lsb_noise(n, 20 + seed)
    if name == "square":
        return square(n)
    if name == "dc_min":
        return dc_min(n)
    if name == "noise":
        return noise(n, 10 + seed)
    if name == "tone":
        return tone(n)
    if name == "loud_lsb":
        return loud_then_lsb(n, seed=30 + seed)
    raise KeyError(name)


CONTENTS = ("silence", "lsb", "square", "dc_min", "noise", "tone", "loud_lsb")
FLAT_N = 8000                                 # 0.5 s


def flat_inputs():
    """The flat-spectrum inputs whose bound is asserted to be tight (tests/test_frontend_host.py): white noise at sigma 3000 and +-1 LSB noise."""
    return [("noise", noise(FLAT_N, 1, 3000.0)), ("lsb", lsb_noise(FLAT_N, 2))]
