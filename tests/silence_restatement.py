"""pydub 0.25.1's ``detect_silence`` restated twice, for the tests of ``pce_silence_*``.

``detect_silence``: the specification of include/pce.h in numpy -- an int64 cumulative sum of the squares, the window test in integers
(``sum x^2 < (T + 1)^2 n``), the combining rule on the silent starts.

``detect_silence_literal``: pydub's own loop -- ``hostrules.pydub_slice_frames`` for ``seg[i:i + min_silence_len]`` with its zero padding
appended, stdlib ``audioop.rms`` on the window's bytes, compared with the FLOAT threshold ``10 ** (dB / 20) * 32768`` -- O(samples x window).
audioop is the function pydub calls, so this pins the window test; pydub itself is absent, so the range bookkeeping (``combine``) is a
restatement of its published source in both.
"""
import numpy as np

from prosody_control_french_tts_amd import hostrules as H


def slice_samples(clip, begin, end):
    """Samples [begin, end) of a clip; positions outside the clip are zeros."""
    out = np.zeros(max(end - begin, 0), dtype=np.int16)
    b, e = max(begin, 0), min(end, len(clip))
    if e > b:
        out[b - begin:e - begin] = clip[b:e]
    return out


def window_starts(len_ms, L, step):
    if len_ms < L:
        return []
    last = len_ms - L
    starts = list(range(0, last + 1, step))
    if last % step:
        starts.append(last)
    return starts


def combine(silent_starts, L, step):
    ranges, prev, first = [], None, None
    for s in silent_starts:
        if prev is None:
            first = s
        elif s != prev + step and s > prev + L:
            ranges.append([first, prev + L])
            first = s
        prev = s
    if prev is not None:
        ranges.append([first, prev + L])
    return ranges


def silent_starts(x, rate, L, T, step=1, channels=1):
    """-> (silent window starts, len_ms) of an interleaved int16 stream."""
    x = np.asarray(x, dtype=np.int16)
    n = len(x) // channels
    len_ms = H.pydub_len_ms(n, rate)
    starts = np.array(window_starts(len_ms, L, step), dtype=np.int64)
    if not len(starts):
        return [], len_ms
    b = (np.arange(len_ms + 1, dtype=np.float64) * (rate / 1000.0)).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(x.astype(np.int64) ** 2)])
    P = csum[np.minimum(b * channels, n * channels)]
    S = P[starts + L] - P[starts]
    n_i = (b[starts + L] - b[starts]) * channels
    return starts[S < (T + 1) ** 2 * n_i].tolist(), len_ms


def detect_silence(x, rate, L=1000, T=None, step=1, channels=1, silence_thresh=-16):
    """-> (silent ranges [[start_ms, end_ms]], len_ms).  ``T``: the integer threshold; None: from ``silence_thresh`` dB."""
    T = H.silence_rms_max(silence_thresh) if T is None else T
    s, len_ms = silent_starts(x, rate, L, T, step, channels)
    return combine(s, L, step), len_ms


def detect_silence_literal(x, rate, L=1000, silence_thresh=-16, step=1, channels=1):
    import audioop
    x = np.asarray(x, dtype=np.int16)
    n = len(x) // channels
    len_ms = H.pydub_len_ms(n, rate)
    thr = 10 ** (float(silence_thresh) / 20) * 32768.0
    silent = []
    for i in window_starts(len_ms, L, step):
        b, e = H.pydub_slice_frames(n, rate, i, i + L)
        w = np.concatenate([x[b * channels:min(e, n) * channels], np.zeros(max(e - n, 0) * channels, dtype=np.int16)])
        if audioop.rms(w.astype("<i2").tobytes(), 2) <= thr:
            silent.append(i)
    return combine(silent, L, step), len_ms


def bursts(rate, plan, seed=0, amplitude=3000, channels=1):
    """A clip of ``plan`` = [(milliseconds, loud)]: uniform noise where loud, zeros elsewhere."""
    rng = np.random.default_rng(seed)
    parts = []
    for ms, loud in plan:
        k = int(round(ms * rate / 1000.0)) * channels
        parts.append(rng.integers(-amplitude, amplitude + 1, k).astype(np.int16) if loud else np.zeros(k, dtype=np.int16))
    return np.concatenate(parts)


def case_clips(rate):
    """The clips both test files use, by name."""
    rng = np.random.default_rng(rate)
    c = {
        "const103": np.full(2 * rate, 103, dtype=np.int16),                   # at -50 dB T = 103: every window silent
        "const104": np.full(2 * rate, 104, dtype=np.int16),                   # ... and none
        "rounds_up": bursts(rate, [(700, 0), (900, 1), (1400, 0)], 1)[:3 * rate],
        "gaps": bursts(rate, [(400, 0), (60, 1), (300, 0), (100, 1), (250, 0), (101, 1), (260, 0), (99, 1), (1231, 0), (1, 1), (1200, 0)], 2),
        "lead_tail": bursts(rate, [(1300, 0), (500, 1), (37, 0), (700, 1), (1500, 0)], 3),
        "loud": bursts(rate, [(2100, 1)], 4),
        "zeros": np.zeros(2 * rate + 5, dtype=np.int16),
        "short": bursts(rate, [(20, 0), (15, 1)], 5),                         # 35 ms: shorter than most windows
        "minimum": np.full(rate + 3, -32768, dtype=np.int16),
        "straddle": rng.integers(-180, 181, 3 * rate + 7).astype(np.int16),   # rms about 104: windows fall on both sides of T = 103
    }
    # len_ms rounds up and the last windows hold padded zeros: 3 s + 0.7 ms
    c["rounds_up"] = np.concatenate([c["rounds_up"], np.zeros(int(0.7 * rate / 1000), dtype=np.int16)])
    return c
