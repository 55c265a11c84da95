"""Host side of ``Pipeline/evaluate_voice.py`` (Code/Pipeline/evaluate_voice.ipynb) without a GPU, and the plain restatements the GPU
file (tests/test_gpu_evaluate_voice.py) compares the device against.

The restatements are written from the published source of the ``fastdtw`` package (absent here: parity unpinned) and from the
arithmetic ``include/pce.h`` states for ``pce_dtw_series``: float64 adds and compares in a fixed order, so every comparison of a path
or a distance in these two files is EXACT.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from prosody_control_french_tts_amd import engine as E
from prosody_control_french_tts_amd.Pipeline import evaluate_voice as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EMPTY, NO_PATH = 0, 1, 2


# ----------------------------------------------------------------------------------------------------- restatements
def ref_dtw(a, b, lo=None, hi=None):
    """The dynamic programme of fastdtw's ``__dtw`` on |a_i - b_j|: D[i+1][j+1] = min over the sums (up, left, diagonal) + dt in that
    order, first minimum; cells outside [lo[i], hi[i]) are +inf.  Anti-diagonal by anti-diagonal (the cells of one are independent).
    -> (path int32 [k, 2], dist, status)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return np.zeros((0, 2), np.int32), float("nan"), EMPTY
    lo = np.zeros(n, np.int64) if lo is None else np.asarray(lo, dtype=np.int64)
    hi = np.full(n, m, np.int64) if hi is None else np.asarray(hi, dtype=np.int64)
    D = np.full((n + 1, m + 1), np.inf)
    D[0, 0] = 0.0
    T = np.zeros((n, m), np.uint8)
    for d in range(n + m - 1):
        i = np.arange(max(0, d - m + 1), min(n - 1, d) + 1)
        j = d - i
        dt = np.abs(a[i] - b[j])
        su = D[i, j + 1] + dt; sl = D[i + 1, j] + dt; sd = D[i, j] + dt
        cur = su.copy(); tt = np.zeros(len(i), np.uint8)
        k = sl < cur; cur[k] = sl[k]; tt[k] = 1
        k = sd < cur; cur[k] = sd[k]; tt[k] = 2
        inw = (j >= lo[i]) & (j < hi[i])
        D[i[inw] + 1, j[inw] + 1] = cur[inw]
        T[i[inw], j[inw]] = tt[inw]
    dist = float(D[n, m])
    if not dist < np.inf:
        return np.zeros((0, 2), np.int32), dist, NO_PATH
    path = []
    i, j = n - 1, m - 1
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        t = T[i, j]
        if t != 1:
            i -= 1
        if t != 0:
            j -= 1
    return np.array(path[::-1], dtype=np.int32), dist, OK


def ref_dtw_series(pairs, windows=None):
    """``ProsodyEngine.dtw_series`` on the restatement (what the host tests inject for the device call)."""
    windows = windows if windows is not None else [None] * len(pairs)
    return [ref_dtw(a, b, *(w if w is not None else (None, None))) for (a, b), w in zip(pairs, windows)]


def ref_window_cells(path, len_x, len_y, radius):
    """``__expand_window`` of the fastdtw package as published: sets of cells, then the row scan -> list of (i, j)."""
    path = [tuple(int(v) for v in p) for p in path]
    path_ = set(path)
    for i, j in path:
        for a, b in ((i + a, j + b) for a in range(-radius, radius + 1) for b in range(-radius, radius + 1)):
            path_.add((a, b))
    window_ = set()
    for i, j in path_:
        for a, b in ((i * 2, j * 2), (i * 2, j * 2 + 1), (i * 2 + 1, j * 2), (i * 2 + 1, j * 2 + 1)):
            window_.add((a, b))
    window = []
    start_j = 0
    for i in range(0, len_x):
        new_start_j = None
        if start_j is None:                 # (the package would raise on range(None, ..): only ever the row after an empty LAST row)
            break
        for j in range(start_j, len_y):
            if (i, j) in window_:
                window.append((i, j))
                if new_start_j is None:
                    new_start_j = j
            elif new_start_j is not None:
                break
        start_j = new_start_j
    return window


def cells_to_rows(cells, len_x):
    lo = np.zeros(len_x, np.int32); hi = np.zeros(len_x, np.int32)
    rows = {}
    for i, j in cells:
        rows.setdefault(i, []).append(j)
    for i, js in rows.items():
        assert js == list(range(js[0], js[-1] + 1))                       # one contiguous run per row
        lo[i], hi[i] = js[0], js[-1] + 1
    return lo, hi


def ref_fastdtw(x, y, radius):
    """``__fastdtw``: the recursion as published -> (dist, path)."""
    x = np.asarray(x, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    if len(x) < radius + 2 or len(y) < radius + 2:
        path, dist, _ = ref_dtw(x, y)
        return dist, path
    xs = np.array([(x[i] + x[1 + i]) / 2 for i in range(0, len(x) - len(x) % 2, 2)])
    ys = np.array([(y[i] + y[1 + i]) / 2 for i in range(0, len(y) - len(y) % 2, 2)])
    _, coarse = ref_fastdtw(xs, ys, radius)
    lo, hi = cells_to_rows(ref_window_cells(coarse, len(x), len(y), radius), len(x))
    path, dist, status = ref_dtw(x, y, lo, hi)
    assert status == OK
    return dist, path


def ref_rmse(f0_r, f0_s, radius=25, exact=False):
    f0_r = np.asarray(f0_r, dtype=np.float64); f0_s = np.asarray(f0_s, dtype=np.float64)
    log_r = np.log(f0_r[~np.isnan(f0_r)]); log_s = np.log(f0_s[~np.isnan(f0_s)])
    if log_r.size == 0 or log_s.size == 0:
        return float("nan")
    wp = ref_dtw(log_r, log_s)[0] if exact else ref_fastdtw(log_r, log_s, radius)[1]
    diffs = log_r[wp[:, 0]] - log_s[wp[:, 1]]
    return float(np.sqrt(np.mean(diffs ** 2)))


def ref_edit_distance(a, b):
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def ref_edit_distances(pairs):
    return [ref_edit_distance(a, b) for a, b in pairs]


def random_monotone_path(rng, n, m):
    i = j = 0
    out = [(0, 0)]
    while (i, j) != (n - 1, m - 1):
        moves = [(di, dj) for di, dj in ((1, 0), (0, 1), (1, 1)) if i + di < n and j + dj < m]
        di, dj = moves[rng.integers(len(moves))]
        i, j = i + di, j + dj
        out.append((i, j))
    return np.array(out, dtype=np.int32)


def random_walk(rng, n, scale=0.05):
    return 5.0 + np.cumsum(rng.normal(0.0, scale, n))


WER_CASES = [("le chat dort ici", "le chat dort ici", 0.0), ("le chat dort ici", "le chien dort ici", 0.25), ("bonjour le monde", "", 1.0),
             ("  le   chat \n\n dort  ici ", "le chat dort ici", 0.0), ("un deux trois quatre", "un trois quatre cinq six", 0.75),
             ("a b", "a\tb", 1.0)]            # (a single tab is not a run of whitespace: jiwer's RemoveMultipleSpaces leaves it, "a\tb" is one word)


# ----------------------------------------------------------------------------------------------------- tests
def test_compute_f1_break_hand_cases():
    assert EV.compute_f1_break([], []) == (0.0, 0.0, 0.0)
    assert EV.compute_f1_break([1.0], []) == (0.0, 0.0, 0.0)
    assert EV.compute_f1_break([], [1.0]) == (0.0, 0.0, 0.0)
    assert EV.compute_f1_break([1.0, 2.0], [1.1, 2.1]) == (1.0, 1.0, 1.0)
    # two reference breaks compete for one system break: the first takes it
    f1, prec, rec = EV.compute_f1_break([1.0, 1.2], [1.1])
    assert (prec, rec) == (1.0, 0.5) and f1 == 2 * 0.5 / 1.5
    # abs == tol counts (0.5 and 0.25 are exact in binary), just beyond does not
    assert EV.compute_f1_break([0.5], [0.75], tol=0.25) == (1.0, 1.0, 1.0)
    assert EV.compute_f1_break([0.5], [0.75 + 2 ** -30], tol=0.25) == (0.0, 0.0, 0.0)
    # greedy first match, not best match: 1.0 takes 1.25 (the first within tol), which leaves 1.5 with 0.9 only -- the pairing
    # 1.0 / 0.9, 1.5 / 1.25 would have matched both
    f1, prec, rec = EV.compute_f1_break([1.0, 1.5], [1.25, 0.9], tol=0.3)
    assert (f1, prec, rec) == (0.5, 0.5, 0.5)


def test_compute_wer_word_splitting_and_known_answers():
    for ref, hyp, want in WER_CASES:
        assert EV.compute_wer(ref, hyp, edit_distance=ref_edit_distances) == want, (ref, hyp)
    assert EV.wer_words("  le   chat \n\n dort  ici ") == ["le", "chat", "dort", "ici"]
    seen = []
    got = EV.compute_wer_batch([("a b a", "b a"), ("c a", "a c d")], edit_distance=lambda pairs: seen.extend(pairs) or ref_edit_distances(pairs))
    assert got == [1 / 3, 1.0]
    # one id per distinct word over the whole batch, equal words = equal ids
    assert [p.tolist() for pair in seen for p in pair] == [[0, 1, 0], [1, 0], [2, 0], [0, 2, 3]]
    assert all(p.dtype == np.uint32 for pair in seen for p in pair)
    for empty in ("", "   ", "\n"):
        with pytest.raises(ValueError):
            EV.compute_wer(empty, "un mot", edit_distance=ref_edit_distances)


def test_reduce_by_half_drops_an_odd_tail():
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    assert EV.reduce_by_half(x).tolist() == [1.5, 6.0]
    assert EV.reduce_by_half(x[:4]).tolist() == [1.5, 6.0]
    assert EV.reduce_by_half(x[:1]).tolist() == []


@pytest.mark.parametrize("radius", [0, 1, 25])
def test_expand_window_equals_the_set_based_scan(radius):
    rng = np.random.default_rng(100 + radius)
    for nc, mc in [(1, 1), (1, 9), (7, 1), (6, 6), (13, 40), (40, 13), (60, 75)]:
        for odd_x in (0, 1):
            for odd_y in (0, 1):
                path = random_monotone_path(rng, nc, mc)
                len_x, len_y = 2 * nc + odd_x, 2 * mc + odd_y
                lo, hi = EV.expand_window(path, len_x, len_y, radius)
                want_lo, want_hi = cells_to_rows(ref_window_cells(path, len_x, len_y, radius), len_x)
                live = want_hi > want_lo
                assert np.array_equal(hi > lo, live), (nc, mc, odd_x, odd_y)
                assert np.array_equal(lo[live], want_lo[live]) and np.array_equal(hi[live], want_hi[live]), (nc, mc, odd_x, odd_y)
                assert lo.dtype == np.int32 and hi.dtype == np.int32


@pytest.mark.parametrize("radius", [1, 3, 25])
def test_fastdtw_recursion_equals_the_recursive_restatement(radius):
    rng = np.random.default_rng(7 + radius)
    pairs = [(random_walk(rng, n), random_walk(rng, m)) for n, m in [(1, 1), (2, 3), (40, 40), (41, 77), (130, 97), (radius + 1, 90), (radius + 2, radius + 2)]]
    got = EV.fastdtw_batch(pairs, radius, dtw_series=ref_dtw_series)
    for (x, y), (dist, path) in zip(pairs, got):
        want_dist, want_path = ref_fastdtw(x, y, radius)
        assert dist == want_dist and np.array_equal(path, want_path)
        one = EV.fastdtw(x, y, radius, dtw_series=ref_dtw_series)
        assert one[0] == dist and np.array_equal(one[1], path)


def test_fastdtw_with_a_radius_beyond_the_series_is_the_exact_programme():
    rng = np.random.default_rng(3)
    for n, m in [(30, 50), (64, 17)]:
        x, y = random_walk(rng, n), random_walk(rng, m)
        for radius in (max(n, m), max(n, m) + 5):
            dist, path = EV.fastdtw(x, y, radius, dtw_series=ref_dtw_series)
            want_path, want_dist, _ = ref_dtw(x, y)
            assert dist == want_dist and np.array_equal(path, want_path)
    # and a radius that does recurse stays above the exact distance
    x, y = random_walk(rng, 300), random_walk(rng, 280)
    assert EV.fastdtw(x, y, 2, dtw_series=ref_dtw_series)[0] >= ref_dtw(x, y)[1]


def test_contour_rmse_on_the_restatement():
    rng = np.random.default_rng(11)
    f = 200.0 * 2.0 ** rng.normal(0.0, 0.1, 90)
    g = f.copy(); g[10:20] = np.nan
    kw = dict(dtw_series=ref_dtw_series)
    assert EV.f0_contour_rmse(g, g, **kw) == 0.0
    assert np.isnan(EV.f0_contour_rmse(np.full(5, np.nan), g, **kw)) and np.isnan(EV.f0_contour_rmse(g, np.zeros(0), **kw))
    c = np.full(40, 180.0); c2 = np.full(57, 180.0 * 2.0 ** (1 / 12))
    assert abs(EV.f0_contour_rmse(c, c2, **kw) - np.log(2.0) / 12) <= 1e-12
    h = 210.0 * 2.0 ** rng.normal(0.0, 0.1, 120)
    assert EV.f0_contour_rmse(g, h, **kw) == ref_rmse(g, h)
    assert EV.f0_contour_rmse(g, h, method="exact", **kw) == ref_rmse(g, h, exact=True)
    assert EV.C2_HZ == pytest.approx(65.40639132514966, rel=1e-15) and EV.C6_HZ == pytest.approx(1046.5022612023945, rel=1e-15)


def test_dtw_series_is_declared_exported_and_versioned():
    import __graft_entry__ as ge
    ge.build()
    header = open(os.path.join(ROOT, "include", "pce.h")).read()
    assert re.search(r"\bint pce_dtw_series\s*\(", header) and "pce_dtw_series" in E.EXPORTS
    assert re.search(r"global:\s*pce_\*;", open(os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc", "libpce.map")).read())
    lib = ctypes.CDLL(E.native_library_path())
    assert hasattr(lib, "pce_dtw_series")
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 6
    # the tile the tests import is the tile the kernel was compiled with
    assert int(re.search(r"#define PCE_DTW_SERIES_ROWS (\d+)", header).group(1)) == E.DTW_SERIES_ROWS
    assert int(re.search(r"#define PCE_DTW_SERIES_COLS (\d+)", header).group(1)) == E.DTW_SERIES_COLS
    assert {"k_dtw_series", "k_dtw_series_trace"} <= set(E.KERNEL_IDS)
