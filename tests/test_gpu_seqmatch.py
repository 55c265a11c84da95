"""GPU tests of k_seqmatch / k_seqmatch_align (csrc/pce_seqmatch.hip): the matched totals and the ratios against live stdlib ``difflib``,
the alignment against the Python DP of Code/audioPipeline.py:973-998 (tests/seqmatch_restatement.py) fed with ``difflib`` ratios, and
"Compare Breaks" against the reference's own output (golden G10).  Every comparison is ``==``: integers, and float64 bit patterns."""
import ctypes
import random
from difflib import SequenceMatcher

import numpy as np
import pytest

import seqmatch_cases as SC
import seqmatch_restatement as SR

pytestmark = pytest.mark.gpu

E_INVALID, E_LIMIT = -1, -5


def difflib_matches(a, b, autojunk=True):
    return sum(blk.size for blk in SequenceMatcher(None, a, b, autojunk=autojunk).get_matching_blocks())


def difflib_ratio(a, b, autojunk=True):
    return SequenceMatcher(None, a, b, autojunk=autojunk).ratio()


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))


def diag_pairs(n):
    return [(i, i) for i in range(n)]


# ------------------------------------------------------------------ 1. matched totals against difflib
@pytest.mark.parametrize("autojunk", [True, False])
def test_matches_on_every_shape(engine, autojunk):
    cases = SC.shape_cases()
    a, b = [c[1] for c in cases], [c[2] for c in cases]
    got = engine.seqmatch_matches(a, b, pairs=diag_pairs(len(cases)), autojunk=autojunk)
    want = [difflib_matches(x, y, autojunk) for x, y in zip(a, b)]
    assert got.dtype == np.int32
    wrong = [(c[0], int(g), w) for c, g, w in zip(cases, got, want) if g != w]
    assert not wrong, wrong


def test_matches_on_ties(engine):
    pairs = SC.tie_cases()
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    got = engine.seqmatch_matches(a, b, pairs=diag_pairs(len(pairs)))
    assert got.tolist() == [difflib_matches(x, y) for x, y in pairs]


# ------------------------------------------------------------------ 2. batch indexing
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_batch_sizes(engine, n):
    rng = random.Random(n)
    a = [SC.french(rng, 0, 70) for _ in range(n)]; b = [SC.french(rng, 0, 230) for _ in range(n)]
    got = engine.seqmatch_matches(a, b, pairs=diag_pairs(n))
    assert got.tolist() == [difflib_matches(x, y) for x, y in zip(a, b)]


def test_explicit_pairs_against_all_pairs(engine):
    a, b = SC.voice(7, 9, seed=11)
    full = engine.seqmatch_matches(a, b)
    assert full.shape == (63,)
    assert full.reshape(7, 9).tolist() == [[difflib_matches(x, y) for y in b] for x in a]
    rng = random.Random(3)
    pairs = [(rng.randrange(7), rng.randrange(9)) for _ in range(40)] + [(6, 8), (0, 0), (6, 8)]
    got = engine.seqmatch_matches(a, b, pairs=pairs)
    assert got.tolist() == [int(full[i * 9 + j]) for i, j in pairs]
    for i, j in pairs[:5]:                                  # a pair alone = the same pair inside a batch
        assert engine.seqmatch_matches([a[i]], [b[j]]).tolist() == [int(full[i * 9 + j])]
    assert engine.seqmatch_matches(a, b, pairs=[]).shape == (0,) and engine.seqmatch_matches([], b).shape == (0,)


# ------------------------------------------------------------------ 3. ratios: the bits of difflib's ratio()
def test_ratio_bits(engine):
    cases = SC.shape_cases()
    a, b = [c[1] for c in cases], [c[2] for c in cases]
    got = engine.seqmatch_ratio(a, b, pairs=diag_pairs(len(cases)))
    assert got.dtype == np.float64 and same_bits(got, [difflib_ratio(x, y) for x, y in zip(a, b)])
    va, vb = SC.voice(6, 8, seed=21)
    assert same_bits(engine.seqmatch_ratio(va, vb).reshape(6, 8), [[difflib_ratio(x, y) for y in vb] for x in va])


# ------------------------------------------------------------------ 4. the alignment against the Python DP on difflib ratios
def check_align(engine, a, b):
    n, m = len(a), len(b)
    matches, sim = engine.seqmatch_align(a, b)
    want_sim = np.array([[difflib_ratio(x, y) for y in b] for x in a], dtype=np.float64).reshape(n, m)
    assert matches.dtype == np.int32 and matches.shape[1:] == (2,) and sim.shape == (n, m)
    assert same_bits(sim, want_sim)
    assert [tuple(r) for r in matches.tolist()] == SR.align(want_sim.tolist(), n, m)
    return matches


@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (7, 1), (3, 65), (65, 3), (64, 64), (130, 70)])
def test_align_shapes(engine, n, m):
    rng = random.Random(1000 * n + m)
    base = [SC.french(rng, 8, 40) for _ in range(max(n, m))]
    a = [base[i] if rng.random() < 0.7 else SC.french(rng, 8, 40) for i in range(n)]
    b = [base[j] if rng.random() < 0.7 else SC.french(rng, 8, 40) for j in range(m)]
    check_align(engine, a, b)


def test_align_all_ties_and_nothing_to_match(engine):
    same = ["oui oui"] * 9
    assert check_align(engine, same, same).tolist() == [[i, i] for i in range(9)]     # every sim is 1.0, every comparison a tie
    assert check_align(engine, same[:4], same).shape == (4, 2)
    assert check_align(engine, ["abc", "bca", "cab"] * 3, ["xyz", "zyx"] * 4).shape == (0, 2)      # disjoint alphabets: every sim is 0
    assert check_align(engine, ["", "a", ""], ["", ""]).shape[1] == 2                  # empty strings: sim 1.0 against each other


def test_align_empty_tables(engine):
    for a, b in (([], ["abc", "d"]), (["abc", "d"], []), ([], [])):
        matches, sim = engine.seqmatch_align(a, b)
        assert matches.shape == (0, 2) and sim.shape == (len(a), len(b))


def striped_voice(n, m, rows):
    """n chunks against m short blocks; block j is chunk rows[j], the other chunks are digits (ratio 0) or other words (partial ratios)."""
    rng = random.Random(7 * n + m)
    b = [rng.choice(SC.WORDS) + " " + rng.choice(SC.WORDS) for _ in range(m)]
    a = [rng.choice(["12 345", "6789", "0"]) if rng.random() < 0.5 else rng.choice(SC.WORDS) for _ in range(n)]
    for j, r in enumerate(rows):
        a[r] = b[j]
    return a, b


# k_seqmatch_align sweeps stripes of 1 024 rows and hands each stripe's last row to the next through a global row: more rows than one
# stripe, short strings so that difflib stays cheap, and the chunks worth matching on both sides of the boundaries
@pytest.mark.parametrize("n,m,rows", [(1024, 3, (1021, 1022, 1023)), (1025, 2, (1023, 1024)), (2049, 3, (1023, 1024, 2048)),
                                      (1100, 40, tuple(range(1004, 1084, 2)))], ids=lambda v: str(v) if isinstance(v, int) else "rows")
def test_align_across_row_stripes(engine, n, m, rows):
    a, b = striped_voice(n, m, rows)
    matches = check_align(engine, a, b)
    assert matches[:, 1].tolist() == list(range(m)) and matches[-1, 0] >= 1023       # the case does reach past the first stripe


def test_align_ties_across_row_stripes(engine):
    assert check_align(engine, ["oui"] * 1030, ["oui"] * 5).tolist() == [[i, i] for i in range(5)]
    assert check_align(engine, ["oui"] * 5, ["oui"] * 1030).tolist() == [[i, i] for i in range(5)]
    a = ["123"] * 2050                                      # nothing matches but rows 1023 / 1024 and 2047 / 2048: equal chunks, ties
    a[1023] = a[1024] = a[2047] = a[2048] = "oui"
    assert check_align(engine, a, ["oui", "oui", "oui"]).tolist() == [[1023, 0], [1024, 1], [2047, 2]]


# ------------------------------------------------------------------ 5. the step
@pytest.mark.parametrize("case", SC.golden_cases(), ids=lambda c: c["name"])
def test_compare_breaks_device_reproduces_the_reference(engine, case, tmp_path):
    from prosody_control_french_tts_amd import break_check as BC
    tg_path, csv_path = SC.write_case(case, str(tmp_path))
    out = tmp_path / "pause_comparison_full.csv"
    BC.compare_breaks(tg_path, csv_path, out, tol_ms=case["tol_ms"], engine=engine)
    assert out.read_text(encoding="utf-8") == case["pause_comparison_full_csv"]


def test_compare_breaks_device_equals_host_on_a_voice(engine, tmp_path):
    from prosody_control_french_tts_amd import break_check as BC
    chunks, blocks = SC.voice(60, 80, seed=77)
    rng = random.Random(78)
    for k in range(0, 60, 3):                               # every third chunk is (most of) a block, so that the alignment has something to find
        chunks[k] = blocks[k + 5][:90]
    intervals, t = [], 0.0
    for blk in blocks:
        for w in blk.split():
            intervals.append([t, t + 0.25, w]); t += 0.25
        d = rng.choice([0.1, 0.2, 0.35]); intervals.append([t, t + d, ""]); t += d
    rows = []
    for k, c in enumerate(chunks):
        rows.append({"segment": f"segment_ph{k // 6}", "syntagme": c, "pause": 0, "ssml": ""})
        rows.append({"segment": f"segment_ph{k // 6}", "syntagme": None, "pause": rng.choice([100, 200, 350]), "ssml": ""})
    case = {"intervals": intervals, "csv_rows": rows, "csv_columns": ["segment", "syntagme", "pause", "ssml"]}
    tg_path, csv_path = SC.write_case(case, str(tmp_path))
    host, dev = tmp_path / "host.csv", tmp_path / "device.csv"
    BC.compare_breaks(tg_path, csv_path, host, engine=None)
    BC.compare_breaks(tg_path, csv_path, dev, engine=engine)
    assert dev.read_text(encoding="utf-8") == host.read_text(encoding="utf-8")
    assert len(host.read_text(encoding="utf-8").splitlines()) == 61


# ------------------------------------------------------------------ 6. error codes
def raw_seqmatch(engine, a_off, b_off, pair_a=None, pair_b=None, n_pairs=None, n_a=None, n_b=None):
    ao = np.asarray([0] if a_off is None else a_off, dtype=np.int64); bo = np.asarray([0] if b_off is None else b_off, dtype=np.int64)
    chars = np.full(64, 97, dtype=np.uint32)
    n_a = len(ao) - 1 if n_a is None else n_a; n_b = len(bo) - 1 if n_b is None else n_b
    pa = None if pair_a is None else np.asarray(pair_a, dtype=np.int32)
    pb = None if pair_b is None else np.asarray(pair_b, dtype=np.int32)
    n_pairs = (n_a * n_b if pa is None else len(pa)) if n_pairs is None else n_pairs
    out = np.zeros(max(min(n_pairs, 1024), 1), dtype=np.int32)
    return engine._lib.pce_seqmatch(engine._ctx, chars.ctypes.data, ao.ctypes.data if a_off is not None else None, n_a, chars.ctypes.data,
                                    bo.ctypes.data if b_off is not None else None, n_b, pa.ctypes.data if pa is not None else None,
                                    pb.ctypes.data if pb is not None else None, n_pairs, 1, out.ctypes.data)


def test_error_codes(engine):
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4]) == 0
    assert raw_seqmatch(engine, [0, 3, 2], [0, 4]) == E_INVALID                       # decreasing offsets
    assert raw_seqmatch(engine, [0, 3], [0, 4, 1]) == E_INVALID
    assert raw_seqmatch(engine, [1, 3], [0, 4]) == E_INVALID                          # offsets start at 0
    assert raw_seqmatch(engine, None, [0, 4], n_a=1) == E_INVALID                     # null offsets
    assert raw_seqmatch(engine, [0, 3], None, n_b=1) == E_INVALID
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], [0, 2], [0, 0]) == E_INVALID       # pair index past its table
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], [0, 1], [0, 1]) == E_INVALID
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], [0, -1], [0, 0]) == E_INVALID
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], [0, 1], None, n_pairs=2) == E_INVALID           # one index array without the other
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], n_pairs=3) == E_INVALID            # all pairs of 2 x 1 are not 3
    assert raw_seqmatch(engine, [0, 3, 5], [0, 4], [1, 0], [0, 0]) == 0
    side = int(SC.MAX_PAIRS ** 0.5) + 1                                               # the stated limit: PCE_SEQMATCH_MAX_PAIRS
    assert side * side > SC.MAX_PAIRS
    empty = np.zeros(side + 1, dtype=np.int64)
    assert raw_seqmatch(engine, empty, empty) == E_LIMIT
    assert raw_seqmatch(engine, [0, 1 << 30], [0, 4]) == E_LIMIT                      # a string of 2^30 elements
    assert raw_seqmatch(engine, [0, 1 << 26], [0, 1 << 26]) == E_LIMIT                # 4 waves x (4 + 16) x 2^26 bytes of scratch > SCRATCH_MAX
    k = ctypes.c_int32(-1)
    buf = np.zeros(side, dtype=np.int32)
    rc = engine._lib.pce_seqmatch_align(engine._ctx, None, empty.ctypes.data, side, None, empty.ctypes.data, side, 1, None, buf.ctypes.data,
                                        buf.ctypes.data, ctypes.byref(k))
    assert rc == E_LIMIT
    from prosody_control_french_tts_amd import PceError
    with pytest.raises(PceError):
        engine.seqmatch_matches(["a"], ["b"], pairs=[(0, 1)])
    assert engine.seqmatch_matches(["abc"], ["abd"]).tolist() == [2]                  # the context still works after the refusals


def test_profile_ids_count_swept_cells(engine):
    a, b = SC.voice(5, 6, seed=9)
    engine.profile_enable(True); engine.profile_reset()
    try:
        engine.seqmatch_align(a, b)
        prof = engine.profile()
    finally:
        engine.profile_enable(False)
    cells, stats = 0, {}
    for x in a:
        for y in b:
            SR.matches(x, y, True, stats); cells += stats["cells"]
    assert prof["k_seqmatch"]["launches"] == 1 and prof["k_seqmatch"]["flops"] == cells
    assert prof["k_seqmatch_align"]["launches"] == 1 and prof["k_seqmatch_align"]["flops"] == 30
