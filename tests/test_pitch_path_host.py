"""tests/pitch_restatement.py against the CPU oracle and against hand-computed expectations; no GPU.

``path_finder`` on the oracle's own candidates returns the oracle's f0 and strength bit for bit on every clip of every stage-A set of
tests/test_gpu_pitch_stages.py (oracle/pce_oracle.c runs Pitch_pathFinder with scalar loops and libm's log, the restatement with numpy: the two
agree on every decision, and the track is a copy of candidates).  The exact-tie and class-boundary cases of stage B are pinned by the numbers in
``pitch_cases.exact_cases``.  Every stage-B batch clears its gap precondition here already, so a seed that does not is found without a GPU."""
import time

import numpy as np
import pytest

import pitch_cases as PC
from pitch_restatement import gap_bound, path_finder


@pytest.mark.parametrize("form_id", list(PC.FORMS))
def test_restatement_equals_the_oracle_on_its_own_candidates(form_id):
    worst = np.inf
    for name, c, w in PC.oracle(form_id):
        if w is None:
            continue
        pl = w["plan"]
        r = path_finder(w["cand_f"], w["cand_s"], w["ncand"], w["intensity"], pl.dt, PC.params(form_id), ceiling=pl.ceiling)
        assert np.array_equal(r["f0"], w["f0"]) and np.array_equal(r["strength"], w["strength"]), (form_id, name)
        assert r["min_gap"] > gap_bound(len(w["ncand"]), r["max_abs_delta"]), (form_id, name, r["min_gap"])
        worst = min(worst, r["min_gap"])
    print(form_id, "smallest gap with twins collapsed:", worst)


@pytest.mark.parametrize("form_id", list(PC.FORMS))
def test_stage_a_sets_hold_their_edges_and_no_marginal_replacement(form_id):
    cnt = PC.assert_stage_a_preconditions(form_id)
    print(form_id, cnt, "smallest replacement margin:", PC.min_replace_margin(form_id))


def test_the_sustained_tone_is_one_run_longer_than_the_lds_back_pointers():
    c = PC.sustained_tone()
    w = PC.O.pitch_ac(c.astype(np.float64) / 32768.0, 1.0 / 16000, 0.5 / 16000, PC.params("16k-150"), want_candidates=True)
    assert PC.longest_run(w["ncand"]) == len(w["ncand"]) > 1024


def test_exact_ties_and_class_boundaries_by_hand():
    p, dt, _ = PC.batches()["exact"]
    for name, (cf, cs, n, inten), f0, psi in PC.exact_cases():
        r = path_finder(cf, cs, n, inten, dt, p)
        assert np.array_equal(r["f0"], f0), (name, r["f0"], f0)
        for (t, c), want in psi.items():
            assert r["psi"][t, c] == want, (name, t, c, r["psi"][t, c], want)
    by_name = {c[0]: path_finder(*c[1], dt, p) for c in PC.exact_cases()}
    assert by_name["tie-at-threshold"]["end_gap"] == 0.0                       # an exact tie between two candidates that are no twins
    assert by_name["above-ceiling"]["gap"][1, 1] == np.inf                     # every predecessor is a twin of the winner
    assert by_name["duplicates-mid-run"]["gap"][1, 1] > 0.2                    # the duplicate does not count against its twin


def test_twins_do_not_hide_a_real_near_tie():
    """Two distinct voiced candidates 1e-15 apart in strength: the gap is that difference, not the distance to the third."""
    cf, cs, n, inten = PC.blank(2)
    n[:] = [4, 2]
    cf[0, 1:4] = [200.0, 200.0, 400.0]; cs[0, 1:4] = [0.8, 0.8 * (1 + 1e-15), 0.1]
    cf[1, 1] = 200.0; cs[1, 1] = 0.9
    r = path_finder(cf, cs, n, inten, 0.01, PC.path_params())
    assert r["psi"][1, 1] == 2 and 0.0 < r["gap"][1, 1] < 2e-15


@pytest.mark.parametrize("name", list(PC.batches()))
def test_every_stage_b_batch_clears_its_gap_precondition(name):
    exempt = {"tie-at-threshold", "just-above-threshold"}                      # exact arithmetic on both sides: 0.45 against 0.45 (+ 1 ulp)
    names = [c[0] for c in PC.exact_cases()] if name == "exact" else [None] * len(PC.expected(name))
    for label, r in zip(names, PC.expected(name)):
        if label not in exempt:
            assert r["min_gap"] > r["bound"], (name, label, r["min_gap"], r["bound"])


def test_intended_shapes_of_the_batches():
    B = PC.batches()
    runs = [PC.longest_run(s[2]) for s in B["ladder"][2]]
    assert runs[:len(PC.LADDER)] == list(PC.LADDER) and runs[len(PC.LADDER):2 * len(PC.LADDER)] == list(PC.LADDER)
    n = B["run-lists-alternating"][2][0][2]
    starts = np.flatnonzero(n > 1)
    per_list = np.bincount((starts >> 2) & 63, minlength=64)                  # k_pitch_delta's list of a run start
    assert len(starts) == 10000 and per_list.min() > 64                      # every list holds more runs than one pass of the grid takes
    assert all(s[2][0] > 1 for s in B["run-lists-one-frame-slices"][2]) and len(B["run-lists-one-frame-slices"][2]) == 4096
    assert max(int(s[2].max()) for s in B["counts-16"][2]) == 16 and max(int(s[2].max()) for s in B["counts"][2]) == 15
    voiced = [int(np.count_nonzero(r["f0"] > 0)) for r in PC.expected("medians")]
    assert voiced[3:9] == [0, 1, 2, 14, 14, 30] and voiced[9:11] == [256, 255] and voiced[0] > 8192 and voiced[1] > 8192
    assert len(set(PC.expected("medians")[8]["f0"])) == 1                     # all voiced values equal
    lens = [len(s[2]) for s in B["medians"][2]]
    assert lens[:2] == [16384, 16385] and lens[-2:] == [16385, 16390]


def test_a_slice_of_40000_frames_takes_well_under_a_second():
    p, dt, (s,) = PC.batches()["median-40000"]
    t = time.process_time()                                                   # CPU time of this process: a loaded machine does not count
    path_finder(*s, dt, p)
    assert time.process_time() - t < 1.0
