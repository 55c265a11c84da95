"""CPU tests of "Compare Breaks": the restatement of SequenceMatcher (tests/seqmatch_restatement.py, the rules include/pce.h states for
k_seqmatch) is exactly stdlib ``difflib``; ``break_check.compare_breaks`` on its host path reproduces the reference's own
``pause_comparison_full.csv`` (golden G10, tests/golden/make_goldens_compare_breaks.py); the step's opt-in dispatch; the C ABI."""
import logging
import os
import re
import struct
from difflib import SequenceMatcher

import pytest

import seqmatch_cases as SC
import seqmatch_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def difflib_matches(a, b, autojunk=True):
    return sum(blk.size for blk in SequenceMatcher(None, a, b, autojunk=autojunk).get_matching_blocks())


def bits(x):
    return struct.pack("<d", x)


def test_restatement_equals_difflib_on_every_shape():
    stats = {}
    for name, a, b in SC.shape_cases():
        for autojunk in (True, False):
            assert SR.matches(a, b, autojunk, stats) == difflib_matches(a, b, autojunk), (name, autojunk)
            assert bits(SR.ratio(a, b, autojunk)) == bits(SequenceMatcher(None, a, b, autojunk=autojunk).ratio()), (name, autojunk)
    for a, b in SC.tie_cases():
        assert SR.matches(a, b) == difflib_matches(a, b), (a, b)
        assert bits(SR.ratio(a, b)) == bits(SequenceMatcher(None, a, b).ratio()), (a, b)
    ca, cb = SC.voice(12, 16, seed=5)
    for a in ca:
        for b in cb:
            assert SR.matches(a, b) == difflib_matches(a, b), (a, b)


def test_shapes_reach_what_they_are_meant_to_reach():
    """The cases do exercise the paths they are named for: autojunk changes totals, the stack passes its LDS part, the row its capacity."""
    cases = {name: (a, b) for name, a, b in SC.shape_cases()}
    assert any(SR.matches(a, b, True) != SR.matches(a, b, False) for a, b in cases.values())
    stats = {}
    SR.matches(*cases["deep_stack"], True, stats)
    assert stats["deepest"] > SC.STACK_LDS + 8 and stats["blocks"] == 60
    SR.matches(*cases["deep_stack_lds_only"], True, stats)
    assert stats["deepest"] <= SC.STACK_LDS
    assert len(cases[f"row_{SC.ROW_LDS}_tail"][1]) == SC.ROW_LDS and len(cases[f"row_{SC.ROW_LDS + 1}_tail"][1]) == SC.ROW_LDS + 1
    assert SR.matches(*cases["extension_both_sides"]) == 9 and SR.matches(*cases["only_popular_matches"]) == 4
    a, b = cases["popular_3_inside_run"]; assert SR.popular_flags(b).count(True) == 0
    a, b = cases["popular_4_inside_run"]; assert SR.popular_flags(b).count(True) == 4
    assert SR.matches(*cases["high_bits_differ"]) == 0


def test_alignment_restatement_equals_host_path():
    from prosody_control_french_tts_amd import break_check as BC
    for n, m, seed in ((1, 1, 1), (1, 7, 2), (7, 1, 3), (9, 13, 4), (0, 3, 5), (3, 0, 6)):
        a, b = SC.voice(n, m, seed)
        matches, sim = BC.align_host(a, b)
        assert matches == SR.align(sim, n, m)
        assert all(bits(sim[i][j]) == bits(SR.ratio(a[i], b[j])) for i in range(n) for j in range(m))
    same = ["oui oui"] * 5
    assert BC.align_host(same, same)[0] == SR.align([[1.0] * 5] * 5, 5, 5) == [(i, i) for i in range(5)]


@pytest.mark.parametrize("case", SC.golden_cases(), ids=lambda c: c["name"])
def test_compare_breaks_host_reproduces_the_reference(case, tmp_path):
    from prosody_control_french_tts_amd import break_check as BC
    tg_path, csv_path = SC.write_case(case, str(tmp_path))
    out = tmp_path / "pause_comparison_full.csv"
    df = BC.compare_breaks(tg_path, csv_path, out, tol_ms=case["tol_ms"], engine=None)
    assert out.read_text(encoding="utf-8") == case["pause_comparison_full_csv"]
    assert len(df) == case["n_rows"]
    if case["n_rows"]:
        assert list(df.columns) == ["segment", "syntagme", "nat_voice_ms", "synth_voice_ms", "diff_ms", "ok", "match_quality"]


def test_golden_covers_the_listed_situations():
    from prosody_control_french_tts_amd import break_check as BC
    cases = {c["name"]: c for c in SC.golden_cases()}
    assert {"one_to_one", "more_chunks", "more_blocks", "two_pauses_one_block", "punctuation_accents", "autojunk_block", "repeated_chunks",
            "no_pause_rows"} <= set(cases)
    blocks, _ = BC.speech_blocks([tuple(iv) for iv in cases["autojunk_block"]["intervals"]])
    assert max(len(BC.normalize(b)) for b in blocks) >= 200
    assert cases["no_pause_rows"]["n_rows"] == 0


def test_summary_log_lines_and_low_quality_warning(tmp_path, caplog):
    from prosody_control_french_tts_amd import break_check as BC
    cases = {c["name"]: c for c in SC.golden_cases()}
    tg_path, csv_path = SC.write_case(cases["more_chunks"], str(tmp_path))
    with caplog.at_level(logging.INFO):
        BC.compare_breaks(tg_path, csv_path, tmp_path / "out.csv", tol_ms=5)
    text = [r.getMessage() for r in caplog.records]
    assert text[-4:] == ["Breaks compared: 4", "Within ±5 ms: 1/4 (25.0%)", "Avg |diff|: 175 ms", "Avg match_quality: 0.6"]
    assert "Low match quality for “dort” → “le petit chat dort sur le tapis”: 0.23" in text


def test_step_dispatch_is_opt_in(tmp_path, monkeypatch, caplog):
    """Without ``compare_breaks_on_device`` the step is skipped with the warning, as before; with it ``compare_breaks`` is called, and
    ``strict_steps`` accepts the step."""
    from prosody_control_french_tts_amd import audio_pipeline as AP
    cfg = {"data_dir": "Data", "out_dir": "Out", "steps_to_run": ["Measure & Build SSML", "Final Transcribe", "Compare Breaks"]}
    assert AP.ACCELERATED_STEPS == ("Align+Transcribe", "Measure & Build SSML", "Final Transcribe")

    def run(cfg, name):
        calls = []
        ap = AP.AudioPipeline(name, cfg, base=tmp_path)
        for step in ("measure_prosody_and_build_ssml", "final_transcribe", "compare_breaks"):
            monkeypatch.setattr(ap, step, lambda n=step: calls.append(n))
        ap.run()
        return calls
    with caplog.at_level(logging.WARNING):
        assert run(cfg, "v1") == ["measure_prosody_and_build_ssml", "final_transcribe"]
    assert any('step "Compare Breaks" is outside the accelerated hot path' in r.getMessage() for r in caplog.records)
    assert run(dict(cfg, compare_breaks_on_device=True), "v2") == ["measure_prosody_and_build_ssml", "final_transcribe", "compare_breaks"]
    with pytest.raises(NotImplementedError):
        AP.AudioPipeline("v3", dict(cfg, strict_steps=True), base=tmp_path)
    AP.AudioPipeline("v3", dict(cfg, strict_steps=True, compare_breaks_on_device=True), base=tmp_path)
    with pytest.raises(NotImplementedError):               # the key opens this step alone
        AP.AudioPipeline("v3", dict(cfg, strict_steps=True, compare_breaks_on_device=True, steps_to_run=["Export JSON"]), base=tmp_path)


def test_pipeline_method_uses_the_pipeline_paths(tmp_path, monkeypatch):
    from prosody_control_french_tts_amd import audio_pipeline as AP, break_check as BC
    seen = {}
    ap = AP.AudioPipeline("v1", {"data_dir": "Data", "out_dir": "Out"}, base=tmp_path, engine="the engine")
    monkeypatch.setattr(BC, "compare_breaks", lambda tg, csv, out, tol_ms=5, engine=None: seen.update(tg=tg, csv=csv, out=out, tol=tol_ms, engine=engine) or "table")
    assert ap.compare_breaks(tol_ms=7) == "table"
    assert seen == {"tg": ap.results_dir / "OUT.TextGrid", "csv": ap.bdd_syntagme_synth_csv, "out": ap.results_dir / "pause_comparison_full.csv",
                    "tol": 7, "engine": "the engine"}


def test_header_exports_and_minor_agree():
    from prosody_control_french_tts_amd import engine as E
    header = open(os.path.join(ROOT, "include", "pce.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pce_[a-z0-9_]+)\s*\(", header))
    assert {"pce_seqmatch", "pce_seqmatch_align"} <= declared and declared == set(E.EXPORTS)
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 10
    ids = re.search(r"enum pce_kernel_id \{(.*?)\};", header, re.S).group(1)
    ids = [x for x in re.findall(r"\bPCE_K_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", ids, flags=re.S)) if x != "PCE_K_COUNT"]
    assert ids[-2:] == ["PCE_K_SEQMATCH", "PCE_K_SEQMATCH_ALIGN"] and len(ids) == len(E.KERNEL_IDS)
    assert E.KERNEL_IDS[-2:] == ["k_seqmatch", "k_seqmatch_align"]
    assert SC.MAX_PAIRS == 1 << 26 and SC.ROW_LDS >= 64 and SC.STACK_LDS >= 1
    for name in ("seqmatch_matches", "seqmatch_ratio", "seqmatch_align"):
        assert callable(getattr(E.ProsodyEngine, name))
