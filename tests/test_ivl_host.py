"""CPU tests of the aligner evaluation (``whisper_testing/splitting.py``): with ``engine=None`` the module reproduces every case of golden
G11, which tests/golden/make_goldens_aligner_eval.py recorded from the reference's own functions; the bitmap restatement equals a plain
scan by the reference's rule on every shape the GPU tests use; three mutations of the restatement each break a golden case; the C ABI."""
import os
import re
import warnings

import pytest

import ivl_cases as IC
from prosody_control_french_tts_amd.whisper_testing import splitting as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = IC.GOLDEN["align"]
STATS = IC.GOLDEN["stats"]


def align_pairs(case, engine=None):
    return [[g["i"], p["i"]] for g, p in SP.align_intervals(case["gold"], case["pred"], engine=engine)]


def multilevel(case, engine=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # np.mean([]) -> nan warns, in the reference as here
        mock = SP.create_mock_segments_from_intervals(case["pred"], case["audio_duration"])
        segments = mock if case["segments"] is None else case["segments"]
        return mock, SP.calculate_multilevel_stats(case["gold"], case["pred"], segments, case["audio_duration"], engine=engine)


@pytest.mark.parametrize("case", ALIGN, ids=lambda c: c["name"])
def test_align_intervals_reproduces_the_reference(case):
    assert align_pairs(case) == case["pairs"]


@pytest.mark.parametrize("case", STATS, ids=lambda c: c["name"])
def test_multilevel_stats_reproduce_the_reference(case):
    mock, stats = multilevel(case)
    assert mock == case["mock_segments"]                   # adds, subtractions and comparisons of the inputs: exact
    assert SP.create_mock_segments_from_intervals(case["pred"], case["audio_duration"], 20) == case["mock_segments_20s"]
    IC.same_stats(stats, case["stats"])


@pytest.mark.parametrize("case", IC.GOLDEN["textgrids"], ids=lambda c: c["name"])
def test_parse_textgrid_reproduces_the_reference(case, tmp_path):
    path = tmp_path / "case.TextGrid"
    path.write_text(case["text"], encoding="utf-8")
    assert SP.parse_textgrid(str(path)) == case["intervals"]


def test_golden_holds_the_listed_situations():
    """The conditions on G11's inputs, read off the golden itself."""
    align = {c["name"]: c for c in ALIGN}
    stats = {c["name"]: c for c in STATS}
    texts = [iv["text"] for c in ALIGN + STATS for iv in c["gold"] + c["pred"]]
    assert {"aujourd'hui", "l'eau", "est-ce", "Bonjour,"} <= set(texts)
    norm = SP.normalize_text
    assert any(norm(iv["text"]) == "" for c in ALIGN for iv in c["gold"]) and any(norm(iv["text"]) == "" for c in ALIGN for iv in c["pred"])
    assert any(" " in norm(t) for t in texts) and any(ord(ch) > 0xFFFF for t in texts for ch in t)
    # repeated words: a later gold interval falls to a lower class than an earlier one of the same text
    c = align["collision_falls_to_lower_class"]
    classes = IC.scan([norm(g["text"]) for g in c["gold"]], [norm(p["text"]) for p in c["pred"]])
    assert [k for _, k in classes] == [3, 2, 2, 2] and len({g["text"] for g in c["gold"]}) == 1
    seeded = align["seeded_300"]
    assert len(seeded["pred"]) != len(seeded["gold"]) and 0 < len(seeded["pairs"]) < len(seeded["gold"])      # dropped, inserted, substituted
    span = stats["interval_spans_two_windows"]
    assert any(iv["start"] < 15 < iv["end"] for iv in span["gold"])
    w = stats["all_windows_empty"]["stats"]
    assert w["window_15s"]["window_count"] > 0 and w["window_15s"]["mean_MAE_start"] != w["window_15s"]["mean_MAE_start"]      # nan
    assert w["entire_audio"]["count"] > 0
    assert stats["empty_pred"]["pred"] == [] and stats["empty_pred"]["stats"]["entire_audio"]["MAE_start"] == float("inf")
    assert all(c["audio_duration"] % 15 != 0 for c in STATS)
    assert stats["shorter_than_a_second"]["stats"]["window_15s"]["window_count"] == 0
    run = stats["run_longer_than_a_segment"]              # segments that close on their length, at both limits
    assert len(run["mock_segments"]["segments"]) == 2 and len(run["mock_segments_20s"]["segments"]) == 3
    assert run["mock_segments"] != run["mock_segments_20s"] and all(iv["duration"] == 0.5 for iv in run["gold"])       # (no gap anywhere)
    assert max(len(c["gold"]) + len(c["pred"]) for c in STATS) <= 2000             # the n of the float bound (ivl_cases.REL)


def test_restatement_equals_the_plain_scan_on_the_kernel_shapes():
    for make in (IC.bitmap_edges, IC.text_cases, IC.membership_cases, IC.random_batch):
        tables, problems = make()
        assert IC.as_pairs(SP.interval_match_host(tables, problems)) == IC.expect(tables, problems), make.__name__
    tables, problems = IC.random_batch()
    classes = {k for result in IC.expect(tables, problems) for _, k in result}
    assert classes == {0, 1, 2, 3} and len(problems) == 200 and len(tables) == 8
    # collisions: the same prediction is the best of two gold rows of one problem, and the later one gets another or none
    assert any(len({tables[t][0][g] for g in gold}) < len(gold) for t, gold, _ in problems)


def golden_fails():
    """Cases of G11 the module, as it is patched now, does not reproduce."""
    failed = [c["name"] for c in ALIGN if align_pairs(c) != c["pairs"]]
    for c in STATS:
        try:
            IC.same_stats(multilevel(c)[1], c["stats"])
        except AssertionError:
            failed.append(c["name"])
    return failed


def test_mutations_of_the_restatement_break_the_golden(monkeypatch):
    """The golden is not vacuous: the tie rule, the empty substring and the per-call claims each decide a recorded case."""
    assert golden_fails() == []
    with monkeypatch.context() as m:                       # the tie rule takes the last instead of the first
        m.setattr(SP, "_first_bit", lambda x: x.bit_length() - 1)
        assert "ties_first_wins" in golden_fails()
    with monkeypatch.context() as m:                       # the empty string is not a substring
        m.setattr(SP, "_is_substring", lambda a, b: a != "" and a in b)
        assert "punctuation_gold_claims_first" in golden_fails()
    with monkeypatch.context() as m:                       # the claimed set is shared across windows
        shared = [0]
        m.setattr(SP, "_new_claims", lambda: shared)
        assert {"french_mock_segments", "seeded_300"} & set(golden_fails())
    assert golden_fails() == []


def test_batch_form_and_summary_csv(tmp_path):
    """``evaluate_textgrids`` over several TextGrids equals ``evaluate_nemo_textgrid`` one by one; ``run_evaluation`` writes the
    reference's summary columns, duration from the WAV header."""
    import wave
    case = {c["name"]: c for c in STATS}["seeded_300"]

    def grid(name, intervals):
        path = tmp_path / f"{name}.TextGrid"
        path.write_text("".join(f'        intervals [{n + 1}]:\n            xmin = {max(iv["start"], 0.0)!r}\n            xmax = {iv["end"]!r}\n'
                                f'            text = "{iv["text"]}"\n' for n, iv in enumerate(intervals)), encoding="utf-8")
        return path
    gold_path = grid("gold", case["gold"])
    preds = {"one": grid("one", case["pred"]), "two": grid("two", case["gold"]), "none": grid("none", [])}
    gold = SP.parse_textgrid(gold_path)
    assert [iv["text"] for iv in gold] == [iv["text"] for iv in case["gold"]]
    duration = case["audio_duration"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        batch = SP.evaluate_textgrids(gold_path, preds, duration)
        assert [r["model"] for r in batch] == ["one", "two"] and all(r["processing_time"] == 0 for r in batch)
        for r in batch:
            alone = SP.evaluate_nemo_textgrid(preds[r["model"]], gold, duration)
            assert alone["model"] == "NeMo"
            IC.same_stats({k: v for k, v in r.items() if k != "model"}, {k: v for k, v in alone.items() if k != "model"}, bits=True)
        assert SP.evaluate_nemo_textgrid(preds["none"], gold, duration) is None
        assert batch[1]["entire_audio"]["ARR"] == 1.0 and batch[1]["entire_audio"]["MAE_start"] == 0.0
        wav = tmp_path / "audio.wav"
        with wave.open(str(wav), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000); w.writeframes(b"\0\0" * int(8000 * 2.5))
        assert SP.audio_duration_of(wav) == 2.5 and SP.audio_duration_of(31) == 31
        df = SP.run_evaluation(gold_path, preds, duration, tmp_path / "out")
    assert list(df.columns) == ["model", "time_s", "entire_ARR", "entire_MAE_start", "entire_MAE_end", "entire_MAE_duration", "entire_RMSE_start",
                                "entire_RMSE_end", "entire_RMSE_duration", "win15s_mean_ARR", "win15s_mean_MAE_start", "win15s_mean_MAE_duration",
                                "sent_mean_ARR", "sent_mean_MAE_start", "sent_mean_MAE_duration", "word_mean_start_error", "word_mean_duration_error",
                                "word_median_start_error", "word_max_start_error"]
    assert df["model"].tolist() == ["one", "two"] and df["entire_ARR"].tolist() == [r["entire_audio"]["ARR"] for r in batch]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["one_evaluation_summary.csv", "two_evaluation_summary.csv"]
    assert (tmp_path / "out" / "two_evaluation_summary.csv").read_text().splitlines()[0].split(",") == list(df.columns)


def test_header_ids_and_engine_agree():
    from prosody_control_french_tts_amd import engine as E
    header = open(os.path.join(ROOT, "include", "pce.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pce_[a-z0-9_]+)\s*\(", header))
    assert "pce_ivl_match" in declared and declared == set(E.EXPORTS)
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 24
    ids = re.search(r"enum pce_kernel_id \{(.*?)\};", header, re.S).group(1)
    ids = [x for x in re.findall(r"\bPCE_K_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", ids, flags=re.S)) if x != "PCE_K_COUNT"]
    k = ids.index("PCE_K_IVL_CLASSES")
    assert ids[k - 1:k + 3] == ["PCE_K_CREPE_VITERBI", "PCE_K_IVL_CLASSES", "PCE_K_IVL_CLAIM", "PCE_K_W2V"] and len(ids) == len(E.KERNEL_IDS)
    assert E.KERNEL_IDS[k:k + 2] == ["k_ivl_classes", "k_ivl_claim"]
    lib = E.load_library()
    lib.pce_kernel_name.restype = __import__("ctypes").c_char_p
    assert [lib.pce_kernel_name(i).decode() for i in range(len(E.KERNEL_IDS))] == E.KERNEL_IDS and lib.pce_api_minor() >= 24
    names = re.search(r"static const char \*names\[PCE_K_COUNT\] = \{(.*?)\};", open(os.path.join(
        ROOT, "prosody-control-french-tts_amd", "csrc", "pce_ctx.hip"), encoding="utf-8").read(), re.S).group(1)
    assert re.findall(r'"([^"]+)"', names) == E.KERNEL_IDS
    assert int(re.search(r"#define PCE_IVL_MAX_PRED \(1 << (\d+)\)", header).group(1)) == 18
    assert callable(E.ProsodyEngine.interval_match)
