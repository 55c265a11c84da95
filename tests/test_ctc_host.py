"""CPU tests of the CTC forced alignment's host side: the restatement the GPU tests compare with (tests/ctc_restatement.py) against
exhaustive enumeration, the post-processing of Aligners/ctc_segments.py on hand-made paths, Aligners/CTCFA.txt_to_textgrid against the
reference's logic, Aligners/ctc_emissions.hf_emissions on a random-init Wav2Vec2ForCTC, and the library's declaration of pce_ctc_align."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import ctc_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log_softmax_rows(rng, T, V, quantised=False):
    x = rng.standard_normal((T, V)).astype(np.float32) * (0.5 if quantised else 2)       # (a narrow spread: few distinct quantised values)
    lp = (x - np.log(np.sum(np.exp(x.astype(np.float64)), axis=1, keepdims=True))).astype(np.float32)
    return (np.round(lp * 4) / 4).astype(np.float32) if quantised else lp


def all_targets(V, max_l, blank=0):
    labels = [v for v in range(V) if v != blank]
    for L in range(1, max_l + 1):
        yield from itertools.product(labels, repeat=L)


# ------------------------------------------------------------------ the restatement
def test_restatement_finds_the_best_path_by_enumeration():
    """Every T <= 7, V = 4, L <= 3 (repeats included): the restatement's score is the maximum over all valid state sequences, in float32
    bits, and its path is one of the maximisers."""
    rng = np.random.default_rng(5)
    checked = 0
    for tg in all_targets(4, 3):
        tg = np.array(tg)
        lab = CR.state_labels(tg, 0)
        for T in range(1, 8):
            if T < len(tg) + CR.n_repeats(tg):
                continue
            lp = log_softmax_rows(rng, T, 4)
            got = CR.forced_align(lp, tg)
            scores = {seq: CR.path_score(lp, lab[list(seq)]) for seq in CR.valid_state_paths(T, tg)}
            best = max(scores.values())
            assert got["status"] == CR.OK and got["score"] == best, (tg, T)
            assert CR.path_score(lp, got["path"]) == best
            checked += 1
    assert checked == 189                     # 39 target sequences, every T from L + R to 7


def test_shortest_clip_has_one_path():
    rng = np.random.default_rng(6)
    for tg in ([1], [1, 2, 3], [3, 3, 3], [1, 1, 2, 2, 1], [2, 1, 1, 1, 3]):
        tg = np.array(tg)
        T = len(tg) + CR.n_repeats(tg)
        assert len(CR.valid_state_paths(T, tg)) == 1
        lp = log_softmax_rows(rng, T, 4)
        got = CR.forced_align(lp, tg)
        (seq,) = CR.valid_state_paths(T, tg)
        assert got["status"] == CR.OK and got["path"].tolist() == CR.state_labels(tg, 0)[list(seq)].tolist()
        assert CR.forced_align(lp[:-1], tg)["status"] == (CR.TOO_SHORT if T > 1 else CR.EMPTY)
    assert CR.forced_align(np.zeros((0, 4), np.float32), [1])["status"] == CR.EMPTY
    assert CR.forced_align(np.zeros((3, 4), np.float32), [])["status"] == CR.EMPTY


def scalar_rule(lp, tg, blank=0):
    """The recurrence, one state at a time with the strict comparisons spelt out -> (final score, labels of the
    path, number of choices made between two equal finite candidates)."""
    T, S = len(lp), 2 * len(tg) + 1
    lab = [blank if i % 2 == 0 else tg[i // 2] for i in range(S)]
    ninf = np.float32(-np.inf)
    alpha = [ninf] * S
    alpha[0], alpha[1] = lp[0][blank], lp[0][tg[0]]
    back, ties = [[0] * S], 0
    for t in range(1, T):
        new, bp = [ninf] * S, [0] * S
        for i in range(S):
            x0 = alpha[i]
            x1 = alpha[i - 1] if i >= 1 else ninf
            x2 = alpha[i - 2] if (i % 2 == 1 and i != 1 and tg[i // 2] != tg[i // 2 - 1]) else ninf
            finite = [x for x in (x0, x1, x2) if x > ninf]
            ties += len(set(finite)) < len(finite)
            if x2 > x1 and x2 > x0:
                chosen, bp[i] = x2, 2
            elif x1 > x0 and x1 > x2:
                chosen, bp[i] = x1, 1
            else:
                chosen, bp[i] = x0, 0
            new[i] = np.float32(chosen + lp[t][lab[i]])
        alpha = new; back.append(bp)
    i = S - 1 if alpha[S - 1] > alpha[S - 2] else S - 2
    score, seq = alpha[i], []
    for t in range(T - 1, -1, -1):
        seq.append(i); i -= back[t][i]
    return score, [lab[j] for j in reversed(seq)], ties


def test_tie_rule_on_quantised_emissions():
    """Multiples of 0.25 make ties everywhere.  The vectorised restatement follows the scalar rule on them, path and score; with ties the
    rule is NOT the maximiser any more (x1 == x2 > x0 keeps x0), and the cases where it falls short of the enumerated maximum are kept."""
    rng = np.random.default_rng(7)
    ties = short = 0
    for tg in all_targets(4, 3):
        tg = np.array(tg)
        lab = CR.state_labels(tg, 0)
        for T in range(len(tg) + CR.n_repeats(tg), 8):
            lp = log_softmax_rows(rng, T, 4, quantised=True)
            assert np.array_equal(lp * 4, np.round(lp * 4))
            got = CR.forced_align(lp, tg)
            score, path, n_ties = scalar_rule(lp, tg.tolist())
            assert got["status"] == CR.OK and got["score"] == score and got["path"].tolist() == path, (tg, T)
            scores = [CR.path_score(lp, lab[list(seq)]) for seq in CR.valid_state_paths(T, tg)]
            assert got["score"] <= max(scores) and CR.path_score(lp, got["path"]) == got["score"]
            ties += n_ties
            short += bool(got["score"] < max(scores))
    print(f"tied choices {ties}, cases below the enumerated maximum {short}")
    assert ties > 0 and short > 0              # the inputs do exercise the rule, and some ties cost the maximum
    # targets [1, 2], frame 1, state 3: x0 = alpha[3] = -inf, x1 = alpha[2] = -inf, x2 = alpha[1]; frame 2, state 3 with x1 == x2 > x0
    lp = np.zeros((3, 3), np.float32)
    lp[0] = [-1.0, -1.0, -9.0]; lp[1] = [0.0, 0.0, -5.0]; lp[2] = [-9.0, -9.0, 0.0]
    got = CR.forced_align(lp, [1, 2])
    # frame 1: alpha = [-1, -1, -1, -6, -inf]; frame 2, state 3: x0 = -6, x1 = alpha[2] = -1, x2 = alpha[1] = -1: a tie above x0 -> x0 is kept
    assert got["score"] == np.float32(-6.0) and got["path"].tolist() == [1, 2, 2]


# ------------------------------------------------------------------ ctc_segments
def _segments():
    from prosody_control_french_tts_amd.Aligners import ctc_segments as S
    return S


def test_merge_repeats():
    S = _segments()
    path = [0, 0, 3, 3, 3, 0, 4, 4]
    assert S.merge_repeats(path) == [(0, 0, 1), (3, 2, 4), (0, 5, 5), (4, 6, 7)] == CR.merge_repeats(path)
    assert S.merge_repeats([]) == [] and S.merge_repeats([7]) == [(7, 0, 0)]


def test_spans_share_blanks():
    S = _segments()
    # leading blank (frames 0-1), word [1, 2] (2-4), a 3-frame blank (5-7), word [3] (8), a 4-frame blank (9-12), word [1] (13), trailing blank (14-15)
    path = [0, 0, 1, 1, 2, 0, 0, 0, 3, 0, 0, 0, 0, 1, 0, 0]
    seg = S.merge_repeats(path)
    spans = S.get_spans([[1, 2], [3], [1]], seg, 0)
    # odd blank 5..7: previous word ends at floor(6) = 6, next starts at int(6) = 6; even blank 9..12: 10.5 -> 10 and 10
    assert [(s.first_frame, s.last_frame) for s in spans] == [(0, 6), (6, 10), (10, 15)]
    fs = np.log(np.linspace(0.2, 0.95, len(path))).astype(np.float32)
    rows = S.word_times(["ab", "c", "a"], [[1, 2], [3], [1]], spans, seg, fs, blank=0, stride_ms=20)
    assert [(r["start"], r["end"], r["text"]) for r in rows] == [(0.0, 0.12, "ab"), (0.12, 0.2, "c"), (0.2, 0.3, "a")]
    assert rows[0]["confidence"] == pytest.approx(math.exp(float(np.mean(fs[2:5].astype(np.float64)))))
    assert rows[1]["confidence"] == pytest.approx(float(np.exp(np.float64(fs[8]))))
    # no blank between two words: nothing is shared
    spans = S.get_spans([[1], [2]], S.merge_repeats([1, 1, 2]), 0)
    assert [(s.first_frame, s.last_frame) for s in spans] == [(0, 1), (2, 2)]


def test_spans_with_a_star_before_every_word_and_an_emptied_word():
    S = _segments()
    vocab = {"a": 1, "b": 2, "c": 3}
    text, tokens = S.tokenize("Ab, ÉÉ c!", vocab, "segment")
    assert text == ["<star>", "ab", "<star>", "éé", "<star>", "c"] and tokens == [[4], [1, 2], [4], [], [4], [3]]
    path = [4, 4, 1, 0, 2, 4, 0, 4, 4, 3, 3, 0]       # star, a, blank, b, star, blank, star, c, blank
    seg = S.merge_repeats(path)
    spans = S.get_spans(tokens, seg, 0)
    # "éé" lost every character: a zero-length span at the segment of the star before it (the previous entry's last segment)
    assert (spans[3].seg_first, spans[3].seg_last) == (spans[2].seg_first, spans[2].seg_last)
    rows = S.word_times(text, tokens, spans, seg, np.zeros(len(path), np.float32), blank=0, n_samples=12 * 320)
    assert [r["text"] for r in rows] == ["ab", "éé", "c"]                  # the stars are dropped
    assert rows[0]["start"] == 2 * 20 / 1000 and rows[0]["end"] == 4 * 20 / 1000
    assert math.isnan(rows[1]["confidence"]) and rows[0]["confidence"] == 1.0
    assert rows[2]["start"] == 9 * 20 / 1000 and rows[2]["end"] == 11 * 20 / 1000     # the last entry takes the whole trailing blank
    text, tokens = S.tokenize("a b", vocab, "edges")
    assert text == ["<star>", "a", "b", "<star>"] and tokens == [[4], [1], [2], [4]]
    assert S.default_stride_ms(16000 * 7, 349) == math.ceil(7000 / 349) == 21
    with pytest.raises(NotImplementedError):
        S.tokenize("a", vocab, romanize=True)
    with pytest.raises(ValueError):
        S.get_spans([[1], [2]], S.merge_repeats([1, 0, 3]), 0)


def test_spans_without_segments():
    S = _segments()
    assert S.merge_repeats(np.zeros(0, np.int32)) == []
    spans = S.get_spans([[], []], [], 0)                           # every word emptied, a path without frames
    assert [(s.first_frame, s.last_frame) for s in spans] == [(0, 0), (0, 0)]
    rows = S.word_times(["é", "è"], [[], []], spans, [], np.zeros(0, np.float32), blank=0, stride_ms=20)
    assert [(r["start"], r["end"]) for r in rows] == [(0.0, 0.0)] * 2 and all(math.isnan(r["confidence"]) for r in rows)
    with pytest.raises(ValueError):
        S.get_spans([[], [1]], [], 0)
    spans = S.get_spans([[], [1]], S.merge_repeats([0, 1, 1]), 0)  # a leading emptied word sits at the first segment
    assert (spans[0].seg_first, spans[0].seg_last) == (0, 0) and (spans[1].first_frame, spans[1].last_frame) == (0, 2)


# ------------------------------------------------------------------ CTCFA.txt_to_textgrid
def reference_logic(lines):
    """What Code/Aligners/CTCFA.py:45-71 keeps of a word file -> (intervals, messages)."""
    kept, said = [], []
    for line in lines:
        if not line.strip():
            continue
        parts = line.strip().split(":")
        if len(parts) != 2:
            said.append(f"Incorrect line format: {line}"); continue
        se = parts[0].strip().split("-")
        if len(se) != 2:
            said.append(f"Incorrect time format in line: {line}"); continue
        try:
            a, b = float(se[0].strip()), float(se[1].strip())
        except ValueError:
            said.append(f"Time conversion error in line: {line}"); continue
        if a == b:
            b += 0.005
        if a > b or any(x < b and a < y for x, y, _ in kept):      # textgrid's Interval / IntervalTier.add raise ValueError
            said.append(f"Time conversion error in line: {line}"); continue
        kept.append((a, b, parts[1].strip()))
    return kept, said


def test_txt_to_textgrid_matches_the_reference_logic(tmp_path, capsys):
    from prosody_control_french_tts_amd.Aligners import CTCFA
    from prosody_control_french_tts_amd.textgrid_io import read_textgrid
    lines = ["0.1-0.5: bonjour\n", "\n", "0.5-0.5: le\n", "0.62-1.0: monde\n", "sans deux points\n", "1.0-1.2: a: b\n", "1.2: seul\n",
             "1.3-x: faux\n", "0.7-0.9: chevauche\n", "  1.5 - 2.25 :  fin  \n"]
    src = tmp_path / "a.txt"
    src.write_text("".join(lines), encoding="utf-8")
    CTCFA.txt_to_textgrid(str(src), str(tmp_path / "a.TextGrid"))
    said = capsys.readouterr().out
    kept, want_said = reference_logic(lines)
    assert said == "".join(m + "\n" for m in want_said) and len(want_said) == 5
    tg = read_textgrid(tmp_path / "a.TextGrid")
    assert len(tg.tiers) == 1 and tg.tiers[0].name == "Mots"
    assert [iv for iv in tg.tiers[0].intervals if iv[2] != ""] == kept
    assert kept[1] == (0.5, 0.505, "le") and tg.max_time == 2.25
    assert CTCFA.preprocess_text(' «Oui», dit-il: "non" (peut_être)!  ') == "Oui dit il non peut être"


class RestatementEngine:
    """Stands in for ProsodyEngine in process_files: ctc_align through the CPU restatement."""
    device = 0

    def ctc_align(self, emissions, targets, blank=0, n_frames=None):
        em = emissions.numpy()
        return [CR.forced_align(em[k, :n_frames[k]], tg, blank) for k, tg in enumerate(targets)]


def test_process_files_on_the_host_and_a_clip_without_a_path(tmp_path, capsys):
    """process_files end to end with given emissions and the restatement in the engine's place: the word file beside each recording, the
    TextGrid, the reference's messages; a clip with fewer frames than characters gets an empty word file and an empty ``Mots`` tier."""
    import wave
    torch = pytest.importorskip("torch")
    from prosody_control_french_tts_amd.Aligners import CTCFA, ctc_segments
    from prosody_control_french_tts_amd.textgrid_io import read_textgrid
    rng = np.random.default_rng(11)
    vocab = {ch: i + 1 for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz")}
    audio, trans, out = tmp_path / "a", tmp_path / "t", tmp_path / "o"
    audio.mkdir(); trans.mkdir()
    texts = {"long": "Oui, le chat dort.", "short": "anticonstitutionnellement"}
    frames = {"long": 40, "short": 12}
    for name in ("long", "short", "orphan"):
        with wave.open(str(audio / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(np.zeros(frames.get(name, 5) * 320, np.int16).tobytes())
        if name in texts:
            (trans / f"{name}.txt").write_text(texts[name], encoding="utf-8")
    em = np.zeros((2, 40, 28), np.float32)                         # sorted file order: long, (orphan left out), short; column 27 is the star
    em[:, :, :27] = log_softmax_rows(rng, 80, 27).reshape(2, 40, 27)
    rows = CTCFA.process_files(str(audio), str(trans), str(out), "fra", "segment", False, engine=RestatementEngine(), vocab=vocab,
                               emissions=(torch.from_numpy(em), np.array([40, 12], np.int32)))
    said = capsys.readouterr().out
    assert said.count("Missing transcription file: ") == 1 and said.count("Processed file : ") == 2
    assert [r["text"] for r in rows["long.wav"]] == ["oui", "le", "chat", "dort"] and rows["short.wav"] == []
    assert (audio / "short.txt").read_text(encoding="utf-8") == "" and len((audio / "long.txt").read_text(encoding="utf-8").splitlines()) == 4
    tg = read_textgrid(out / "long.TextGrid")
    words = [iv for iv in tg.tiers[0].intervals if iv[2] != ""]
    assert [iv[2] for iv in words] == ["oui", "le", "chat", "dort"] and all(0 <= a < b <= 40 * 0.02 for a, b, _ in words)
    empty = read_textgrid(out / "short.TextGrid")
    assert [t.name for t in empty.tiers] == ["Mots"] and empty.tiers[0].intervals == []
    with pytest.raises(NotImplementedError):
        CTCFA.process_files(str(audio), str(trans), str(out), "fra", "segment", True, engine=RestatementEngine(), vocab=vocab, emissions=(None, None))


# ------------------------------------------------------------------ hf_emissions
@pytest.fixture(scope="module")
def tiny_ctc_model():
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = transformers.Wav2Vec2Config(vocab_size=32, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                      conv_dim=(16,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    return transformers.Wav2Vec2ForCTC(cfg).eval()


def test_hf_emissions_windows(tiny_ctc_model):
    import torch
    from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE
    rng = np.random.default_rng(3)
    long_clip = (rng.standard_normal(70 * 16000) * 3000).astype(np.int16)
    short_clip = (rng.standard_normal(16000 * 3 + 123) * 3000).astype(np.int16)
    em, n_frames = CE.hf_emissions(tiny_ctc_model, [long_clip, short_clip], "cpu")
    # the context rule: every 30 s window keeps 30 * 50 frames, the frames of the padding behind the clip leave
    assert n_frames.tolist() == [3 * 1500 - CE.time_to_frame(20.0), 1500 - CE.time_to_frame((30 * 16000 - len(short_clip)) / 16000)]
    with torch.inference_mode():
        whole = tiny_ctc_model(torch.from_numpy(long_clip.astype(np.float32) / 32768.0)[None]).logits.shape[1]
    assert whole == (len(long_clip) - 400) // 320 + 1 and 0 <= n_frames[0] - whole <= 1       # 50 frames a second against the encoder's own count
    assert em.shape == (2, int(n_frames.max()), 33) and em.dtype == torch.float32 and em.is_contiguous()
    for c in range(2):
        rows = em[c, :n_frames[c]]
        assert torch.all(rows[:, 32] == 0)                                                    # the star column
        assert torch.allclose(torch.exp(rows[:, :32].double()).sum(dim=1), torch.ones(n_frames[c], dtype=torch.float64), atol=1e-5)
    assert torch.all(em[1, n_frames[1]:] == 0)
    # content: the second 30 s of the long clip are the model's own output for samples 28 s .. 62 s (the window with its 2 s of context on both
    # sides) with the context's 100 frames cut from its front.  The same fp32 forward, alone instead of in a batch of four windows: 1e-4 on
    # log-probabilities of magnitude log(32) is a hundred times what reordered fp32 sums of this depth differ by.  (Not compared with the
    # unwindowed forward: the encoder's group norm and its attention span the whole input, so a window's frames differ from it by design.)
    x = torch.from_numpy(long_clip.astype(np.float32) / 32768.0)
    with torch.inference_mode():
        alone = tiny_ctc_model(x[28 * 16000:62 * 16000][None]).logits[0]
    assert alone.shape[0] == 1699
    assert torch.allclose(em[0, 1500:3000, :32], torch.log_softmax(alone[100:1600].float(), dim=-1), atol=1e-4, rtol=0)


# ------------------------------------------------------------------ the library
def test_header_and_library_declare_ctc_align():
    from prosody_control_french_tts_amd import engine as E
    header = open(os.path.join(ROOT, "include", "pce.h")).read()
    assert re.search(r"\bint pce_ctc_align\s*\(", header) and "pce_ctc_params" in header and "PCE_CTC_NO_PATH = 3" in header
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 15
    assert int(re.search(r"#define PCE_CTC_REG_STATES (\d+)", header).group(1)) == E.CTC_REG_STATES
    lib = ctypes.CDLL(E.native_library_path())
    assert hasattr(lib, "pce_ctc_align") and "pce_ctc_align" in E.EXPORTS
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 15
    assert ctypes.sizeof(E.CtcParams) == 16
    assert E.KERNEL_IDS[-5:-2] == ["k_ctc", "k_ctc_general", "k_ctc_trace"]
