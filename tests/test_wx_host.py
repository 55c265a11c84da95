"""CPU tests of the whisperX alignment's host side: the restatement the GPU tests compare with (tests/wx_restatement.py) against the same
lines written with torch's CPU operators (bit for bit) and against hand-made answers, the host rules of Aligners/wx_segments.py,
Aligners/whisperX.create_textgrid, and the library's declaration of pce_wx_align."""
import ctypes
import os
import re

import numpy as np
import pytest

import wx_restatement as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def torch_trellis(e, tok, blank):
    """whisperx's get_trellis / get_wildcard_emission as published, on torch's CPU operators."""
    import torch
    em, tk = torch.from_numpy(e), torch.tensor(tok, dtype=torch.long)
    T, J = em.shape[0], len(tok)
    tr = torch.zeros((T, J))
    tr[1:, 0] = torch.cumsum(em[1:, blank], 0)
    tr[0, 1:] = -float("inf")
    tr[-J + 1:, 0] = float("inf")

    def wild(frame, tks):
        shut = frame.clone()
        shut[blank] = -float("inf")
        return torch.where(tks < 0, shut.max(), frame[tks.clamp(min=0)])

    for t in range(T - 1):
        tr[t + 1, 1:] = torch.maximum(tr[t, 1:] + em[t, blank], tr[t, :-1] + wild(em[t], tk[1:]))
    return tr.numpy()


def seeded_cases():
    for seed in range(48):
        V = (8, 41)[seed % 2]
        yield seed, WR.make_case(seed, T=12 + 3 * seed, J=1 + seed % 17, V=V, blank=(0, V - 1)[(seed // 2) % 2], quantised=seed % 3 == 0,
                                 wild=(0.0, 0.15, 1.0)[(seed // 4) % 3]), (0, V - 1)[(seed // 2) % 2]


# ------------------------------------------------------------------ the trellis
def test_trellis_equals_the_torch_cpu_operators_bit_for_bit():
    n = 0
    for _, (e, tok), blank in seeded_cases():
        assert np.array_equal(bits(WR.trellis(e, tok, blank)), bits(torch_trellis(e, tok, blank)))
        n += 1
    for T, J in ((1, 1), (1, 3), (2, 5), (5, 5), (6, 5), (4, 9)):         # J = 1, T = 1, J > T, J = T
        for wild in (0.0, 1.0):
            e, tok = WR.make_case(100 + T * 16 + J, T, J, 8, wild=wild)
            assert np.array_equal(bits(WR.trellis(e, tok, 0)), bits(torch_trellis(e, tok, 0)))
            n += 1
    assert n == 60


def test_trellis_at_1500_frames():
    e, tok = WR.make_case(7, 1500, 400, 41, blank=40, wild=0.15)
    want = torch_trellis(e, tok, 40)
    got = WR.trellis(e, tok, 40)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(got[-1, -1]) and np.isinf(got[1500 - 400 + 1:, 0]).all() and np.isfinite(got[:1500 - 400 + 1, 0]).all()


def test_a_sequential_fp32_prefix_differs():
    """Column 0 is a cumsum with an fp64 accumulator: a sequential fp32 sum is another function, so the rule is not vacuous."""
    import torch
    differ = 0
    for seed in range(40):
        e = WR.log_softmax_rows(np.random.default_rng(seed), 300, 8)
        col = e[1:, 0]
        seq = np.empty_like(col)
        acc = np.float32(0.0)
        for k, v in enumerate(col):
            acc = np.float32(acc + v)
            seq[k] = acc
        want = torch.cumsum(torch.from_numpy(col.copy()), 0).numpy()
        assert np.array_equal(bits(np.cumsum(col.astype(np.float64)).astype(np.float32)), bits(want))
        differ += not np.array_equal(bits(seq), bits(want))
    assert differ >= 5


# ------------------------------------------------------------------ the back-track
def test_backtrack_known_answers():
    e = WR.log_softmax_rows(np.random.default_rng(3), 5, 4)
    # J = 1: the loop never runs; every frame carries token 0 on the blank's emission, the score is the wedge's +inf
    r = WR.align(e, [2], 1, 2)
    assert r["status"] == 0 and r["path_tok"].tolist() == [0] * 5 and np.array_equal(bits(r["path_lp"]), bits(e[:, 1])) and r["score"] == np.inf
    # T = 1, J = 2: the one beam stands on frame 0 with j > 0 and is dropped
    assert WR.backtrack(WR.trellis(e[:1], [1, 2], 0), e[:1], [1, 2], 0, 2) is None
    assert WR.align(e[:1], [1, 2], 0, 2)["status"] == 2 and WR.align(e[:3], [1, 2, 3, 1], 0, 5)["status"] == 2          # J > T
    # J = T: the path changes at every step; a change's lp is the emission of the token being LEFT, the last frame's the blank's
    tok = [3, 1, -1, 2, 1]
    r = WR.align(e, tok, 0, 2)
    assert r["status"] == 0 and r["path_tok"].tolist() == [0, 1, 2, 3, 4]
    wm = WR.rowmax(e, 0)
    assert np.array_equal(bits(r["path_lp"]), bits([e[0, 1], wm[1], e[2, 2], e[3, 1], e[4, 0]]))
    assert WR.align(e[:0], tok, 0, 2)["status"] == 1 and WR.align(e, [], 0, 2)["status"] == 1


def test_backtrack_tie_that_only_a_stable_order_resolves():
    """All emissions equal: every finite trellis cell of a frame holds the same value, so each step's candidates tie and only their emission
    order decides.  With W = 1 the first candidate is always the first beam's STAY: the path stays on the last token until the trellis forces
    a change (the cell above is -inf, which is no candidate).  An unstable order, or one that prefers the change, gives another path."""
    T, J, V = 7, 3, 4
    e = np.full((T, V), np.float32(-1.5))
    tr = WR.trellis(e, [1, 2, 3], 0)
    assert tr[4, 1] == tr[4, 2] and tr[3, 1] == tr[3, 2]
    for W in (1, 2, 5):
        tok, _ = WR.backtrack(tr, e, [1, 2, 3], 0, W)
        assert tok.tolist() == [0, 1, 2, 2, 2, 2, 2]


def test_backtrack_is_monotone_and_the_beam_width_is_observable():
    differ = {(1, 2): 0, (2, 5): 0, (1, 5): 0}
    for _, (e, tok), blank in seeded_cases():
        if len(tok) > e.shape[0]:
            continue
        tr = WR.trellis(e, tok, blank)
        paths = {}
        for W in (1, 2, 5):
            got = WR.backtrack(tr, e, tok, blank, W)
            assert got is not None
            p = got[0]
            assert p[0] == 0 and p[-1] == len(tok) - 1 and set(np.diff(p).tolist()) <= {0, 1}
            paths[W] = p
        for a, b in differ:
            differ[(a, b)] += not np.array_equal(paths[a], paths[b])
    assert all(v >= 1 for v in differ.values()), differ


# ------------------------------------------------------------------ the host rules
DICTIONARY = {"[pad]": 0, "|": 1, "a": 2, "b": 3, "c": 4, "é": 5, "'": 6}


def test_clean_segment():
    from prosody_control_french_tts_amd.Aligners import wx_segments as S
    chars, cdx, tokens = S.clean_segment("  Ab cé7 ", DICTIONARY, "fr")
    assert chars == ["a", "b", "|", "c", "é", "*"] and cdx == [2, 3, 4, 5, 6, 7] and tokens == [2, 3, 1, 4, 5, -1]
    assert S.clean_segment("   ", DICTIONARY, "fr") == ([], [], [])
    chars, _, tokens = S.clean_segment("a b", DICTIONARY, "ja")                   # no "|" for a language without spaces: the space is unknown
    assert chars == ["a", "*", "b"] and tokens == [2, -1, 3]
    assert S.clean_segment("*", dict(DICTIONARY, **{"*": 7}), "fr")[2] == [-1]      # the placeholder itself is always the wildcard


def test_merge_repeats():
    from prosody_control_french_tts_amd.Aligners import wx_segments as S
    lp = np.log(np.array([0.5, 0.25, 1.0, 0.5, 0.5, 0.125], dtype=np.float32))
    got = S.merge_repeats([0, 0, 1, 2, 2, 2], lp, "a|b")
    assert [(g[0], g[1], g[2]) for g in got] == [("a", 0, 2), ("|", 2, 3), ("b", 3, 6)]
    assert [round(g[3], 6) for g in got] == [0.375, 1.0, 0.375]


def test_assemble_words_and_rounding():
    from prosody_control_french_tts_amd.Aligners import wx_segments as S
    text = " ab 77 c "
    seg = {"start": 1.0, "end": 2.0, "text": text}
    seg["clean_char"], seg["clean_cdx"], _ = S.clean_segment(text, DICTIONARY, "fr")
    assert "".join(seg["clean_char"]) == "ab|**|c"
    chars = [("a", 0, 3, 0.91249), ("b", 3, 4, 0.5), ("|", 4, 5, 0.1), ("*", 5, 6, 0.25), ("*", 6, 8, 0.75), ("|", 8, 9, 0.1), ("c", 9, 11, 0.33349)]
    out = S.assemble(seg, chars, 11, "fr")                                         # ratio = 1 / 10
    assert out["text"] == text and out["start"] == 1.0 and out["end"] == 2.1
    assert out["words"] == [{"word": "ab", "start": 1.0, "end": 1.4, "score": 0.706},          # (0.912 + 0.5) / 2
                            {"word": "77", "start": 1.5, "end": 1.8, "score": 0.5},            # a word of unknown characters only: the wildcard aligns it
                            {"word": "c", "start": 1.9, "end": 2.1, "score": 0.333}]
    # thirds: round(x * ratio + t1, 3)
    out = S.assemble(dict(seg, end=1.5), chars, 4, "fr")
    assert out["words"][0]["start"] == 1.0 and out["words"][0]["end"] == round(4 * (0.5 / 3) + 1.0, 3) == 1.667
    # a word with no aligned character keeps its text and has no times; the segment's times come from what did align
    seg2 = dict(seg, clean_cdx=[1, 2])
    out = S.assemble(seg2, chars[:2], 11, "fr")
    assert out["words"] == [{"word": "ab", "start": 1.0, "end": 1.4, "score": 0.706}, {"word": "77"}, {"word": "c"}]
    assert (out["start"], out["end"]) == (1.0, 1.4)
    out = S.assemble(dict(seg, clean_cdx=[]), [], 11, "fr")
    assert (out["start"], out["end"]) == (1.0, 2.0) and out["words"] == [{"word": "ab"}, {"word": "77"}, {"word": "c"}]
    # a language without spaces: every character is a word
    out = S.assemble({"start": 0.0, "end": 1.0, "text": "ab", "clean_cdx": [0, 1]}, [("a", 0, 1, 1.0), ("b", 1, 3, 0.5)], 3, "ja")
    assert out["words"] == [{"word": "a", "start": 0.0, "end": 0.5, "score": 1.0}, {"word": "b", "start": 0.5, "end": 1.5, "score": 0.5}]


def test_create_textgrid(tmp_path, capsys):
    from prosody_control_french_tts_amd.Aligners import whisperX as X
    from prosody_control_french_tts_amd.textgrid_io import read_textgrid
    words = [{"word": "un", "start": 0.5, "end": 1.0}, {"word": "sans"}, {"word": "deux", "start": 0.9, "end": 1.5},
             {"text": "trois", "start_time": 2.0, "end_time": 2.5}, {"word": "nul", "start": 3.0, "end": 3.0}, {"word": "fin", "start": 2.75, "end": 3.0}]
    path = tmp_path / "a.TextGrid"
    X.create_textgrid(words, 4.0, str(path))
    said = capsys.readouterr().out
    assert "sans" in said and "nul" in said and said.count("left out") == 2
    tier = read_textgrid(str(path)).tiers[0]
    assert tier.name == "Mots"
    assert [iv for iv in tier.intervals if iv[2]] == [(0.5, 1.0, "un"), (1.0, 1.5, "deux"), (2.0, 2.5, "trois"), (2.75, 3.0, "fin")]    # M moved 0.9 to 1.0
    text = path.read_text(encoding="utf-8")
    assert 'name = "Mots"' in text and "xmax = 4.0" in text and 'text = "deux"' in text and text.count("intervals [") == 8
    X.create_textgrid([], 0.0, str(path))
    assert "intervals: size = 0" in path.read_text(encoding="utf-8")
    assert X.blank_id(DICTIONARY) == 0 and X.blank_id({"a": 0, "<pad>": 3}) == 3 and X.blank_id({"a": 1}) == 0
    assert X.main(["only", "two"]) == 1


# ------------------------------------------------------------------ the library
def test_header_and_library_declare_wx_align():
    from prosody_control_french_tts_amd import engine as E
    header = open(os.path.join(ROOT, "include", "pce.h")).read()
    assert re.search(r"\bint pce_wx_align\s*\(", header) and "pce_wx_params" in header and "PCE_WX_NO_PATH = 2" in header
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 20
    assert int(re.search(r"#define PCE_WX_MAX_TOKENS (\d+)", header).group(1)) == E.WX_MAX_TOKENS
    assert int(re.search(r"#define PCE_WX_MAX_BEAM (\d+)", header).group(1)) == E.WX_MAX_BEAM
    assert (E.WX_OK, E.WX_EMPTY, E.WX_NO_PATH) == (0, 1, 2)
    lib = ctypes.CDLL(E.native_library_path())
    assert hasattr(lib, "pce_wx_align") and "pce_wx_align" in E.EXPORTS
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 20
    assert ctypes.sizeof(E.WxParams) == 16
    k = E.KERNEL_IDS.index("k_ctc")
    assert E.KERNEL_IDS[k - 3:k] == ["k_wx_rowmax", "k_wx_trellis", "k_wx_backtrack"] and E.KERNEL_IDS[k - 4] == "k_w2v_tail"
    assert hasattr(E.ProsodyEngine, "wx_align")
