"""Language detection, the host side: the language token range of the tokenizer, ``Aligners.decoding.detect_language``, and
``transcribe_batch(language=None)`` over a scripted engine (the loop under test is host logic; the kernel behind ``whisper_detect_language``
is checked in tests/test_gpu_langid.py).  Also: the entry point is declared, exported and versioned."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from prosody_control_french_tts_amd import engine as E
from prosody_control_french_tts_amd.Aligners import decoding as DEC, transcribe as TR
from prosody_control_french_tts_amd.Aligners.tokenizer import LANGUAGES, WhisperTokenizer, special_token_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("num_languages", [99, 100])
def test_language_tokens_follow_the_special_token_order(num_languages):
    tk = WhisperTokenizer.toy([b" b", b"on"], num_languages=num_languages)
    names = special_token_names(num_languages)
    assert names[1] == "<|startoftranscript|>" and names[2:2 + num_languages] == [f"<|{c}|>" for c in LANGUAGES[:num_languages]]
    assert names[2 + num_languages] == "<|translate|>"
    assert tk.all_language_tokens == tuple(range(tk.sot + 1, tk.sot + 1 + num_languages))
    assert tk.all_language_codes == tuple(LANGUAGES[:num_languages]) and len(tk.all_language_codes) == num_languages
    assert [tk.special_names[t] for t in tk.all_language_tokens] == names[2:2 + num_languages]
    assert tk.all_language_tokens[-1] + 1 == tk.translate
    assert (tk.all_language_codes[-1] == "yue") == (num_languages == 100)
    for code, t in zip(tk.all_language_codes, tk.all_language_tokens):
        assert tk.language_token(code) == t and tk.sot_sequence(code) == (tk.sot, t, tk.transcribe)


def test_word_splitting_follows_the_language_given():
    tk = WhisperTokenizer.toy([], language="fr")
    toks = [ord("a"), ord("b"), tk.eot]
    assert tk.split_to_word_tokens(toks) == tk.split_to_word_tokens(toks, "fr") == tk.split_tokens_on_spaces(toks)
    assert tk.split_to_word_tokens(toks, "zh") == tk.split_tokens_on_unicode(toks) != tk.split_tokens_on_spaces(toks)


class ScriptedEngine:
    """Answers the calls of ``transcribe_batch`` (vad=None) from a script and writes down their order."""

    def __init__(self, tk, detected):
        self.tk, self.detected, self.calls, self.prompts = tk, detected, [], []

    def upload(self, clips, rate):
        self.n = len(clips)

    def logmel_run_at(self, n_mels, seeks):
        self.calls.append("logmel")

    def whisper_encode_run(self):
        self.calls.append("encode")

    def whisper_num_encoded(self):
        return self.n

    def whisper_sample_keys(self, keys=None):
        pass

    def whisper_detect_language(self, sot, lang_begin, n_lang):
        self.calls.append("detect")
        assert (sot, lang_begin, n_lang) == (self.tk.sot, self.tk.sot + 1, self.tk.num_languages)
        probs = np.full((self.n, n_lang), 0.5 / (n_lang - 1), dtype=np.float32)
        ids = np.asarray([self.tk.language_token(c) for c in self.detected], dtype=np.int32)
        probs[np.arange(self.n), ids - lang_begin] = 0.5
        return ids, probs

    def whisper_decode_step_ex(self, token_lists, sample_begin, eot, timestamp_begin, vocab_mask, max_initial_timestamp_index=None, temperature=0.0,
                               seed=0, probe_token=-1, no_cache=False):
        self.calls.append("step")
        n = len(token_lists)
        return np.full(n, eot, np.int32), np.zeros(n, np.float32), np.zeros(n, np.float32)

    def whisper_decode_loop(self, token_lists, sample_begin, eot, timestamp_begin, vocab_mask, max_new, max_initial_timestamp_index=None, temperature=0.0,
                            seed=0, probe_token=-1, no_cache=False, check_every=4):
        self.calls.append("loop")
        self.prompts.append([list(map(int, p)) for p in token_lists])
        row = [timestamp_begin, ord("a"), ord("b"), timestamp_begin + 50, eot]            # <|0.00|>ab<|1.00|>: one segment, the window consumed
        return np.asarray([row] * len(token_lists), np.int32), np.full((len(token_lists), len(row)), -0.1, np.float32), None

    def whisper_align(self, token_lists, num_frames, sot_len, head_mask=None, **kw):
        self.calls.append("align")
        self.align_tokens = [list(map(int, t)) for t in token_lists]
        assert sot_len == 3
        return [{"text_indices": np.arange(len(t) - sot_len - 1), "time_indices": 10 * np.arange(len(t) - sot_len - 1)} for t in token_lists]


def _run(language, detected=("fr", "zh", "de")):
    tk = WhisperTokenizer.toy([], language="fr")
    eng = ScriptedEngine(tk, detected)
    model = types.SimpleNamespace(dims={"n_mels": 80}, text_dims={"n_vocab": tk.n_vocab, "n_text_ctx": 64}, alignment_heads=None)
    clips = [np.zeros(32000, np.int16)] * 3
    opts = TR.TranscribeOptions(language=language, vad=None, detect_disfluencies=False, sample_len=8)
    return tk, eng, TR.transcribe_batch(eng, model, tk, clips, opts)


def test_transcribe_detects_once_before_decoding_and_prompts_per_clip():
    tk, eng, res = _run(None)
    assert eng.calls.count("detect") == 1
    at = eng.calls.index("detect")
    assert eng.calls[at - 1] == "encode" and "step" not in eng.calls[:at] and "loop" not in eng.calls[:at] and "align" not in eng.calls[:at]
    assert "loop" in eng.calls[at:] and "step" in eng.calls[at:]
    assert eng.prompts[0] == [list(tk.sot_sequence(c)) for c in ("fr", "zh", "de")]
    assert [t[:3] for t in eng.align_tokens] == [list(tk.sot_sequence(c)) for c in ("fr", "zh", "de")]
    assert [r["language"] for r in res] == ["fr", "zh", "de"]
    # word splitting follows the clip's language: "ab" is one word in French and German, two (split on unicode points) in Chinese
    assert [[w["text"] for s in r["segments"] for w in s["words"]] for r in res] == [["ab"], ["a", "b"], ["ab"]]
    assert all(r["text"] == "ab" for r in res)


def test_an_explicit_language_never_detects(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("detect_language called although a language was given")
    monkeypatch.setattr(DEC, "detect_language", refuse)
    tk, eng, res = _run("fr")
    assert "detect" not in eng.calls and "loop" in eng.calls
    assert eng.prompts[0] == [list(tk.sot_sequence("fr"))] * 3 and [r["language"] for r in res] == ["fr"] * 3
    assert [[w["text"] for s in r["segments"] for w in s["words"]] for r in res] == [["ab"]] * 3
    assert TR.TranscribeOptions().language == "fr"                                       # the default is unchanged


def test_detect_language_needs_language_tokens():
    tk = WhisperTokenizer.toy([], num_languages=0, language=None)
    assert tk.all_language_tokens == () and tk.all_language_codes == ()
    with pytest.raises(ValueError, match="language tokens"):
        DEC.detect_language(ScriptedEngine(tk, ()), tk)
    tk = WhisperTokenizer.toy([], language="fr")
    eng = ScriptedEngine(tk, ("ja", "fr")); eng.n = 2
    codes, probs = DEC.detect_language(eng, tk)
    assert codes == ["ja", "fr"] and [max(p, key=p.get) for p in probs] == codes and set(probs[0]) == set(tk.all_language_codes)
    assert abs(sum(probs[1].values()) - 1.0) <= 1e-6


def test_detect_language_is_declared_exported_and_versioned():
    import __graft_entry__ as ge
    ge.build()
    header = open(os.path.join(ROOT, "include", "pce.h")).read()
    assert re.search(r"\bint pce_whisper_detect_language\s*\(", header) and "pce_whisper_detect_language" in E.EXPORTS
    assert int(re.search(r"#define PCE_API_MINOR (\d+)", header).group(1)) >= 11
    lib = ctypes.CDLL(E.native_library_path())
    lib.pce_api_minor.restype = ctypes.c_int
    assert lib.pce_api_minor() >= 11
    assert hasattr(lib, "pce_whisper_detect_language")
    assert hasattr(E.ProsodyEngine, "whisper_detect_language")
