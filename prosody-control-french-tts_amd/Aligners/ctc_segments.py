"""From a CTC alignment path to word times: the text side and the post-processing of the ``ctc-forced-aligner`` command that
``Code/Aligners/CTCFA.py`` runs per file (host, numpy only; the path itself comes from ``ProsodyEngine.ctc_align``).

The command's package (and MMS ``align_utils``, which it follows) is third party and absent: its rules are restated from the published
source, parity unpinned.  A *segment* is a run of equal labels of the path, ``(label, first_frame, last_frame)``
with the last frame inclusive.  A *word* is the list of the vocabulary indices of its characters; ``<star>`` is a one-label word whose
label is the extra emission column appended after the model's vocabulary.

The rule of ``get_spans``: a word's span runs from the segment of its first character to the segment of its last.  A blank segment
directly before it is shared with the previous word at ``int((start + end) / 2)`` (the first word takes all of it); a blank segment
directly after it is shared at ``floor((start + end) / 2)`` (the last word takes all of it).  A word with no characters left in the
vocabulary gets a zero-length span at the previous word's last segment (at the first segment when no word precedes it).  A path
without frames has no segments: then every word must be emptied, and each gets the span ``(0, 0)``."""
from __future__ import annotations

import math
import re
from typing import NamedTuple

import numpy as np

STAR = "<star>"
SAMPLE_RATE = 16000


class Span(NamedTuple):
    first_frame: int      # with the share of a blank segment before the word
    last_frame: int       # with the share of a blank segment after it (inclusive)
    seg_first: int        # the segment of the word's first character
    seg_last: int         # ... of its last


def preprocess_text(text: str) -> str:
    """``preprocess_text`` of Code/Aligners/CTCFA.py:39-42: the punctuation the reference blanks becomes a space, runs of white
    space collapse, the ends are stripped."""
    blanked = "".join(" " if ch in '.,!?;:"\\()-_«»' else ch for ch in text)
    return re.sub(r"\s+", " ", blanked).strip()


def tokenize(text: str, vocab: dict, star_frequency: str = "segment", star_index: int | None = None, romanize: bool = False):
    """Lower-case, ``preprocess_text``, split into words, words into characters; characters outside ``vocab`` (character -> index) are
    dropped.  ``star_frequency``: ``"segment"`` puts ``<star>`` before every word, ``"edges"`` at both ends of the text.  ``star_index``
    (default ``max(vocab.values()) + 1``) is the star's label.  -> (text_starred: the words with the stars, tokens: a list of labels per entry)."""
    if romanize:
        raise NotImplementedError("romanize=True needs uroman, which is absent")
    if star_frequency not in ("segment", "edges"):
        raise ValueError('star_frequency: "segment" or "edges"')
    if star_index is None:
        star_index = max(vocab.values()) + 1
    words = preprocess_text(text.lower()).split()
    text_starred, tokens = [], []

    def star():
        text_starred.append(STAR); tokens.append([star_index])

    if star_frequency == "edges":
        star()
    for w in words:
        if star_frequency == "segment":
            star()
        text_starred.append(w); tokens.append([vocab[ch] for ch in w if ch in vocab])
    if star_frequency == "edges":
        star()
    return text_starred, tokens


def merge_repeats(path):
    """Runs of equal labels -> [(label, first_frame, last_frame)]."""
    path = np.asarray(path).reshape(-1)
    if not len(path):
        return []
    cut = np.flatnonzero(path[1:] != path[:-1]) + 1
    firsts = np.concatenate(([0], cut)); lasts = np.concatenate((cut - 1, [len(path) - 1]))
    return [(int(path[a]), int(a), int(b)) for a, b in zip(firsts, lasts)]


def get_spans(words, segments, blank):
    """``words``: one list of labels per word, in order; ``segments``: ``merge_repeats`` of the path those labels were aligned to.
    -> one ``Span`` per word (the module's docstring has the rule)."""
    if not segments:
        if any(words):
            raise ValueError("no segments, but a word has characters")
        return [Span(0, 0, 0, 0) for _ in words]
    intervals = []                               # (seg_first, seg_last) per word
    w = 0

    def emptied(at):
        nonlocal w
        while w < len(words) and not words[w]:
            intervals.append((at, at)); w += 1

    emptied(0)
    k = 0                                        # character of words[w] the next non-blank segment must carry
    for si, (label, _, _) in enumerate(segments):
        if label == blank:
            continue
        if w >= len(words):
            raise ValueError(f"segment {si} carries label {label} after the last word")
        if label != words[w][k]:
            raise ValueError(f"segment {si} carries label {label}, word {w} expects {words[w][k]}")
        if k == 0:
            seg_first = si
        k += 1
        if k == len(words[w]):
            intervals.append((seg_first, si)); w += 1; k = 0
            emptied(si)
    if w != len(words):
        raise ValueError(f"the path ends inside word {w}")
    spans = []
    for n, (a, b) in enumerate(intervals):
        first, last = segments[a][1], segments[b][2]
        if a > 0 and segments[a - 1][0] == blank:
            _, s, e = segments[a - 1]
            first = s if n == 0 else int((s + e) / 2)
        if b + 1 < len(segments) and segments[b + 1][0] == blank:
            _, s, e = segments[b + 1]
            last = e if n == len(intervals) - 1 else math.floor((s + e) / 2)
        spans.append(Span(first, last, a, b))
    return spans


def default_stride_ms(n_samples: int, n_frames: int) -> int:
    """Milliseconds per emission frame as the command rounds them: ``ceil(n_samples * 1000 / T / 16000)``."""
    return math.ceil(n_samples * 1000 / n_frames / SAMPLE_RATE)


def word_times(text_starred, tokens, spans, segments, frame_score, blank=0, n_samples=None, stride_ms=None):
    """-> [{"start", "end", "text", "confidence"}] for every entry of ``text_starred`` that is not ``<star>``: ``start`` / ``end`` =
    the span's first / last frame ``* stride_ms / 1000`` (``stride_ms`` defaults to ``default_stride_ms(n_samples, T)``), ``confidence`` =
    ``exp(mean frame_score)`` over the frames of the word's character segments (the blanks between them left out; NaN for a word without
    characters)."""
    frame_score = np.asarray(frame_score, dtype=np.float32)
    if stride_ms is None:
        if n_samples is None:
            raise ValueError("word_times: give stride_ms or n_samples")
        stride_ms = default_stride_ms(n_samples, len(frame_score))
    out = []
    for text, labels, sp in zip(text_starred, tokens, spans):
        if text == STAR:
            continue
        conf = float("nan")
        if labels:
            own = np.concatenate([frame_score[a:b + 1] for lab, a, b in segments[sp.seg_first:sp.seg_last + 1] if lab != blank])
            conf = float(np.exp(np.mean(own, dtype=np.float64)))
        out.append({"start": sp.first_frame * stride_ms / 1000, "end": sp.last_frame * stride_ms / 1000, "text": text, "confidence": conf})
    return out


def align_words(path, frame_score, text_starred, tokens, blank, n_samples=None, stride_ms=None):
    """merge_repeats -> get_spans -> word_times for one clip."""
    segments = merge_repeats(path)
    spans = get_spans(tokens, segments, blank)
    return word_times(text_starred, tokens, spans, segments, frame_score, blank, n_samples, stride_ms)
