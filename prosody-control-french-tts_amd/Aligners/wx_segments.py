"""The host rules of ``whisperx.align`` around its dynamic programme (``ProsodyEngine.wx_align``): cleaning a transcript segment into the
characters the alignment model knows, merging the frame path into character segments, and assembling characters into words and segments.

``whisperx`` is third party and absent: restated from the published source of whisperx 3.3.x (alignment.py), parity unpinned.  Not built:
the sentence split (nltk's Punkt tokenizer, absent).  whisperx cuts an aligned segment into one sub-segment per sentence; here each input
segment is one sentence.  ``word_segments``, which is all ``Code/Aligners/whisperX.py`` reads besides the last segment's ``end``, does not
depend on the split: a word never spans two sentences."""
from __future__ import annotations

import numpy as np

LANGUAGES_WITHOUT_SPACES = ("ja", "zh")
WILDCARD = "*"


def clean_segment(text: str, dictionary: dict, language: str):
    """-> ``(clean_char, clean_cdx, tokens)``: the characters of ``text`` that take part in the alignment (lower-cased; ``" "`` -> ``"|"``
    for a language written with spaces; leading and trailing blanks of the segment left out; a character absent from ``dictionary`` becomes
    ``'*'``), their positions in ``text``, and their vocabulary indices (-1 for ``'*'``: the wildcard)."""
    num_leading = len(text) - len(text.lstrip())
    num_trailing = len(text) - len(text.rstrip())
    clean_char, clean_cdx = [], []
    for cdx, char in enumerate(text):
        char_ = char.lower()
        if language not in LANGUAGES_WITHOUT_SPACES:
            char_ = char_.replace(" ", "|")
        if cdx < num_leading or cdx > len(text) - num_trailing - 1:
            continue
        clean_char.append(char_ if char_ in dictionary else WILDCARD)
        clean_cdx.append(cdx)
    tokens = [dictionary.get(c, -1) if c != WILDCARD else -1 for c in clean_char]
    return clean_char, clean_cdx, tokens


def merge_repeats(path_tok, path_lp, text_clean):
    """Runs of equal token index -> ``[(label, start, end, score)]``: ``start`` the run's first frame, ``end`` its last frame + 1, ``score``
    the mean of ``exp(lp)`` over the run (``np.exp`` on float32: parity with torch's scalar ``exp`` in the last bit is not claimed, and the
    scores are rounded to 3 decimals by ``assemble``)."""
    path_tok = np.asarray(path_tok)
    prob = np.exp(np.asarray(path_lp, dtype=np.float32))
    out, i1, n = [], 0, len(path_tok)
    while i1 < n:
        i2 = i1
        while i2 < n and path_tok[i2] == path_tok[i1]:
            i2 += 1
        score = sum(float(p) for p in prob[i1:i2]) / (i2 - i1)
        out.append((text_clean[int(path_tok[i1])], i1, i2, score))
        i1 = i2
    return out


def assemble(segment: dict, char_segments, n_frames: int, language: str = "fr"):
    """One aligned segment ``{"start", "end", "text", "words"}`` from the character segments of ``merge_repeats`` (one per clean character;
    ``segment["clean_cdx"]``: their positions in the text, from ``clean_segment``).
    ``ratio = (t2 - t1) / (T - 1)``; a character's ``start`` / ``end`` = ``round(x * ratio + t1, 3)``, its score rounded to 3 decimals; the
    word index advances at the last character and before every space (at every character for a language without spaces); a word is the
    stripped join of its characters (an empty one is skipped), ``start`` = min, ``end`` = max and ``score`` = ``round(mean, 3)`` over its
    non-space aligned characters, each key left out where nothing aligned; the segment's ``start`` / ``end`` = min / max over its aligned
    characters, its own times when nothing aligned."""
    t1, t2, text = segment["start"], segment["end"], segment["text"]
    ratio = (t2 - t1) / (n_frames - 1)
    where = {cdx: k for k, cdx in enumerate(segment["clean_cdx"])}
    chars, word_idx = [], 0
    for cdx, char in enumerate(text):
        start = end = score = None
        if cdx in where:
            _, f1, f2, sc = char_segments[where[cdx]]
            start, end, score = round(f1 * ratio + t1, 3), round(f2 * ratio + t1, 3), round(sc, 3)
        chars.append((char, start, end, score, word_idx))
        if language in LANGUAGES_WITHOUT_SPACES or cdx == len(text) - 1 or text[cdx + 1] == " ":
            word_idx += 1
    words = []
    for w in range(word_idx):
        mine = [c for c in chars if c[4] == w]
        word_text = "".join(c[0] for c in mine).strip()
        if not word_text:
            continue
        timed = [c for c in mine if c[0] != " " and c[1] is not None]
        word = {"word": word_text}
        if timed:
            word["start"] = min(c[1] for c in timed)
            word["end"] = max(c[2] for c in timed)
            word["score"] = round(sum(c[3] for c in timed) / len(timed), 3)
        words.append(word)
    timed = [c for c in chars if c[1] is not None]
    return {"start": min(c[1] for c in timed) if timed else t1, "end": max(c[2] for c in timed) if timed else t2, "text": text, "words": words}


def unaligned(segment: dict):
    """What whisperx returns for a segment it cannot align: the original times, no words."""
    return {"start": segment["start"], "end": segment["end"], "text": segment["text"], "words": []}
