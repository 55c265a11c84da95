"""The "Compare Breaks" step of ``Code/audioPipeline.py`` (:895-1074): did the synthesised pauses land where the SSML asked?

Reads ``OUT.TextGrid`` ("Final Transcribe") and ``BDD_syntagme_for_synth.csv`` ("Measure & Build SSML"), aligns every speech chunk of the
CSV with the speech blocks of the TextGrid, and writes ``pause_comparison_full.csv``.  The step's cost is its alignment: the ratio of
``difflib.SequenceMatcher`` for all n x m (chunk, block) pairs, then an n x m DP over them.  With an engine both run on the device in
one ``seqmatch_align`` call; with ``engine=None`` the same function runs ``difflib`` and a DP on the host.  The two paths give the same
bits: the matching is integer, the ratio one fp64 division, the DP fp64 adds and ``>=`` in a fixed order.

What is kept of the reference is its observable contract -- the CSV columns, the log lines, the roundings -- pinned by golden G10
(tests/golden/compare_breaks.json, written by the reference's own step).  The bookkeeping around the alignment is array work:
    blocks   the maximal runs of non-empty marks of the first tier; the interval that ends a run is empty, and is the run's silence
    events   the blank CSV rows that follow a row with a word character; an event belongs to that row's chunk
    spans    chunk c reaches up to the block before the next matched block (the last block, after the last match), so its events go
             to block ``stop[k] - 1``, k = the number of matches at or before c; a chunk before the first match has no block
    silence  of the events that share a block only the last one is given the measured silence, the others 0 ms
"""
from __future__ import annotations

import logging
import re
from difflib import SequenceMatcher

import numpy as np

from .textgrid_io import read_textgrid

COLUMNS = ("segment", "syntagme", "nat_voice_ms", "synth_voice_ms", "diff_ms", "ok", "match_quality")
DIAGONAL, UP, LEFT = 0, 1, 2            # the 2-bit trace of the DP, as k_seqmatch_align keeps it


def normalize(s: str) -> str:
    """What the ratios are taken of: lower case, only word characters and single spaces."""
    return " ".join(re.sub(r"[^\w\s]", "", s.lower()).split())


def to_ms(seconds) -> int:
    return int(round(seconds * 1000))


def speech_blocks(intervals):
    """``intervals`` = [(t_min, t_max, mark), ...] of the first tier -> (the text of every speech block, the silence after each in ms)."""
    marks = [mark.strip() for _, _, mark in intervals]
    voiced = np.array([bool(mark) for mark in marks] + [False])
    edges = np.flatnonzero(voiced[1:] != voiced[:-1]) + 1                  # where a run of marks starts or stops
    if voiced[0]:
        edges = np.concatenate(([0], edges))
    texts, silences = [], []
    for first, stop in edges.reshape(-1, 2).tolist():
        texts.append(" ".join(marks[first:stop]))
        # intervals[stop] ended the run, so it is empty; a run that reaches the end of the tier has no silence
        silences.append(to_ms(intervals[stop][1] - intervals[stop][0]) if stop < len(marks) else 0)
    return texts, np.array(silences, dtype=np.int64)


def pause_events(df):
    """The CSV -> (text of every speech chunk, row of every pause event, chunk index of every pause event)."""
    text = df["syntagme"].fillna("").astype(str)
    worded = text.str.contains(r"\w", regex=True).to_numpy(dtype=bool)
    blank = (text.str.strip() == "").to_numpy()
    chunk_of_row = np.cumsum(worded) - 1                                   # the chunk a worded row is
    event_rows = np.flatnonzero(blank[1:] & worded[:-1]) + 1
    return [t.strip() for t in text[worded]], event_rows, chunk_of_row[event_rows - 1]


def align_host(a, b):
    """The alignment on the CPU: ``a`` / ``b`` normalised strings -> (matches [(i, j), ...] ascending, sim [n][m]).
    Cell (i, j) takes the larger of the cell above, the cell to the left and the diagonal cell plus sim; above wins ties, then left."""
    n, m = len(a), len(b)
    sim = [[SequenceMatcher(None, x, y).ratio() for y in b] for x in a]
    trace = np.empty((n, m), dtype=np.uint8)
    above = [0.0] * (m + 1)
    for i in range(n):
        here = [0.0] * (m + 1)
        for j in range(m):
            up, left, diagonal = above[j + 1], here[j], above[j] + sim[i][j]
            if up >= left and up >= diagonal:
                here[j + 1], trace[i, j] = up, UP
            elif left >= diagonal:
                here[j + 1], trace[i, j] = left, LEFT
            else:
                here[j + 1], trace[i, j] = diagonal, DIAGONAL
        above = here
    matches = []
    i, j = n - 1, m - 1
    while i >= 0 and j >= 0:
        step = trace[i, j]
        if step == DIAGONAL:
            matches.append((i, j))
        if step != LEFT:
            i -= 1
        if step != UP:
            j -= 1
    return matches[::-1], sim


def compare_breaks(textgrid_path, syntagme_csv, out_csv, tol_ms: int = 5, engine=None):
    """``AudioPipeline.compare_breaks`` on explicit paths -> the DataFrame it returns; ``out_csv`` receives ``pause_comparison_full.csv``.
    ``engine``: a ``ProsodyEngine`` (one ``seqmatch_align`` call) or None (``difflib`` + the DP on the host)."""
    import pandas as pd

    block_text, silence_ms = speech_blocks(read_textgrid(textgrid_path).tiers[0].intervals)
    df = pd.read_csv(syntagme_csv)
    chunk_text, event_rows, event_chunk = pause_events(df)

    a, b = [normalize(t) for t in chunk_text], [normalize(t) for t in block_text]
    if engine is None:
        matches, sim = align_host(a, b)
    else:
        matches, sim = engine.seqmatch_align(a, b)
    matches = np.asarray(matches, dtype=np.int64).reshape(-1, 2)
    sim = np.asarray(sim, dtype=np.float64).reshape(len(a), len(b))

    # the block of every event (-1: none), and whether it is the last event of its block
    stop = np.append(matches[:, 1], len(b))
    k = np.searchsorted(matches[:, 0], event_chunk, side="right")
    block = np.where(k > 0, stop[k] - 1, -1)
    last_of_block = np.ones(len(block), dtype=bool)
    last_of_block[:-1] = block[:-1] != block[1:]                           # (event_chunk ascends, hence block does)
    placed = block >= 0

    expected = np.array([int(round(float(p))) for p in df["pause"].to_numpy()[event_rows]], dtype=np.int64)
    measured = np.where(placed & last_of_block, silence_ms[block] if len(silence_ms) else 0, 0).astype(np.int64)
    quality = [float(sim[c, t]) if t >= 0 else 0.0 for c, t in zip(event_chunk.tolist(), block.tolist())]
    syntagme = [chunk_text[c] for c in event_chunk.tolist()]
    for txt, t, q in zip(syntagme, block.tolist(), quality):
        if t >= 0 and q < 0.5:
            logging.warning(f"Low match quality for “{txt}” → “{block_text[t]}”: {q:.2f}")

    diff = measured - expected
    table = dict(zip(COLUMNS, (df["segment"].to_numpy()[event_rows], syntagme, expected, measured, diff, np.abs(diff) <= tol_ms,
                               [round(q, 2) for q in quality])))
    result = pd.DataFrame(table) if len(event_rows) else pd.DataFrame([])
    if len(result):
        total, within = len(result), int(result["ok"].sum())
        logging.info(f"Breaks compared: {total}")
        logging.info(f"Within ±{tol_ms} ms: {within}/{total} ({within/total*100:.1f}%)")
        logging.info(f"Avg |diff|: {int(round(result['diff_ms'].abs().mean()))} ms")
        logging.info(f"Avg match_quality: {round(result['match_quality'].mean(), 2)}")
    else:
        logging.warning("No breaks found to compare.")
    result.to_csv(out_csv, index=False)
    return result
