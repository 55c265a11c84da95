"""Score aligner TextGrids against a hand-made gold word tier: the reference's ``Code/whisper_testing/splitting.py`` with its names and
signatures, every function taking an additive ``engine=None``.

The reference pairs gold and predicted word intervals by their normalised texts (``align_intervals``) for the whole recording, for every
15 s window and for every sentence, and reports the alignment recall rate (ARR) and the MAE / RMSE of starts, ends and durations at those
levels and per word.  The pairing is a loop over every (gold, unclaimed predicted) pair per call; here it is stated in BITMAP FORM, which is
what the device runs (``ProsodyEngine.interval_match``, ``pce_ivl_match`` of include/pce.h):

* the score of a pair depends on its two normalised texts alone, so a recording has ONE class table -- per gold interval three bitmaps over
  the predicted tier: equal (1.0), one text inside the other (0.8), a shared word (0.5), in the reference's order of tests;
* a call of ``align_intervals`` is a PROBLEM on that table: the gold rows it walks, in order, and the predicted intervals that are members
  (a window or sentence filters both tiers and keeps their order); a gold row claims the lowest set bit of ``row & members & ~claimed`` of
  the best class that has one, which is the reference's strict ``>``: the first of the best score.

With ``engine=None`` the same decisions run on the host with Python integers as bitmaps; with an engine, all problems of a recording --
or, in ``evaluate_textgrids``, of all recordings' tiers -- go through one ``interval_match`` call.  Normalisation (once per interval),
word interning, the overlap tests and the metrics stay on the host; the metrics are the reference's numpy calls on the same lists in
the same order, so the two paths return the same bits.  The printed table of ``run_nemo_evaluation`` is not built."""
import logging
import re
import wave
from pathlib import Path

import numpy as np

log = logging.getLogger(__name__)

INF = float("inf")
_NUMBER = r"([\d.]+)"
# an interval of a long-format TextGrid as the reference's parser sees it: any text between the quotes, a newline included, but no quote
_INTERVAL = re.compile(r"intervals \[\d+\]:\s*xmin = " + _NUMBER + r"\s*xmax = " + _NUMBER + r'\s*text = "([^"]*)"')
_NOT_WORD_OR_SPACE = re.compile(r"[^\w\s]")
WINDOW_S = 15


def parse_textgrid(textgrid_path, engine=None):
    """The word intervals of a TextGrid (:8-24): every ``intervals [n]`` record of every tier whose text is not blank, text stripped."""
    content = Path(textgrid_path).read_text(encoding="utf-8")
    intervals = []
    for m in _INTERVAL.finditer(content):
        xmin, xmax, text = m.groups()
        if text.strip():
            intervals.append({"start": float(xmin), "end": float(xmax), "text": text.strip(), "duration": float(xmax) - float(xmin)})
    return intervals


def normalize_text(text, engine=None):
    """Lower case, everything that is neither a word character nor whitespace removed (Unicode-aware), stripped (:90-92)."""
    return _NOT_WORD_OR_SPACE.sub("", text.lower()).strip()


def create_mock_segments_from_intervals(intervals, audio_duration, max_segment_duration=30, engine=None):
    """Sentence-like segments for a tier that has none (:51-88): a new segment opens at a gap of more than 1 s or once the running one has
    passed ``max_segment_duration``; the last one is kept when it starts inside the audio."""
    if not intervals:
        return {"segments": []}
    segments = []
    start, end = intervals[0]["start"], intervals[0]["end"]
    for interval in intervals[1:]:
        if interval["start"] - end > 1.0 or end - start > max_segment_duration:
            segments.append({"start": start, "end": end})
            start = interval["start"]
        end = interval["end"]
    if start < audio_duration:
        segments.append({"start": start, "end": end})
    return {"segments": segments}


# ---- the matching, in bitmap form (the host restatement of k_ivl_classes / k_ivl_claim; the GPU tests compare the device with it)

def _is_substring(a, b):
    """``a in b``: the empty string is inside every string."""
    return a in b


def _pair_class(gold_norm, pred_norm, gold_words, pred_words):
    """3 / 2 / 1 / 0 for the reference's scores 1.0 / 0.8 / 0.5 / 0, in its order of tests (:111-118)."""
    if gold_norm == pred_norm:
        return 3
    if _is_substring(gold_norm, pred_norm) or _is_substring(pred_norm, gold_norm):
        return 2
    if any(w in pred_words for w in gold_words):
        return 1
    return 0


def _first_bit(x):
    """The index of the lowest set bit: the first candidate in list order (the reference replaces its best on a strict > only)."""
    return (x & -x).bit_length() - 1


def _new_claims():
    """The claimed set of one ``align_intervals`` call: a one-element list holding the bitmap.  Every problem starts with its own."""
    return [0]


def class_rows(gold_norms, pred_norms):
    """Per gold text ``(equal, substring, word)`` bitmaps over the predicted tier, exclusive.  The class is a function of the two texts,
    so it is worked out once per distinct pair of texts."""
    positions = {}
    for j, p in enumerate(pred_norms):
        positions[p] = positions.get(p, 0) | (1 << j)
    pred_words = {p: p.split() for p in positions}
    rows = {}
    for g in gold_norms:
        if g in rows:
            continue
        masks = [0, 0, 0, 0]
        g_words = g.split()
        for p, bits in positions.items():
            masks[_pair_class(g, p, g_words, pred_words[p])] |= bits
        rows[g] = (masks[3], masks[2], masks[1])
    return [rows[g] for g in gold_norms]


def claim(rows, gold_indices, members):
    """One problem: ``rows`` of ``class_rows``, the gold rows to walk and the bitmap of member predictions (None: all) ->
    (match, cls): per gold entry the claimed predicted index or -1, and its class."""
    claims = _new_claims()
    match, cls = [], []
    for g in gold_indices:
        hit, klass = -1, 0
        for k, row in zip((3, 2, 1), rows[g]):
            free = row & ~claims[0] if members is None else row & members & ~claims[0]
            if free:
                hit, klass = _first_bit(free), k
                claims[0] |= 1 << hit
                break
        match.append(hit); cls.append(klass)
    return np.array(match, dtype=np.int32).reshape(-1), np.array(cls, dtype=np.int8).reshape(-1)


def interval_match_host(tables, problems):
    """``ProsodyEngine.interval_match`` on the host: same arguments, same result."""
    rows = {}
    out = []
    for t, gold_indices, pred_indices in problems:
        if t not in rows:
            rows[t] = class_rows(*tables[t])
        members = None if pred_indices is None else sum(1 << int(j) for j in set(pred_indices))
        out.append(claim(rows[t], [int(g) for g in gold_indices], members))
    return out


def _match(tables, problems, engine):
    return interval_match_host(tables, problems) if engine is None else engine.interval_match(tables, problems)


def _pairs(gold_intervals, pred_intervals, gold_indices, match):
    return [(gold_intervals[g], pred_intervals[m]) for g, m in zip(gold_indices, match.tolist()) if m >= 0]


def align_intervals(gold_intervals, pred_intervals, engine=None):
    """(gold, predicted) interval pairs by text similarity (:94-128), in gold order."""
    table = ([normalize_text(g["text"]) for g in gold_intervals], [normalize_text(p["text"]) for p in pred_intervals])
    gold_indices = list(range(len(gold_intervals)))
    (match, _), = _match([table], [(0, gold_indices, None)], engine)
    return _pairs(gold_intervals, pred_intervals, gold_indices, match)


# ---- the metrics (:130-252): the reference's numpy calls on the same lists in the same order

def _errors(aligned_pairs, key):
    return [abs(gold[key] - pred[key]) for gold, pred in aligned_pairs]


def calculate_metrics(aligned_pairs, total_gold, engine=None):
    if not aligned_pairs:
        return {"ARR": 0.0, "MAE_start": INF, "MAE_end": INF, "MAE_duration": INF, "RMSE_start": INF, "RMSE_end": INF, "RMSE_duration": INF,
                "count": 0}
    out = {"ARR": len(aligned_pairs) / total_gold if total_gold > 0 else 0}
    errors = {key: _errors(aligned_pairs, key) for key in ("start", "end", "duration")}
    for key in ("start", "end", "duration"):
        out[f"MAE_{key}"] = np.mean(errors[key])
    for key in ("start", "end", "duration"):
        out[f"RMSE_{key}"] = np.sqrt(np.mean(np.array(errors[key]) ** 2))
    out["count"] = len(aligned_pairs)
    return out


def _times(intervals):
    """(starts, ends) of a tier as float64 arrays: the numbers ``parse_textgrid`` makes."""
    return (np.array([interval["start"] for interval in intervals], dtype=np.float64),
            np.array([interval["end"] for interval in intervals], dtype=np.float64))


def _indices_in_window(times, start_time, end_time):
    """The reference's overlap test (:155-160) on a tier's ``_times``: the two comparisons per interval, for all intervals at once."""
    starts, ends = times
    return np.nonzero((starts < end_time) & (ends > start_time))[0].tolist()


def get_intervals_in_window(intervals, start_time, end_time, engine=None):
    """The intervals that overlap [start_time, end_time), list order kept (:155-160)."""
    return [intervals[i] for i in _indices_in_window(_times(intervals), start_time, end_time)]


def _segment_bounds(segment):
    seg_start = segment.get("start", 0)
    seg_end = segment.get("end", seg_start + 1 if seg_start is not None else 1)
    return None if seg_start is None or seg_end is None else (seg_start, seg_end)


def get_intervals_in_segment(intervals, segment, engine=None):
    """The intervals that overlap a segment of the model's output (:162-168); a segment without an end is taken as 1 s long."""
    bounds = _segment_bounds(segment)
    return [] if bounds is None else get_intervals_in_window(intervals, *bounds)


class _Plan:
    """The problems of one (gold tier, predicted tier) pair -- entire audio, the windows and the sentences that hold a gold interval --
    and how their matches become the reference's result."""

    def __init__(self, gold_intervals, pred_intervals, model_output_segments, audio_duration):
        self.gold, self.pred = gold_intervals, pred_intervals
        self.table = ([normalize_text(g["text"]) for g in gold_intervals], [normalize_text(p["text"]) for p in pred_intervals])
        self.lists = [(list(range(len(gold_intervals))), None)]
        self.window_starts = []
        gold_times, pred_times = _times(gold_intervals), _times(pred_intervals)
        gold_window = lambda start, end: _indices_in_window(gold_times, start, end)        # noqa: E731
        pred_window = lambda start, end: _indices_in_window(pred_times, start, end)        # noqa: E731
        for start in range(0, int(audio_duration), WINDOW_S):
            end = min(start + WINDOW_S, audio_duration)
            gold_indices = gold_window(start, end)
            if gold_indices:
                self.window_starts.append(start)
                self.lists.append((gold_indices, pred_window(start, end)))
        self.n_sentences = 0
        if "segments" in model_output_segments and model_output_segments["segments"]:
            for segment in model_output_segments["segments"]:
                bounds = _segment_bounds(segment)
                gold_indices = [] if bounds is None else gold_window(*bounds)
                if gold_indices:
                    self.n_sentences += 1
                    self.lists.append((gold_indices, pred_window(*bounds)))

    def problems(self, table_index):
        return [(table_index, g, p) for g, p in self.lists]

    def results(self, matches):
        """``matches``: what the matching returned for ``problems``, in order."""
        stats = []
        pairs_entire = None
        for (gold_indices, _), (match, _) in zip(self.lists, matches):
            pairs = _pairs(self.gold, self.pred, gold_indices, match)
            if pairs_entire is None:
                pairs_entire = pairs
            stats.append(calculate_metrics(pairs, len(gold_indices)))
        results = {"entire_audio": stats[0]}
        windows = stats[1:1 + len(self.window_starts)]
        sentences = stats[1 + len(self.window_starts):]
        for w, start in zip(windows, self.window_starts):
            w["window_start"] = start
        if windows:
            results["window_15s"] = {"mean_ARR": np.mean([w["ARR"] for w in windows])}
            for key in ("start", "end", "duration"):
                results["window_15s"][f"mean_MAE_{key}"] = np.mean([w[f"MAE_{key}"] for w in windows if w[f"MAE_{key}"] != INF])
            results["window_15s"]["std_ARR"] = np.std([w["ARR"] for w in windows])
            results["window_15s"]["window_count"] = len(windows)
        else:
            results["window_15s"] = {"mean_ARR": 0, "window_count": 0, "mean_MAE_start": INF, "mean_MAE_end": INF, "mean_MAE_duration": INF}
        if sentences:
            results["sentence"] = {"mean_ARR": np.mean([s["ARR"] for s in sentences])}
            for key in ("start", "end", "duration"):
                results["sentence"][f"mean_MAE_{key}"] = np.mean([s[f"MAE_{key}"] for s in sentences if s[f"MAE_{key}"] != INF])
            results["sentence"]["sentence_count"] = len(sentences)
        else:
            results["sentence"] = {"mean_ARR": 0, "sentence_count": 0, "mean_MAE_start": INF, "mean_MAE_end": INF, "mean_MAE_duration": INF}
        if pairs_entire:
            errors = {key: _errors(pairs_entire, key) for key in ("start", "end", "duration")}
            word = {f"mean_{key}_error": np.mean(errors[key]) for key in ("start", "end", "duration")}
            word.update({f"median_{key}_error": np.median(errors[key]) for key in ("start", "end", "duration")})
            word.update({"max_start_error": np.max(errors["start"]), "max_end_error": np.max(errors["end"]), "word_count": len(pairs_entire)})
        else:
            word = {"word_count": 0}
            word.update({f"{stat}_{key}_error": INF for stat in ("mean", "median") for key in ("start", "end", "duration")})
            word.update({"max_start_error": INF, "max_end_error": INF})
        results["word"] = word
        return results


def calculate_multilevel_stats(gold_intervals, pred_intervals, model_output_segments, audio_duration, engine=None):
    """The statistics at all four levels (:171-252): entire audio, 15 s windows, the segments of ``model_output_segments`` and single
    words.  With an engine the entire-audio problem, all windows and all sentences go through one ``interval_match`` call."""
    plan = _Plan(gold_intervals, pred_intervals, model_output_segments, audio_duration)
    return plan.results(_match([plan.table], plan.problems(0), engine))


def evaluate_nemo_textgrid(nemo_textgrid_path, gold_intervals, audio_duration, engine=None):
    """One aligner TextGrid against the gold intervals (:28-49); None when the TextGrid holds no interval."""
    (stats,) = _evaluate(gold_intervals, {"NeMo": nemo_textgrid_path}, audio_duration, None, engine) or (None,)
    return stats


def _evaluate(gold_intervals, pred_paths, audio_duration, segments, engine):
    plans, names = [], []
    for name, path in pred_paths.items():
        pred_intervals = parse_textgrid(path)
        log.info("%s: %d intervals in %s", name, len(pred_intervals), path)
        if not pred_intervals:
            log.warning("No intervals found in %s TextGrid %s", name, path)
            continue
        model_output = segments[name] if segments is not None and name in segments else create_mock_segments_from_intervals(pred_intervals, audio_duration)
        plans.append(_Plan(gold_intervals, pred_intervals, model_output, audio_duration)); names.append(name)
    problems, first = [], [0]
    for t, plan in enumerate(plans):
        problems.extend(plan.problems(t)); first.append(len(problems))
    matches = _match([plan.table for plan in plans], problems, engine) if problems else []
    out = []
    for t, (plan, name) in enumerate(zip(plans, names)):
        stats = plan.results(matches[first[t]:first[t + 1]])
        stats["model"] = name
        stats["processing_time"] = 0                       # not measured for a TextGrid made beforehand, as the reference sets it
        out.append(stats)
    return out


def evaluate_textgrids(gold_path, pred_paths, audio_duration, segments=None, engine=None):
    """The batch form: every TextGrid of ``pred_paths`` ({model name: path}) against the gold tier of ``gold_path``, all problems of all
    of them through one matching call.  ``segments``: {model name: the model's result with its 'segments'}; a model without an entry gets
    the mock segments of its own intervals.  -> the stats dicts of ``evaluate_nemo_textgrid``, ``'model'`` = the dict key; a TextGrid
    without intervals is left out."""
    gold_intervals = parse_textgrid(gold_path)
    if not gold_intervals:
        log.warning("No gold intervals found in %s", gold_path)
        return []
    return _evaluate(gold_intervals, pred_paths, audio_duration, segments, engine)


SUMMARY_LEVELS = (("entire", "entire_audio", ("ARR", "MAE_start", "MAE_end", "MAE_duration", "RMSE_start", "RMSE_end", "RMSE_duration")),
                  ("win15s", "window_15s", ("mean_ARR", "mean_MAE_start", "mean_MAE_duration")),
                  ("sent", "sentence", ("mean_ARR", "mean_MAE_start", "mean_MAE_duration")),
                  ("word", "word", ("mean_start_error", "mean_duration_error", "median_start_error", "max_start_error")))


def summary_row(stats):
    """One row of the reference's summary table (:312-336)."""
    row = {"model": stats["model"], "time_s": stats["processing_time"]}
    for prefix, level, keys in SUMMARY_LEVELS:
        for key in keys:
            row[f"{prefix}_{key}"] = stats[level].get(key, 0 if key == "mean_ARR" else INF)
    return row


def audio_duration_of(audio):
    """Seconds: a number as it is, a WAV file by its header."""
    if isinstance(audio, (int, float)):
        return audio
    with wave.open(str(audio), "rb") as w:
        return w.getnframes() / w.getframerate()


def run_evaluation(gold_path, pred_paths, audio, output_dir, engine=None):
    """The reference's ``run_nemo_evaluation`` (:254-341) with its paths as parameters and any number of aligners: the summary table
    of all models, one row each, also written per model as ``<name>_evaluation_summary.csv`` under ``output_dir``."""
    import pandas as pd
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    all_results = evaluate_textgrids(gold_path, pred_paths, audio_duration_of(audio), engine=engine)
    rows = [summary_row(r) for r in all_results]
    for row in rows:
        pd.DataFrame([row]).to_csv(output_dir / f"{row['model']}_evaluation_summary.csv", index=False)
        log.info("%s: ARR %.3f, MAE_start %.3fs, MAE_duration %.3fs", row["model"], row["entire_ARR"], row["entire_MAE_start"], row["entire_MAE_duration"])
    return pd.DataFrame(rows)
