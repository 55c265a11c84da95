#!/usr/bin/env python3
"""Generate tests/golden/aligner_eval.json (G11) by RUNNING THE REFERENCE'S OWN ``Code/whisper_testing/splitting.py``.

Runs only in the build container (needs the reference tree, see make_goldens.py).  The module imports as it is: numpy, pandas and ``re``.
What is committed is data: seeded word tiers (stored once each as ``[start, end, text, duration]`` rows, times in hundredths of a second so
that the file stays small; tests/ivl_cases.py makes the interval dicts), TextGrid texts, and what the reference's functions return for them --
``align_intervals`` as (gold index, predicted index) pairs (every interval dict carries its index as ``'i'``; the functions pass the
dicts through), ``create_mock_segments_from_intervals`` and ``calculate_multilevel_stats`` as they are, ``parse_textgrid`` as its
interval list.  ``Infinity`` and ``NaN`` are written as Python's ``json`` writes them.
"""
import json
import random
import sys
import tempfile
import warnings
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_goldens as MG  # noqa: E402

sys.path.insert(0, str(MG.REF / "Code" / "whisper_testing"))
import splitting as S  # noqa: E402

VOCAB = ["le", "la", "de", "un", "une", "et", "chat", "château", "chante", "chanter", "l'eau", "eau", "aujourd'hui", "hui", "—", "...",
         "Bonjour,", "bonjour", "est-ce", "ce", "que", "qu'il", "il", "a", "à", "été", "ete", "le chat", "de la", "😀"]


def tier(items, t0=0.0):
    """[(text, duration, gap before), ...] -> intervals, tagged with their index."""
    t, out = t0, []
    for i, (text, dur, gap) in enumerate(items):
        t = round(t + gap, 2)
        out.append({"start": t, "end": round(t + dur, 2), "text": text, "duration": dur, "i": i})
        t = round(t + dur, 2)
    return out


def retag(intervals):
    return [dict(iv, i=i) for i, iv in enumerate(intervals)]


def seeded_tier(rng, n):
    return tier([(rng.choice(VOCAB), round(rng.uniform(0.05, 0.6), 2), round(rng.uniform(1.0, 2.5), 2) if rng.random() < 0.08 else 0.0) for _ in range(n)])


def perturb(rng, gold, jitter=0.04):
    """An aligner's tier for a gold tier: words dropped, substituted, doubled and inserted, boundaries moved."""
    out = []
    for iv in gold:
        r = rng.random()
        if r < 0.10:
            continue                                                         # dropped
        iv = dict(iv, start=round(iv["start"] + rng.uniform(-jitter, jitter), 2), end=round(iv["end"] + rng.uniform(-jitter, jitter), 2))
        iv["duration"] = round(iv["end"] - iv["start"], 2)
        if r < 0.20:
            iv["text"] = rng.choice(VOCAB)                                   # substituted
        out.append(iv)
        if r > 0.95:
            out.append(dict(iv))                                             # doubled
        elif r > 0.92:
            out.append(dict(iv, text=rng.choice(VOCAB), start=iv["end"], end=round(iv["end"] + 0.01, 2), duration=0.01))      # inserted
    return retag(out)


FRENCH_GOLD = [("Bonjour,", 0.4, 0.2), ("aujourd'hui", 0.6, 0.0), ("l'eau", 0.3, 0.1), ("est-ce", 0.3, 0.0), ("que", 0.2, 0.0), ("...", 0.2, 0.0),
               ("le", 0.1, 1.4), ("chat", 0.3, 0.0), ("chante", 0.4, 0.0), ("—", 0.1, 0.0), ("le", 0.1, 0.0), ("chat", 0.3, 0.0), ("dort", 0.3, 0.0),
               ("à côté", 0.5, 0.0), ("de la", 0.2, 0.0), ("rivière", 0.6, 8.0), ("😀", 0.2, 0.0), ("Été", 0.3, 0.0), ("le", 0.1, 0.0), ("le", 0.1, 0.0),
               ("château", 0.7, 0.0), ("fin", 0.4, 12.0)]
FRENCH_PRED = [("bonjour", 0.41, 0.22), ("aujourd", 0.3, 0.0), ("hui", 0.3, 0.0), ("l eau", 0.31, 0.1), ("est ce que", 0.5, 0.0), ("le", 0.1, 1.6),
               ("le chat", 0.42, 0.0), ("chanter", 0.4, 0.0), ("...", 0.05, 0.0), ("chat", 0.3, 0.05), ("dort", 0.3, 0.0), ("a cote", 0.5, 0.0),
               ("de", 0.1, 0.0), ("la", 0.1, 0.0), ("rivière", 0.8, 7.8), ("😀", 0.2, 0.0), ("été", 0.3, 0.0), ("le", 0.1, 0.0), ("chateau", 0.7, 0.1),
               ("fin.", 0.4, 12.1)]


_SEEDED = {}


def seeded_pair(n):
    """One seeded (gold, predicted) pair per size, shared by the align and the stats cases."""
    if n not in _SEEDED:
        rng = random.Random(1100 + n)
        gold = seeded_tier(rng, n)
        _SEEDED[n] = (gold, perturb(rng, gold))
    return _SEEDED[n]


def align_cases(rng):
    unit = lambda texts: tier([(t, 0.2, 0.0) for t in texts])      # noqa: E731
    cases = [
        ("french", tier(FRENCH_GOLD), tier(FRENCH_PRED)),
        ("ties_first_wins", unit(["le", "le", "le"]), unit(["le", "le", "la", "le", "le"])),
        ("collision_falls_to_lower_class", unit(["chat", "chat", "chat", "chat"]), unit(["le chat", "chat", "chats", "un chat noir"])),
        ("punctuation_gold_claims_first", unit(["...", "le", "—", "chat"]), unit(["le", "chat", "la"])),
        ("punctuation_pred", unit(["le", "chat", "dort"]), unit(["...", "—", "chat"])),
        ("punctuation_both", unit(["...", "?!"]), unit(["—", "le", "…"])),
        ("substring_either_way", unit(["eau", "aujourd'hui", "chateau"]), unit(["chateau", "hui", "eau"])),
        ("multi_word", unit(["le chat dort", "un  chien", "de la"]), unit(["chat", "le chat dort", "chien un", "la de"])),
        ("non_bmp", unit(["😀", "a😀b", "𝒳 y"]), unit(["b😀", "😀", "y 𝒳 z"])),
        ("nothing_matches", unit(["un", "deux"]), unit(["trois", "quatre"])),
        ("empty_pred", unit(["un", "deux"]), []),
        ("empty_gold", [], unit(["un"])),
        ("accents_differ", unit(["été", "à", "Noël"]), unit(["ete", "a", "noël"])),
    ]
    for n in (40, 300):
        cases.append((f"seeded_{n}",) + seeded_pair(n))
    return cases


def stats_cases(rng):
    french_gold, french_pred = tier(FRENCH_GOLD), tier(FRENCH_PRED)
    spanning = tier([("un", 0.5, 14.0), ("pont", 1.0, 0.0), ("loin", 0.5, 0.0), ("tard", 0.4, 14.0)])        # "pont": 14.5 .. 15.5 s
    shifted = [dict(iv, start=iv["start"] + 100.0, end=iv["end"] + 100.0) for iv in spanning]
    g300, p300 = seeded_pair(300)
    run = tier([(VOCAB[i % 14], 0.5, 0.0) for i in range(90)])                       # 45 s without a gap: mock segments close on their length
    cases = [
        ("run_longer_than_a_segment", run, retag([dict(iv) for iv in run if iv["i"] % 7]), None, 45.2),
        ("french_mock_segments", french_gold, french_pred, None, 47.3),
        ("french_model_segments", french_gold, french_pred,
         {"segments": [{"start": 0.0, "end": 2.5}, {"start": 2.5}, {"end": 3.0}, {"start": None, "end": 4.0}, {"start": 40.0, "end": 41.0}, {"start": 10.0, "end": 30.0}]}, 47.3),
        ("no_segments_key", french_gold, french_pred, {}, 47.3),
        ("interval_spans_two_windows", spanning, retag([dict(iv) for iv in spanning[1:]]), None, 31.0),
        ("all_windows_empty", spanning, retag(shifted), None, 31.5),
        ("nothing_matches_anywhere", spanning, tier([("xx", 0.5, 14.0), ("yy", 1.0, 0.0)]), None, 20.2),
        ("empty_pred", french_gold, [], None, 47.3),
        ("shorter_than_a_second", french_gold[:4], french_pred[:4], None, 0.9),
        ("duration_cuts_the_tier", french_gold, french_pred, None, 16.7),
        ("seeded_300", g300, p300, None, round(g300[-1]["end"] + 0.37, 2)),
    ]
    return cases


TEXTGRIDS = {
    "two_tiers_long_format": '''File type = "ooTextFile"
Object class = "TextGrid"

xmin = 0
xmax = 2.5
tiers? <exists>
size = 2
item []:
    item [1]:
        class = "IntervalTier"
        name = "words"
        xmin = 0
        xmax = 2.5
        intervals: size = 4
        intervals [1]:
            xmin = 0
            xmax = 0.5
            text = ""
        intervals [2]:
            xmin = 0.5
            xmax = 1.25
            text = " Bonjour, "
        intervals [3]:
            xmin = 1.25
            xmax = 1.5
            text = "   "
        intervals [4]:
            xmin = 1.5
            xmax = 2.5
            text = "aujourd'hui"
    item [2]:
        class = "IntervalTier"
        name = "phones"
        xmin = 0
        xmax = 2.5
        intervals: size = 2
        intervals [1]:
            xmin = 0.5
            xmax = 0.75
            text = "b"
        intervals [2]:
            xmin = 0.75
            xmax = 1.25
            text = "õ"
''',
    "quirks": '''intervals [1]:
    xmin = 0
    xmax = 1
    text = "deux
lignes"
intervals [2]:
    xmin = 1
    xmax = 2
    text = "il dit ""oui"" ici"
intervals [3]:
    xmin = 2.0
    xmax = 2.5e0
    text = "exposant"
intervals [4]: xmin = 3 xmax = 3.25 text = "une ligne"
intervals [5]:
    xmin = -1
    xmax = 4
    text = "negatif"
intervals [6]:
    xmin = 4
    xmax = 4.125
    text = "😀 l'eau"
''',
    "short_format": '''"ooTextFile"
"TextGrid"
0
1
<exists>
1
"IntervalTier"
"words"
0
1
1
0
1
"mot"
''',
}


def plain(x):
    """numpy scalars -> Python numbers (the json module writes inf / nan as Infinity / NaN)."""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if hasattr(x, "item"):
        return x.item()
    return x


def main():
    rng = random.Random(11)
    warnings.simplefilter("ignore")                        # np.mean([]) warns and returns nan: the value is what is recorded
    golden = {"tiers": [], "align": [], "stats": [], "textgrids": []}
    stored = {}

    def ref(intervals):
        """The tier's place in ``golden["tiers"]``: equal tiers are stored once."""
        rows = [[iv["start"], iv["end"], iv["text"], iv["duration"]] for iv in intervals]
        assert [iv["i"] for iv in intervals] == list(range(len(intervals)))
        key = json.dumps(rows)
        if key not in stored:
            stored[key] = len(golden["tiers"]); golden["tiers"].append(rows)
        return stored[key]
    for name, gold, pred in align_cases(rng):
        pairs = S.align_intervals(gold, pred)
        golden["align"].append({"name": name, "gold": ref(gold), "pred": ref(pred), "pairs": [[g["i"], p["i"]] for g, p in pairs]})
    for name, gold, pred, segments, duration in stats_cases(rng):
        mock = S.create_mock_segments_from_intervals(pred, duration)
        stats = S.calculate_multilevel_stats(gold, pred, mock if segments is None else segments, duration)
        golden["stats"].append({"name": name, "gold": ref(gold), "pred": ref(pred), "segments": segments, "audio_duration": duration,
                                "mock_segments": plain(mock), "mock_segments_20s": plain(S.create_mock_segments_from_intervals(pred, duration, 20)),
                                "stats": plain(stats)})
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in TEXTGRIDS.items():
            path = Path(tmp) / f"{name}.TextGrid"
            path.write_text(text, encoding="utf-8")
            golden["textgrids"].append({"name": name, "text": text, "intervals": S.parse_textgrid(str(path))})
    sections = []
    for key, cases in golden.items():                      # one case per line, no indentation
        sections.append(json.dumps(key) + ":[\n" + ",\n".join(json.dumps(c, ensure_ascii=False, separators=(",", ":")) for c in cases) + "\n]")
    with open(MG.OUT / "aligner_eval.json", "w", encoding="utf-8") as f:
        f.write("{" + ",\n".join(sections) + "}\n")
    print("wrote aligner_eval.json")


if __name__ == "__main__":
    main()
