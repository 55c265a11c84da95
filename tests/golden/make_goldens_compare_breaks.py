#!/usr/bin/env python3
"""Generate tests/golden/compare_breaks.json (G10) by RUNNING THE REFERENCE'S OWN ``AudioPipeline.compare_breaks``
(Code/audioPipeline.py:895-1074).

Runs only in the build container (needs the reference tree, see make_goldens.py).  The stand-ins of make_goldens.py replace the
third-party packages the reference imports; its ``textgrid`` stand-in serves the intervals this script registers (``fromFile`` is added
here, the reference's step reads its TextGrid through it).  Real pandas, real ``difflib``.  What is committed is data: per case the
TextGrid intervals, the rows of BDD_syntagme_for_synth.csv, ``tol_ms`` and the text of the ``pause_comparison_full.csv`` the reference wrote.
"""
import importlib
import json
import sys
import tempfile
from pathlib import Path

import pandas as pd

sys.path.insert(0, str(Path(__file__).resolve().parent))
import make_goldens as MG  # noqa: E402

CSV_COLUMNS = ["segment", "syntagme", "pause", "ssml"]


def grid(blocks):
    """[(words, silence_s or None), ...] -> intervals: 0.3 s per word, then the silence (an empty-mark interval) when there is one."""
    t, ivs = 0.0, []
    for words, sil in blocks:
        for w in words.split():
            ivs.append((t, t + 0.3, w)); t += 0.3
        if sil is not None:
            ivs.append((t, t + sil, "")); t += sil
    return ivs


def table(items):
    """[(segment, syntagme, pause_ms), ...]: a pause row is (segment, None, ms)."""
    return [{"segment": s, "syntagme": txt, "pause": p, "ssml": ""} for s, txt, p in items]


LONG = ("il etait une fois dans un pays tres lointain un roi qui avait trois filles et la plus jeune etait si belle que le soleil lui meme "
        "qui a pourtant vu tant de choses s etonnait chaque fois qu il eclairait son visage pres du chateau du roi il y avait une grande foret")


def cases():
    out = []
    # a clean one-to-one voice
    out.append(("one_to_one", 5,
                grid([("bonjour tout le monde", 0.412), ("voici la suite", 0.25), ("et la fin", 0.6)]),
                table([("segment_ph1", "Bonjour tout le monde,", 0), ("segment_ph1", None, 410), ("segment_ph1", "voici la suite", 0),
                       ("segment_ph1", None, 300), ("segment_ph2", "et la fin.", 0), ("segment_ph2", None, 598)])))
    # more CSV chunks than blocks
    out.append(("more_chunks", 5,
                grid([("le petit chat dort sur le tapis", 0.2), ("il reve", None)]),
                table([("s1", "le petit chat", 0), ("s1", None, 120), ("s1", "dort", 0), ("s1", None, 80), ("s1", "sur le tapis", 0), ("s1", None, 200),
                       ("s2", "il reve", 0), ("s2", None, 500)])))
    # more blocks than chunks
    out.append(("more_blocks", 10,
                grid([("le petit", 0.1), ("chat dort", 0.15), ("sur le", 0.05), ("tapis rouge", 0.33), ("et il reve", 0.7)]),
                table([("s1", "le petit chat dort sur le tapis rouge", 0), ("s1", None, 335), ("s1", "et il reve", 0), ("s1", None, 650)])))
    # two pause rows that land on one block
    out.append(("two_pauses_one_block", 5,
                grid([("un deux trois quatre cinq six", 0.5), ("sept", 0.1)]),
                table([("a", "un deux trois", 0), ("a", None, 150), ("a", "quatre cinq six", 0), ("a", None, 500), ("b", "sept", 0), ("b", None, 100)])))
    # punctuation, capitals and accents
    out.append(("punctuation_accents", 5,
                grid([("Où est-il allé", 0.3), ("À Noël peut-être", 0.22), ("ÇA alors", 0.18)]),
                table([(1, "« Où est-il allé ? »", 0), (1, None, 300), (1, "À NOËL, peut-être…", 0), (1, None, 225), (2, "Ça, alors !", 0), (2, None, 190)])))
    # a speech block of >= 200 normalised characters (autojunk)
    out.append(("autojunk_block", 5,
                grid([(LONG, 0.45), ("la fin", 0.2)]),
                table([("s1", "Il était une fois, dans un pays très lointain,", 0), ("s1", None, 100),
                       ("s1", "un roi qui avait trois filles", 0), ("s1", None, 120),
                       ("s1", LONG[120:], 0), ("s1", None, 450), ("s2", "la fin", 0), ("s2", None, 210)])))
    # repeated identical chunks (ties in the DP)
    out.append(("repeated_chunks", 5,
                grid([("oui oui", 0.1), ("oui oui", 0.2), ("non", 0.3), ("oui oui", 0.4)]),
                table([("r", "oui oui", 0), ("r", None, 100), ("r", "oui oui", 0), ("r", None, 200), ("r", "oui oui", 0), ("r", None, 300),
                       ("r", "non", 0), ("r", None, 300), ("r", "oui oui", 0), ("r", None, 405)])))
    # no pause rows at all
    out.append(("no_pause_rows", 5,
                grid([("bonjour", 0.2), ("au revoir", 0.3)]),
                table([("s1", "bonjour", 0), ("s1", "au revoir", 0)])))
    # nothing matches well: the low-quality warning, a leading silence, a block without a following silence
    out.append(("low_quality", 5,
                [(0.0, 0.5, "")] + [(a + 0.5, b + 0.5, m) for a, b, m in grid([("xyz", 0.2), ("qqq www", None)])],
                table([("s1", "bonjour le monde", 0), ("s1", None, 200), ("s1", "abc", 0), ("s1", None, 50)])))
    return out


def main():
    TextGrid, *_ = MG.install_stubs()

    def from_file(cls, f, name=None):
        tg = cls()
        tg.read(f)
        return tg
    TextGrid.fromFile = classmethod(from_file)
    ap = importlib.import_module("audioPipeline")
    golden = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, tol, intervals, rows in cases():
            root = Path(tmp) / name; root.mkdir()
            TextGrid.registry.clear(); TextGrid.registry["OUT.TextGrid"] = intervals
            pd.DataFrame(rows, columns=CSV_COLUMNS).to_csv(root / "BDD_syntagme_for_synth.csv", index=False)
            pipe = ap.AudioPipeline.__new__(ap.AudioPipeline)
            pipe.results_dir = root; pipe.bdd_syntagme_synth_csv = root / "BDD_syntagme_for_synth.csv"
            df = pipe.compare_breaks(tol_ms=tol)
            text = (root / "pause_comparison_full.csv").read_text(encoding="utf-8")
            golden.append({"name": name, "tol_ms": tol, "intervals": [list(iv) for iv in intervals], "csv_columns": CSV_COLUMNS, "csv_rows": rows,
                           "n_rows": int(len(df)), "pause_comparison_full_csv": text})
    with open(MG.OUT / "compare_breaks.json", "w", encoding="utf-8") as f:      # one case per line, no indentation: a few KB
        f.write("[\n" + ",\n".join(json.dumps(case, ensure_ascii=False, separators=(",", ":")) for case in golden) + "\n]\n")
    print("wrote compare_breaks.json")


if __name__ == "__main__":
    main()
