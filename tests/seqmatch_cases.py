"""The string pairs on which a SequenceMatcher kernel can go wrong, shared by tests/test_compare_breaks_host.py (the restatement against
``difflib``) and tests/test_gpu_seqmatch.py (the kernels against ``difflib``).  Seeded: the same pairs everywhere."""
import json
import os
import random
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "pce.h"), encoding="utf-8").read()
ROW_LDS = int(re.search(r"#define PCE_SEQMATCH_ROW_LDS (\d+)", _HEADER).group(1))
STACK_LDS = int(re.search(r"#define PCE_SEQMATCH_STACK_LDS (\d+)", _HEADER).group(1))
MAX_PAIRS = 1 << int(re.search(r"#define PCE_SEQMATCH_MAX_PAIRS \(\(int64_t\)1 << (\d+)\)", _HEADER).group(1))

WORDS = ("le la les un une des de du et ou que qui il elle ne pas dans sur avec pour bonjour monde voila phrase tres longue ici oui non mer puis "
         "petit chat dort tapis rouge reve roi fille soleil visage chateau grande foret etait avait chaque fois pays lointain").split()


def french(rng, lo, hi):
    """A French-like string of lo .. hi characters."""
    want = rng.randint(lo, hi)
    s = rng.choice(WORDS)
    while len(s) < want:
        s += " " + rng.choice(WORDS)
    return s[:want]


def rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def distinct(start, n):
    return "".join(chr(start + i) for i in range(n))


def shape_cases():
    """[(name, a, b), ...]: every shape the kernel treats differently."""
    rng = random.Random(20260)
    out = [("empty_a", "", "abc"), ("empty_b", "abc", ""), ("both_empty", "", ""), ("one_equal", "x", "x"), ("one_differs", "x", "y"),
           ("one_in_many", "c", "abcabc"), ("many_in_one", "abcabc", "c")]
    for la in (63, 64, 65):                                 # the 64-column chunk, either side
        for lb in (63, 64, 65):
            b = rand(rng, lb, "abcd")
            a = (b[lb // 2:] + rand(rng, la, "abcd"))[:la]
            out.append((f"chunk_{la}x{lb}", a, b))
    out.append(("run_across_chunks", distinct(0x400, 140)[50:80], distinct(0x400, 140)))
    for lb in (199, 200, 201, 300):                         # autojunk starts at len(b) == 200
        b = french(rng, lb, lb)
        out.append((f"junk_{lb}", french(rng, 60, 90), b))
        out.append((f"junk_{lb}_substring", b[lb // 3: lb // 3 + 70], b))
    # the popular threshold: len(b) = 200 -> more than 200 // 100 + 1 = 3 occurrences
    for times, where in ((3, (5, 50, 100)), (4, (5, 50, 100, 150))):
        b = list(distinct(0x400, 200))
        for p in where:
            b[p] = "x"
        b = "".join(b)
        out.append((f"popular_{times}_inside_run", b[46:55], b))
        out.append((f"popular_{times}_alone", "xx", b))
        out.append((f"popular_{times}_leading", "x" + b[51:60], b))
    # a run anchored on a rare element with popular neighbours on both sides: the extension
    b = "ab" * 75 + "Z" + "ab" * 75
    out.append(("extension_both_sides", "abab" + "Z" + "abab", b))
    out.append(("extension_to_the_range_ends", "b" + "Z" + "a", b))
    out.append(("only_popular_matches", "abab", "ab" * 150))     # k = 0 from the sweep, the right extension alone finds a block
    # distinct separators alternating with repeated pairs: one block per pair, and every block leaves a range on the stack
    reps = 60
    out.append(("deep_stack", "".join(chr(0x2000 + i) + "ab" for i in range(reps)), "-ab" * reps))
    out.append(("deep_stack_lds_only", "".join(chr(0x2000 + i) + "ab" for i in range(STACK_LDS - 1)), "-ab" * (STACK_LDS - 1)))
    # the LDS row capacity and one element past it (the global row), against 8 elements
    alphabet = distinct(0x3000, 1000)
    for lb in (ROW_LDS, ROW_LDS + 1):
        b = rand(rng, lb, alphabet)
        out.append((f"row_{lb}_tail", b[lb - 8:], b))
        out.append((f"row_{lb}_across_chunk", b[60:68], b))
    b = rand(rng, ROW_LDS + 1, alphabet)                    # many rows over the global row, then narrower ranges in LDS
    out.append(("row_global_many_rows", b[100:130] + "?" + b[1500:1540], b))
    # code points above 0xFFFF; a pair that differs in the high 16 bits only
    out.append(("astral", "\U0001F600ab\U0010FFFF\U0001F601", "ab\U0001F600\U0010FFFF\U0001F601"))
    out.append(("high_bits_differ", "\U00010041\U00010042", "AB"))
    out.append(("high_bits_mixed", "A\U00010041A", "\U00010041A\U00020041"))
    return out


def tie_cases(n=400):
    """Random strings over three symbols, lengths 0 .. 40: full of equal-length runs, where a wrong tie-break changes the total."""
    rng = random.Random(4040)
    return [(rand(rng, rng.randint(0, 40), "abc"), rand(rng, rng.randint(0, 40), "abc")) for _ in range(n)]


def voice(n, m, seed):
    """n CSV-like chunks against m TextGrid-like blocks of French-like text (blocks reach past 200 characters)."""
    rng = random.Random(seed)
    return [french(rng, 15, 90) for _ in range(n)], [french(rng, 20, 350) for _ in range(m)]


def golden_cases():
    with open(os.path.join(ROOT, "tests", "golden", "compare_breaks.json"), encoding="utf-8") as f:
        return json.load(f)


def write_case(case, folder):
    """A golden case's two input files -> (TextGrid path, CSV path)."""
    import pandas as pd
    from prosody_control_french_tts_amd.textgrid_io import IntervalTier, TextGrid, write_textgrid
    tier = IntervalTier("words")
    tier.intervals = [(float(a), float(b), str(m)) for a, b, m in case["intervals"]]
    tg_path, csv_path = os.path.join(folder, "OUT.TextGrid"), os.path.join(folder, "BDD_syntagme_for_synth.csv")
    write_textgrid(TextGrid([tier], 0.0, tier.intervals[-1][1]), tg_path)
    pd.DataFrame(case["csv_rows"], columns=case["csv_columns"]).to_csv(csv_path, index=False)
    return tg_path, csv_path
