"""Cases shared by tests/test_ivl_host.py (the module's host path against golden G11) and tests/test_gpu_ivl.py (the kernels against
the host path): the golden, the comparison of statistics, a plain scan by the reference's rule, and the seeded shapes on which
k_ivl_classes / k_ivl_claim can go wrong."""
import json
import math
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "aligner_eval.json"), encoding="utf-8"))
# a tier is stored once, as [start, end, text, duration] rows; a case names its tiers by their place: the interval dicts the generator
# gave the reference, each tagged with its index
_TIERS = [[{"start": s, "end": e, "text": t, "duration": d, "i": i} for i, (s, e, t, d) in enumerate(rows)] for rows in GOLDEN["tiers"]]
for _case in GOLDEN["align"] + GOLDEN["stats"]:
    _case["gold"], _case["pred"] = _TIERS[_case["gold"]], _TIERS[_case["pred"]]
EXACT_KEYS = {"ARR", "count", "window_count", "sentence_count", "word_count", "window_start"}
# float statistics against the golden: only numpy's summation order may differ between the machine that recorded it and this one, at
# most n * 2^-53 relative with n <= 2 000 summed values (2.2e-13); the bound the tests hold is 1e-12
REL = 1e-12

VOCAB = ["le", "la", "de", "un", "une", "et", "chat", "château", "chante", "chanter", "leau", "eau", "aujourdhui", "hui", "", "bonjour",
         "estce", "ce", "que", "quil", "il", "a", "à", "été", "ete", "le chat", "de la", "😀", "un  chat", "chat noir"]
assert len(VOCAB) == 30


def same_stats(got, want, bits=False, path=""):
    """``got`` equals ``want``: dicts and lists alike in shape, counts and ARR exact, inf and nan equal in kind, every other float within
    REL (``bits``: identical)."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            same_stats(got[k], want[k], bits or k in EXACT_KEYS, f"{path}/{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            same_stats(g, w, bits, f"{path}[{i}]")
    elif isinstance(want, float) or isinstance(got, float):
        g, w = float(got), float(want)
        if math.isnan(w) or math.isinf(w) or bits:
            assert (math.isnan(g) and math.isnan(w)) or g == w, (path, g, w)
        else:
            assert math.isfinite(g) and abs(g - w) <= REL * abs(w), (path, g, w)
    else:
        assert got == want, (path, got, want)


def scan(gold, pred, gold_indices=None, pred_indices=None):
    """The reference's rule as a plain scan over (gold, unclaimed predicted) pairs of normalised texts -> [(match, class), ...]."""
    gold_indices = range(len(gold)) if gold_indices is None else gold_indices
    members = range(len(pred)) if pred_indices is None else sorted(set(pred_indices))
    used, out = set(), []
    for g in gold_indices:
        best, best_class = -1, 0
        for j in members:
            if j in used:
                continue
            a, b = gold[g], pred[j]
            k = 3 if a == b else 2 if (a in b or b in a) else 1 if any(w in b.split() for w in a.split()) else 0
            if k > best_class:
                best, best_class = j, k
        if best >= 0:
            used.add(best)
        out.append((best, best_class))
    return out


def bitmap_edges():
    """(tables, problems): tiers of every size at which a word of the class rows ends, one lane owns a second word (4 097) or there is
    nothing at all; all predictions identical; the only match in the last bit of the last word."""
    rng = random.Random(3)
    tables, problems = [], []
    for P in (0, 1, 63, 64, 65, 128, 129, 4097):
        for G in (0, 1, 65):
            tables.append(([rng.choice(VOCAB) for _ in range(G)], [rng.choice(VOCAB) for _ in range(P)]))
            problems.append((len(tables) - 1, list(range(G)), None))
            problems.append((len(tables) - 1, list(range(G))[::-1], sorted(rng.sample(range(P), P // 2))))
        tables.append((["le"] * 65, ["le"] * P))
        problems.append((len(tables) - 1, list(range(65)), None))
        if P:
            tables.append((["cible", "cible", "la cible"], ["x"] * (P - 1) + ["cible"]))
            problems.append((len(tables) - 1, [0, 1, 2], None))
            problems.append((len(tables) - 1, [2, 0], [P - 1]))
    # k_ivl_claim keeps words 0 .. 127 of a problem's bitmap in registers and the rest in LDS: claims that run from word 127 into
    # word 128 and on, a lane that owns two words in LDS (word 192: index 12 288), the only match in the last bit of an LDS word
    for P in (8193, 12345):
        tables.append(([rng.choice(VOCAB) for _ in range(65)], [rng.choice(VOCAB) for _ in range(P)]))
        problems.append((len(tables) - 1, list(range(65)), None))
        problems.append((len(tables) - 1, list(range(65)), list(range(8100, P))))
        tables.append((["le"] * 200, ["le"] * P))
        problems.append((len(tables) - 1, list(range(200)), list(range(8120, 8140)) + list(range(P - 50, P))))
        tables.append((["cible", "cible", "la cible"], ["x"] * (P - 1) + ["cible"]))
        problems.append((len(tables) - 1, [0, 1, 2], None))
    return tables, problems


def text_cases():
    """(tables, problems): substrings at the start, in the middle and at the end, a restart inside a partial match, equal lengths that
    differ in the last code point, the longer text on either side, empty texts on either side and on both; shared first, last and only
    words, duplicated words, runs of spaces.  One gold row against one prediction each, so every pair's class is read off alone."""
    pairs = [("abc", "abcdef"), ("cde", "abcdef"), ("def", "abcdef"), ("abcdef", "abc"), ("abcdef", "cde"), ("abcdef", "def"),
             ("aab", "aaab"), ("aaab", "aab"), ("abab", "aabab"), ("abcd", "abce"), ("abce", "abcd"), ("abcd", "abcd"), ("", "abc"),
             ("abc", ""), ("", ""), ("a", "b"), ("a", "a"), ("ab", "ba"), ("été", "ete"), ("😀", "a😀b"), ("a😀b", "😀"), ("😀", "😁"),
             ("le chat dort", "le chien"), ("le chat dort", "il dort"), ("chat", "un chat noir"), ("le chat", "chat le"),
             ("le le le", "la le"), ("un  chat", "chat   un"), ("a b c d e f g h", "h"), ("x", "a b c d e f g x"), ("ab cd", "abcd"),
             ("abcd", "ab cd"), ("ab cd", "cd ab"), ("ab cd", "b c"), ("long texte de plusieurs mots sans rien en commun", "autre phrase"),
             ("a" * 70 + "b", "a" * 140 + "b"), ("a" * 140 + "b", "a" * 70 + "b"), ("a" * 70 + "b", "a" * 140 + "c")]
    tables = [([a], [b]) for a, b in pairs]
    # ... and all of them as one table: 38 x 38 pairs with texts of unequal length in one wave
    tables.append(([a for a, _ in pairs], [b for _, b in pairs]))
    problems = [(t, list(range(len(g))), None) for t, (g, _) in enumerate(tables)]
    return tables, problems


def membership_cases():
    """(tables, problems): bitmaps that exclude the best class, then the second best; a gold list that is a strict subset, in order;
    the same prediction wanted by two gold rows of one problem but free again in the next."""
    gold = ["chat", "le chat", "chat", "chien"]
    pred = ["chat", "chats", "un chat", "chat", "loup", "chien"]
    tables = [(gold, pred)]
    problems = [(0, [0, 1, 2, 3], None), (0, [0, 1, 2, 3], [1, 2, 3, 4, 5]), (0, [0, 2], [1, 2, 4]), (0, [0, 2], [2, 4]), (0, [0], [4]),
                (0, [1, 3], None), (0, [2], [0, 3]), (0, [0, 2, 0], [0, 3]), (0, [3, 3], None), (0, [0, 1, 2, 3], [])]
    return tables, problems


def random_batch(seed=24, n_tables=8, n_problems=200, max_len=300):
    rng = random.Random(seed)
    tables = []
    for _ in range(n_tables):
        G, P = rng.randint(1, max_len), rng.randint(0, max_len)
        tables.append(([rng.choice(VOCAB) for _ in range(G)], [rng.choice(VOCAB) for _ in range(P)]))
    tables[0] = ([rng.choice(VOCAB) for _ in range(max_len)], [rng.choice(VOCAB) for _ in range(max_len)])
    problems = []
    for _ in range(n_problems):
        t = rng.randrange(n_tables)
        G, P = len(tables[t][0]), len(tables[t][1])
        kind = rng.random()
        if kind < 0.2:
            problems.append((t, list(range(G)), None))
        else:                                              # a window: a run of gold rows and a run of predictions around the same place
            a = rng.randrange(G); b = min(G, a + rng.randint(0, 40))
            lo = min(P, max(0, a * P // G - rng.randint(0, 10))); hi = min(P, lo + rng.randint(0, 50))
            problems.append((t, list(range(a, b)), list(range(lo, hi))))
    return tables, problems


def expect(tables, problems):
    return [scan(tables[t][0], tables[t][1], g, p) for t, g, p in problems]


def as_pairs(results):
    return [list(zip(m.tolist(), c.tolist())) for m, c in results]
