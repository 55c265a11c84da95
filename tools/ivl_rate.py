"""Device time of the aligner evaluation (whisper_testing/splitting.py: k_ivl_classes + k_ivl_claim behind one ``evaluate_textgrids``
call) on a seeded gold word tier against four predicted tiers -- entire audio, 15 s windows and mock sentences of each -- beside the
``engine=None`` path of the same module on one core of this host.  The two paths are compared before anything is timed: every statistic
bit for bit.  HIP events via the engine's profiler; five calls after a warm-up.
usage: ivl_rate.py [words [host_words [runs]]]   (default 8000 8000 5; host_words: the tier size the host path is timed on)"""
import os, random, sys, tempfile, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd.whisper_testing import splitting as SP
from ivl_cases import same_stats

SYLLABLES = ["ba", "che", "dou", "fi", "gra", "lan", "mé", "noi", "pon", "qui", "ré", "sou", "ton", "vé", "zi", "l'", "au", "eu", "é", "ç"]
COMMON = ["le", "la", "les", "de", "des", "un", "une", "et", "à", "il", "elle", "que", "qui", "est-ce", "aujourd'hui", "—", "..."]


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def tiers(n, seed):
    """A gold tier of n words (half of them from 17 common ones, the rest from 1 500 made-up ones) and four aligners' tiers: words dropped,
    substituted, doubled, boundaries moved, at four error rates."""
    rng = random.Random(seed)
    rare = ["".join(rng.choice(SYLLABLES) for _ in range(rng.randint(1, 4))) for _ in range(1500)]
    gold, t = [], 0.0
    for _ in range(n):
        if rng.random() < 0.06:
            t += rng.uniform(1.0, 2.5)
        d = rng.uniform(0.08, 0.6)
        word = rng.choice(COMMON) if rng.random() < 0.5 else rng.choice(rare)
        gold.append((t, t + d, word + ("," if rng.random() < 0.1 else ""))); t += d
    preds = {}
    for name, err in (("whisper", 0.05), ("ctc", 0.10), ("whisperx", 0.15), ("nemo", 0.25)):
        out = []
        for a, b, w in gold:
            r = rng.random()
            if r < err / 2:
                continue
            if r < err:
                w = rng.choice(COMMON + rare)
            a = max(a + rng.uniform(-0.03, 0.03), 0.0); b = b + rng.uniform(-0.03, 0.03)
            out.append((a, b, w))
            if r > 1 - err / 4:
                out.append((b, b + 0.02, w))
        preds[name] = out
    return gold, preds, t


def write(path, intervals):
    with open(path, "w", encoding="utf-8") as f:
        for n, (a, b, w) in enumerate(intervals):
            f.write(f'        intervals [{n + 1}]:\n            xmin = {a:.6f}\n            xmax = {b:.6f}\n            text = "{w}"\n')
    return path


def files(tmp, n, seed):
    gold, preds, duration = tiers(n, seed)
    sub = os.path.join(tmp, str(n)); os.makedirs(sub, exist_ok=True)
    return write(os.path.join(sub, "gold.TextGrid"), gold), {k: write(os.path.join(sub, f"{k}.TextGrid"), v) for k, v in preds.items()}, duration, \
        len(gold), {k: len(v) for k, v in preds.items()}


args = [int(x) for x in sys.argv[1:]]
words, host_words, runs = (args + [8000, 8000, 5][len(args):])[:3]
warnings.simplefilter("ignore")
eng = pkg.ProsodyEngine(0)
batch, match_on_device = {}, eng.interval_match


def counted(tables, problems):                             # what one call sends down: its problems, the longest gold list among them
    batch.update(problems=len(problems), longest=max(len(g) for _, g, _ in problems))
    return match_on_device(tables, problems)


eng.interval_match = counted
with tempfile.TemporaryDirectory() as tmp:
    gold_path, pred_paths, duration, n_gold, n_pred = files(tmp, words, 2424)
    dev = SP.evaluate_textgrids(gold_path, pred_paths, duration, engine=eng)              # (the warm-up)
    if host_words == words:
        t0 = time.perf_counter()
        host = SP.evaluate_textgrids(gold_path, pred_paths, duration, engine=None)
        host_s = time.perf_counter() - t0
    else:
        h_gold, h_preds, h_duration, _, _ = files(tmp, host_words, 2424)
        same_stats(SP.evaluate_textgrids(h_gold, h_preds, h_duration, engine=eng), SP.evaluate_textgrids(h_gold, h_preds, h_duration, engine=None), bits=True)
        t0 = time.perf_counter()
        SP.evaluate_textgrids(h_gold, h_preds, h_duration, engine=None)
        host_s = time.perf_counter() - t0
        host = None
    if host is not None:
        try:
            same_stats(dev, host, bits=True)
        except AssertionError as e:
            sys.exit(f"device statistics differ from the engine=None path: nothing timed ({e})")
    eng.profile_enable(True); eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(runs):
        SP.evaluate_textgrids(gold_path, pred_paths, duration, engine=eng)
    wall_ms = (time.perf_counter() - t0) / runs * 1e3
    prof = eng.profile()
    eng.profile_enable(False)
k1, k2 = prof["k_ivl_classes"], prof["k_ivl_claim"]
print(f"gold tier of {n_gold} words, {duration / 60:.1f} min, against {n_pred}: entire audio, 15 s windows, mock sentences; host CPU: {cpu_model()}")
print(f"  equal to the engine=None path, bit for bit: {'yes, at this size' if host is not None else f'yes, at {host_words} words'}")
print(f"  k_ivl_classes     {k1['total_ms'] / runs:10.3f} ms per call   {k1['flops'] / runs / (k1['total_ms'] / runs) / 1e6:8.2f} G text pairs/s ({k1['launches'] // runs} launch)")
print(f"  k_ivl_claim       {k2['total_ms'] / runs:10.3f} ms per call   {k2['flops'] / runs / (k2['total_ms'] / runs) / 1e3:8.2f} M gold steps/s ({k2['launches'] // runs} launch)")
print(f"                    {batch['problems']} problems, one wave each; the longest walks {batch['longest']} gold intervals: at most "
      f"{k2['total_ms'] / runs / batch['longest'] * 1e3:.2f} us per step of that chain")
print(f"  whole call        {wall_ms:10.1f} ms: parsing, normalisation, interning, overlap tests, copies, metrics ({runs} calls after a warm-up)")
print(f"  engine=None       {host_s * 1e3:10.1f} ms on one core, once, gold tier of {host_words} words (the bitmap restatement, not the reference's pair loop)")
eng.close()
