"""Device time of the alignment of "Compare Breaks" (k_seqmatch over all pairs + k_seqmatch_align) on a seeded voice of French-like
strings -- chunks of 15 .. 90 characters against blocks of 20 .. 350 -- beside the yardstick: stdlib ``difflib`` on this host, timed on a
sample of the same pairs and scaled to the full count (the reference calls it once per pair, Code/audioPipeline.py:970-978).  The two
paths are compared before anything is timed: the sample's ratios bit for bit, and the whole alignment when the voice is small enough
for the host DP.  HIP events via the engine's profiler.  usage: seqmatch_rate.py [n [m [sample [runs]]]]   (default 1000 1000 2000 5)"""
import os, random, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from difflib import SequenceMatcher
import numpy as np
import prosody_control_french_tts_amd as pkg
from seqmatch_cases import voice                            # the strings the tests use: one generator for both


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


args = [int(x) for x in sys.argv[1:]]
n, m, sample, runs = (args + [1000, 1000, 2000, 5][len(args):])[:4]
a, b = voice(n, m, seed=1212)
rng = random.Random(1213)
picks = [(rng.randrange(n), rng.randrange(m)) for _ in range(sample)]

eng = pkg.ProsodyEngine(0)
matches, sim = eng.seqmatch_align(a, b)
want = np.array([SequenceMatcher(None, a[i], b[j]).ratio() for i, j in picks])
got = np.array([sim[i, j] for i, j in picks])
if not np.array_equal(want.view(np.uint64), got.view(np.uint64)):
    sys.exit("device ratios differ from difflib on the sample: nothing timed")
if n * m <= 40000:
    from prosody_control_french_tts_amd import break_check
    host_matches, host_sim = break_check.align_host(a, b)
    if host_matches != [tuple(r) for r in matches.tolist()] or not np.array_equal(np.array(host_sim).view(np.uint64), sim.view(np.uint64)):
        sys.exit("device alignment differs from the host path: nothing timed")

t0 = time.perf_counter()
for i, j in picks:
    SequenceMatcher(None, a[i], b[j]).ratio()
host_us = (time.perf_counter() - t0) / sample * 1e6

eng.profile_enable(True); eng.profile_reset()
t0 = time.perf_counter()
for _ in range(runs):
    eng.seqmatch_align(a, b)
wall_ms = (time.perf_counter() - t0) / runs * 1e3
prof = eng.profile()
eng.profile_enable(False)
k1, k2 = prof["k_seqmatch"], prof["k_seqmatch_align"]
dev_ms = (k1["total_ms"] + k2["total_ms"]) / runs
print(f"{n} x {m} = {n * m} pairs, chunks 15..90 x blocks 20..350 characters, {len(matches)} aligned; host CPU: {cpu_model()}")
print(f"  k_seqmatch        {k1['total_ms'] / runs:10.3f} ms per call   {k1['flops'] / runs / (k1['total_ms'] / runs) / 1e6:8.2f} G cells/s ({k1['flops'] / runs / (n * m):.0f} swept cells per pair)")
print(f"  k_seqmatch_align  {k2['total_ms'] / runs:10.3f} ms per call   {k2['flops'] / runs / (k2['total_ms'] / runs) / 1e3:8.2f} M cells/s")
print(f"  device, both      {dev_ms:10.3f} ms per call   ({dev_ms / (n * m) * 1e6:.1f} ns per pair); whole call with packing and copies {wall_ms:.1f} ms")
print(f"  difflib, one core {host_us:10.1f} us per pair on {sample} of the same pairs -> {host_us * n * m / 1e6:.1f} s for all pairs, before the Python DP")
print(f"  difflib / device  {host_us * n * m / 1e3 / dev_ms:10.0f} x")
eng.close()
