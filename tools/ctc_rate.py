"""Device time of the CTC forced alignment (pce_ctc_align: k_ctc / k_ctc_general + k_ctc_trace) on seeded log-softmax rows: a batch of
256 clips x 500 frames x 150 targets at V = 32, and one clip of 30 000 frames (x 3 000 targets, the general form).  Before anything is
timed a small batch is compared with the CPU restatement (tests/ctc_restatement.py), every output bit for bit.  The yardstick beside it is
that restatement in numpy on this host, one clip of the batch's shape (the reference's tools run a single-threaded loop per file).  HIP
events via the engine's profiler.  usage: ctc_rate.py [clips [frames [targets [runs]]]]   (default 256 500 150 5)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch                                                   # (before libpce.so: one HIP runtime for both)
import prosody_control_french_tts_amd as pkg
import ctc_restatement as CR

V = 32


def rows(rng, T):
    x = rng.standard_normal((T, V)) * 2.0
    return (x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))).astype(np.float32)


def report(k, ms, work):
    rate = f"{work / ms / 1e3:8.2f} M frames/s" if k == "k_ctc_trace" else f"{work / ms / 1e6:8.2f} G cells/s"
    print(f"  {k:14s} {ms:10.3f} ms per call   {rate}")


def timed(eng, em, tg, runs, **kw):
    eng.ctc_align(em, tg, **kw)                                  # allocations
    eng.profile_enable(True); eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(runs):
        eng.ctc_align(em, tg, **kw)
    wall = (time.perf_counter() - t0) / runs * 1e3
    prof = eng.profile(); eng.profile_enable(False)
    return {k: (v["total_ms"] / runs, v["flops"] / runs) for k, v in prof.items() if k.startswith("k_ctc")}, wall


args = [int(x) for x in sys.argv[1:]]
n, T, L, runs = (args + [256, 500, 150, 5][len(args):])[:4]
rng = np.random.default_rng(1818)
eng = pkg.ProsodyEngine(0)

small = [(rows(rng, t), rng.integers(1, V, size=l).astype(np.int32)) for t, l in ((1, 1), (40, 9), (300, 140), (700, 300), (90, 0), (5, 9))]
got = eng.ctc_align([c[0] for c in small], [c[1] for c in small])
if not all(CR.same_result(g, CR.forced_align(*c)) for g, c in zip(got, small)):
    sys.exit("device alignment differs from the restatement on the small batch: nothing timed")

em = torch.from_numpy(np.stack([rows(rng, T) for _ in range(n)])).to(f"cuda:{eng.device}")
tg = [rng.integers(1, V, size=L).astype(np.int32) for _ in range(n)]
t0 = time.perf_counter()
CR.forced_align(em[0].cpu().numpy(), tg[0])
host_ms = (time.perf_counter() - t0) * 1e3
prof, wall = timed(eng, em, tg, runs)
cells = n * T * (2 * L + 1)
print(f"{n} clips x {T} frames x {L} targets, V = {V}: {cells / 1e6:.1f} M trellis cells, emissions resident on the device")
for k, (ms, work) in prof.items():
    report(k, ms, work)
dev = sum(ms for ms, _ in prof.values())
print(f"  device, all    {dev:10.3f} ms per call   ({dev / n * 1e3:.1f} us per clip); whole call with packing and copies {wall:.1f} ms")
print(f"  numpy restatement, one core: {host_ms:.1f} ms for one clip -> {host_ms * n / 1e3:.2f} s for the batch")

T1, L1 = 30000, 3000
em1 = torch.from_numpy(rows(rng, T1)[None]).to(f"cuda:{eng.device}")
tg1 = [rng.integers(1, V, size=L1).astype(np.int32)]
prof, wall = timed(eng, em1, tg1, max(1, runs // 2))
print(f"1 clip x {T1} frames x {L1} targets ({2 * L1 + 1} states: the general form)")
for k, (ms, work) in prof.items():
    report(k, ms, work)
tg2 = [rng.integers(1, V, size=2000).astype(np.int32)]
prof, wall = timed(eng, em1, tg2, max(1, runs // 2), form="register")
print(f"1 clip x {T1} frames x 2000 targets (4001 states: the register form on 1 024 threads)")
for k, (ms, work) in prof.items():
    report(k, ms, work)
eng.close()
