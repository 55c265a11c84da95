"""Device time of the whisperX alignment (pce_wx_align: k_wx_rowmax + k_wx_trellis + k_wx_backtrack) on seeded log-softmax rows: a batch of
256 clips x 500 frames x 150 tokens at V = 32 (15 % wildcards), and one clip of 1 500 frames x 400 tokens (whisperX's longest segment at
wav2vec2's stride).  Before anything is timed a small batch is compared with the CPU restatement (tests/wx_restatement.py), every output
bit for bit.  Beside it: pce_ctc_align on the same emissions (the other aligner's programme: 2 L + 1 states, back-pointers instead of a
stored trellis), and the numpy restatement on one core of this host, one clip of the batch's shape (whisperx itself runs a Python loop
over torch rows, one segment at a time).  HIP events via the engine's profiler.
usage: wx_rate.py [clips [frames [tokens [runs]]]]   (default 256 500 150 5)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch                                                   # (before libpce.so: one HIP runtime for both)
import prosody_control_french_tts_amd as pkg
import wx_restatement as WR

V = 32


def report(k, ms, work):
    if k in ("k_wx_backtrack", "k_ctc_trace"):
        rate = f"{work / ms / 1e3:8.2f} M frames/s"
    elif k == "k_wx_rowmax":
        rate = f"{work * 4 / ms / 1e6:8.2f} GB/s read"
    else:
        rate = f"{work / ms / 1e6:8.2f} G cells/s"
    print(f"  {k:14s} {ms:10.3f} ms per call   {rate}")


def timed(call, runs, prefix):
    call()                                                       # allocations
    eng.profile_enable(True); eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(runs):
        call()
    wall = (time.perf_counter() - t0) / runs * 1e3
    prof = eng.profile(); eng.profile_enable(False)
    return {k: (v["total_ms"] / runs, v["flops"] / runs) for k, v in prof.items() if k.startswith(prefix)}, wall


def show(prof, wall, n):
    for k, (ms, work) in prof.items():
        report(k, ms, work)
    dev = sum(ms for ms, _ in prof.values())
    print(f"  device, all    {dev:10.3f} ms per call   ({dev / n * 1e3:.1f} us per clip); whole call with packing and copies {wall:.1f} ms")


def same(g, w):
    if g["status"] != w["status"] or not np.array_equal(g["trellis"].view(np.int32), w["trellis"].view(np.int32)):
        return False
    if w["status"] != 0:
        return True
    return np.array_equal(g["path_tok"], w["path_tok"]) and np.array_equal(g["path_lp"].view(np.int32), w["path_lp"].view(np.int32)) and g["score"] == w["score"]


args = [int(x) for x in sys.argv[1:]]
n, T, J, runs = (args + [256, 500, 150, 5][len(args):])[:4]
rng = np.random.default_rng(2020)
eng = pkg.ProsodyEngine(0)

small = [WR.make_case(s, t, j, V, wild=w) for s, (t, j, w) in enumerate(((1, 1, 0.0), (40, 9, 0.15), (300, 140, 0.0), (700, 300, 0.15), (5, 9, 0.0), (520, 513, 1.0)))]
for W in (1, 2, 8):
    got = eng.wx_align([c[0] for c in small], [c[1] for c in small], beam_width=W, return_trellis=True)
    if not all(same(g, WR.align(c[0], c[1], 0, W)) for g, c in zip(got, small)):
        sys.exit(f"device alignment differs from the restatement on the small batch (beam width {W}): nothing timed")

cases = [WR.make_case(100 + k, T, J, V, wild=0.15) for k in range(n)]
em = torch.from_numpy(np.stack([c[0] for c in cases])).to(f"cuda:{eng.device}")
tok = [c[1] for c in cases]
t0 = time.perf_counter()
WR.align(cases[0][0], tok[0], 0, 2)
host_ms = (time.perf_counter() - t0) * 1e3
print(f"{n} clips x {T} frames x {J} tokens, V = {V}, 15 % wildcards, beam width 2: {n * T * J / 1e6:.1f} M trellis cells, emissions resident on the device")
show(*timed(lambda: eng.wx_align(em, tok), runs, "k_wx"), n)
print(f"  numpy restatement, one core: {host_ms:.1f} ms for one clip -> {host_ms * n / 1e3:.2f} s for the batch")
tg = [np.where(t < 1, 1, t).astype(np.int32) for t in tok]      # (CTC targets: no wildcard, no blank)
print(f"pce_ctc_align on the same emissions and as many targets ({2 * J + 1} states, 2-bit back-pointers):")
show(*timed(lambda: eng.ctc_align(em, tg), runs, "k_ctc"), n)

T1, J1 = 1500, 400
e1, tok1 = WR.make_case(7, T1, J1, V, wild=0.15)
em1 = torch.from_numpy(e1[None]).to(f"cuda:{eng.device}")
print(f"1 clip x {T1} frames x {J1} tokens (one workgroup of 128 threads)")
show(*timed(lambda: eng.wx_align(em1, [tok1]), runs, "k_wx"), 1)
show(*timed(lambda: eng.ctc_align(em1, [np.where(tok1 < 1, 1, tok1).astype(np.int32)]), runs, "k_ctc"), 1)
eng.close()
