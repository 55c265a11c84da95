"""Device time of CREPE pitch tracking (pce_crepe_run: frames, six convolution blocks, classifier, Viterbi) for a batch of clips at `full` widths
with random weights (crepe_weights.random_init: no trained checkpoint is needed to time the arithmetic), at the scoring notebook's hop (512 at
44.1 kHz = 185 samples at 16 kHz) and batch_size 4096.  Prints ms per run, the kernels' shares and the achieved FLOP/s of block 2 (M = 128 rows per
frame, N = 128, K = 65 536: 85 % of the work).  usage: crepe_rate.py [clips [seconds [runs [capacity]]]]   (default 256 10 3 full)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd import crepe_weights as CW, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
capacity = sys.argv[4] if len(sys.argv) > 4 else "full"
hop = CW.hop_at_16k(512, 44100)
fmin, fmax = 440.0 * 2.0 ** ((36 - 69) / 12.0), 440.0 * 2.0 ** ((84 - 69) / 12.0)      # C2, C6
eng = pkg.ProsodyEngine(0)
eng.crepe_load(*CW.fold(CW.random_init(capacity, 0)))
eng.upload(synth.synth_batch(n, seconds, 16000, first=0), 16000)
frames = sum(CW.n_frames(int(k), hop) for k in eng.clip_lengths)
eng.crepe(hop, fmin, fmax); eng.sync()                                                   # warm-up: allocations, code objects
eng.profile_enable(True); eng.profile_reset()
t0 = time.perf_counter()
for _ in range(runs):
    eng.crepe(hop, fmin, fmax)
eng.sync()
wall = (time.perf_counter() - t0) / runs * 1e3
prof = eng.profile()
names = ["k_crepe_frames", "k_crepe_conv1", "k_crepe_conv:block2", "k_crepe_conv", "k_crepe_classifier", "k_crepe_decode", "k_crepe_viterbi"]
dev = sum(prof[k]["total_ms"] for k in names) / runs
print(f"{n} clips x {seconds:g} s, {capacity}: {frames} frames at hop {hop}; {dev:.2f} ms device per run, {wall:.2f} ms wall (fetches included); "
      f"{n * seconds / (dev / 1e3):.0f} x real time")
for k in names:
    ms = prof[k]["total_ms"] / runs
    fl = prof[k].get("flops", 0.0) / runs
    rate = f"{fl / (ms * 1e-3) / 1e12:8.1f} TFLOP/s" if fl and ms else ""
    print(f"  {k:22s} {ms:9.3f} ms  {100 * ms / dev:5.1f} %  {rate}")
eng.close()
