"""Device time of silence detection (k_ms_energy, k_silence_scan, the three launches of k_silence_ranges) beside k_energy -- the yardstick for
"the PCM is read once" -- on the same resident batch in the same run: the C4 shard (1 250 x 10 s at 16 kHz, 400 MB) and one 60-minute
recording at 44.1 kHz (318 MB), both beyond the Infinity Cache.  min_silence_len 1000, -50 dB, seek_step 1: the reference's call.  HIP events
via the engine's profiler; bytes of k_ms_energy = the PCM plus the 8 bytes per millisecond it writes.  usage: silence_rate.py [runs]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd import synth

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
base = synth.synth_batch(256, 10.0, 16000, first=0)
hour = np.concatenate([base[i % 256] for i in range(993)])[:3600 * 44100]
eng = pkg.ProsodyEngine(0)
for label, clips, rate in (("1250 x 10 s, 16 kHz", [base[i % 256] for i in range(1250)], 16000), ("1 x 60 min, 44.1 kHz", [hour], 44100)):
    eng.upload(clips, rate)
    sl = eng.whole_clip_slices()
    nbytes = sum(len(c) for c in clips) * 2
    n_ms = sum(round(1000 * len(c) / rate) for c in clips)
    per_run = {}
    for names, run in ((("k_energy",), lambda: eng.energy_run(sl, 500)),
                       (("k_ms_energy", "k_silence_scan", "k_silence_ranges"), lambda: eng.silence_run(sl, 103, 1000, 1, 1))):
        for _ in range(3):
            run()
        eng.profile_enable(True); eng.profile_reset()
        for _ in range(runs):
            run()
        eng.sync()
        prof = eng.profile()
        eng.profile_enable(False)
        for name in names:
            per_run[name] = prof[name]["total_ms"] / runs
    n_ranges = int(eng.silence_fetch()["range_offsets"][-1])
    print(f"{label} ({nbytes / 1e6:.0f} MB, {n_ms} ms bins, {n_ranges} silent ranges)")
    for name, ms in per_run.items():
        moved = {"k_energy": nbytes, "k_ms_energy": nbytes + 8 * n_ms}.get(name)
        tail = f"  {moved / ms / 1e6:7.0f} GB/s = {moved / ms / 1e6 / 80:4.1f} % of 8 TB/s" if moved else ""
        print(f"  {name:18s} {ms * 1e3:8.1f} us per run{tail}")
    total = sum(v for k, v in per_run.items() if k != "k_energy")
    print(f"  k_ms_energy / k_energy = {per_run['k_ms_energy'] / per_run['k_energy']:.2f}   all silence kernels / k_energy = {total / per_run['k_energy']:.2f}")
eng.close()
