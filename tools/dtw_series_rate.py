#!/usr/bin/env python3
"""Rates of ``pce_dtw_series`` on the device (profiles/r08/dtw_series.txt).

For 1 and 10 pairs of random-walk series of 8 192, 32 768 and 65 536 points: the exact programme and fastdtw(radius = 25), one warm-up
call and ``--reps`` timed ones.  Two clocks per case: the host clock around the call (it ends in a device synchronise: upload, launches,
walk back, download, and for fastdtw the host's halving / window building) and the device time of the two kernels from the engine's own
HIP-event brackets (``pce_profile_get``; cells = ``pce_profile_get_work``).  Then the one yardstick the parent commit offers: its
``pce_dtw`` on the dense |a_i - b_j| matrix of a 1 024 x 16 384 pair, batch 8, against ``dtw_series`` on the same series (another
recurrence -- float32 accumulator, diagonal first -- so the paths are not compared, only the time per cell), and the DTW stage of
``evaluate_all`` for ten episodes of 30 000 voiced frames.

    python tools/dtw_series_rate.py [--reps 10] [--out profiles/r08/dtw_series.txt] [--max 65536]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import prosody_control_french_tts_amd as P                                          # noqa: E402
from prosody_control_french_tts_amd.Pipeline import evaluate_voice as EV            # noqa: E402


def walk(rng, n):
    return 5.0 + np.cumsum(rng.normal(0.0, 0.01, n))


def timed(eng, fn, reps):
    fn()                                                                            # warm-up: code objects, buffer growth
    wall, sweep, trace, cells = [], [], [], 0.0
    for _ in range(reps):
        eng.profile_reset()
        t0 = time.perf_counter(); fn(); wall.append((time.perf_counter() - t0) * 1e3)
        pr = eng.profile()
        sweep.append(pr.get("k_dtw_series", {}).get("total_ms", 0.0)); trace.append(pr.get("k_dtw_series_trace", {}).get("total_ms", 0.0))
        cells = pr.get("k_dtw_series", {}).get("flops", 0.0)
    return np.array(wall), np.array(sweep), np.array(trace), cells


def line(name, wall, sweep, trace, cells):
    med = np.median
    rate = cells / (med(sweep) * 1e-3) / 1e9 if med(sweep) > 0 else float("nan")
    return (f"{name:<34} wall {med(wall):9.2f} ms (min {wall.min():.2f} max {wall.max():.2f})  sweep {med(sweep):9.2f} ms (min {sweep.min():.2f} max {sweep.max():.2f})"
            f"  walk back {med(trace):8.2f} ms  cells {cells:.3e}  {rate:8.1f} Gcell/s in the sweep, {cells / (med(wall) * 1e-3) / 1e9:8.1f} end to end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max", type=int, default=65536)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = []
    with P.ProsodyEngine(0) as eng:
        info = eng.device_info()
        out.append(f"# {info['name']}, {info['compute_units']} CUs; tile {P.engine.DTW_SERIES_ROWS} x {P.engine.DTW_SERIES_COLS}; {args.reps} timed calls after one warm-up, medians")
        eng.profile_enable(True)
        for n in (8192, 32768, 65536):
            if n > args.max:
                continue
            for batch in (1, 10):
                pairs = [(walk(rng, n), walk(rng, n)) for _ in range(batch)]
                out.append(line(f"exact      {batch:2d} x {n}^2", *timed(eng, lambda: eng.dtw_series(pairs), args.reps)))
                print(out[-1], flush=True)
                out.append(line(f"fastdtw r25 {batch:2d} x {n}^2", *timed(eng, lambda: EV.fastdtw_batch(pairs, 25, eng), args.reps)))
                print(out[-1], flush=True)
        # the parent's dense kernel on the same series
        n, m, batch = 1024, 16384, 8
        pairs = [(walk(rng, n), walk(rng, m)) for _ in range(batch)]
        dense = np.stack([np.abs(a[:, None] - b[None, :]) for a, b in pairs])
        eng.dtw(dense)
        td, kd = [], []
        for _ in range(args.reps):
            eng.profile_reset()
            t0 = time.perf_counter(); eng.dtw(dense); td.append((time.perf_counter() - t0) * 1e3)
            kd.append(eng.profile()["k_dtw"]["total_ms"])
        w, s, t, cells = timed(eng, lambda: eng.dtw_series(pairs), args.reps)
        out.append(f"dense pce_dtw   8 x 1024 x 16384      wall {np.median(td):9.2f} ms (min {min(td):.2f} max {max(td):.2f})  kernel {np.median(kd):9.2f} ms (sweep and walk back in one)")
        out.append(line("dtw_series      8 x 1024 x 16384", w, s, t, cells))
        out.append(f"ratio dense / series: wall {np.median(td) / np.median(w):.2f}, kernels {np.median(kd) / (np.median(s) + np.median(t)):.2f}")
        print("\n".join(out[-3:]), flush=True)
        # the DTW stage of evaluate_all: ten episodes of 30 000 voiced frames (F0 contours in Hz)
        cont = [(np.exp(walk(rng, 30000)), np.exp(walk(rng, 30000))) for _ in range(10)]
        for method in ("exact", "fastdtw"):
            EV.f0_contour_rmse_batch(cont, method=method, engine=eng)
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter(); EV.f0_contour_rmse_batch(cont, method=method, engine=eng); ts.append((time.perf_counter() - t0) * 1e3)
            out.append(f"evaluate_all DTW stage, 10 x 30000^2, {method:<8} wall {np.median(ts):9.2f} ms (min {min(ts):.2f} max {max(ts):.2f})")
            print(out[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
