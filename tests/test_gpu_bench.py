"""bench.py's plain line and --dump-outputs: two fresh processes with the same arguments time exactly --steps steps, print the headline
fields with the --full measurements left null, and write the same outputs of their last timed step, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs_repeat(tmp_path):
    common = ["--gpus", "1", "--clips", "16", "--steps", "3", "--warmup", "1"]
    lines, dumps = [], []
    for run in ("a", "b"):
        j = _bench(common + ["--dump-outputs", str(tmp_path / run), "--dump-records", str(tmp_path / f"{run}_records.npy")])
        lines.append(j)
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    j = lines[0]
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["higher_is_better"] is True
    assert abs(j["value"] - 16 * 10.0 * 3 / (j["ms_per_step"] * 3e-3)) <= 1e-6 * j["value"]
    assert j["step_ms_spread"]["n"] == 2                                  # three timed steps: two intervals after the first
    for key in ("metric", "unit", "dtype"):
        assert isinstance(j[key], str) and j[key]
    for key in ("cpu_baseline", "streamed_value", "transcribe", "medium", "framing_hbm"):
        assert j[key] is None, key                                        # measured under --full only
    a, b = dumps
    assert sorted(a) == sorted(b) and {"records", "lufs", "pitch_median_f0", "energy_sum_sq", "align_time_idx", "stft_db"} <= set(a)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), name
    assert a["records"].tobytes() == np.load(tmp_path / "a_records.npy").tobytes()
    assert a["records"].shape == (16, 7) and (a["records"][:, 0] > 0).sum() >= 8      # real measurements, not an empty table
    assert a["stft_db"].shape[0] == len(a["stft_db_clips"]) and a["align_path_len"].min() > 0
