"""csrc/pce_pitch_plan.h, the host plan of the Praat pitch path, alone on the CPU: tests/host/pitch_plan_main.cpp is compiled with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into this interpreter; the sanitizer runtimes
are linked into the program itself).  Run without arguments it checks which k_pitch_frames instantiation every (rate, floor) pair of the
table in its source runs, the two refusals, the LDS / table-layout / staged-sample invariants over a sweep of rates and floors, the tables,
the work list and the buffer sizes, on exactly-sized vectors.  Run as ``plan ...`` it prints pitch_plan_make's fields, which the second test
compares bit for bit with the oracle's restatement (por_pitch_plan_make)."""
import os
import subprocess

import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (rate, floor) at ceiling 600: the pairs whose instantiation the program checks
PAIRS = [(16000, 150.0), (16000, 75.0), (22050, 150.0), (44100, 150.0), (22050, 75.0), (8000, 150.0), (44100, 75.0), (48000, 50.0)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pitch_plan") / "pitch_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "pitch_plan_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def test_pitch_plan_under_asan_and_ubsan(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr}"


def _plan(program, nx, rate, x1, floor, ceiling):
    r = subprocess.run([program, "plan", str(nx), str(rate), float(x1).hex(), float(floor).hex(), float(ceiling).hex()],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr}"
    return dict(ln.split() for ln in r.stdout.splitlines())


def _same_as_oracle(got, nx, rate, x1, floor, ceiling):
    want = O.pitch_plan(nx, 1.0 / rate, x1, O.praat_params(floor, ceiling))
    assert got["status"] == "0"
    for name in ("dt", "t1", "ceiling", "dt_window"):
        assert float.fromhex(got[name]).hex() == float(getattr(want, name)).hex(), name
    for name in ("n_frames", "nsamp_period", "halfnsamp_period", "nsamp_window", "halfnsamp_window", "maximum_lag", "brent_ixmax",
                 "max_candidates", "nsamp_fft"):
        assert int(got[name]) == getattr(want, name), name


@pytest.mark.parametrize("rate,floor", PAIRS)
def test_pitch_plan_make_equals_the_oracle_bit_for_bit(program, rate, floor):
    """One second and an odd length, from sample 0 and from a cut inside a recording."""
    for nx, x1 in ((rate, 0.5 / rate), (2 * rate - 7, 12345.5 / rate)):
        _same_as_oracle(_plan(program, nx, rate, x1, floor, 600.0), nx, rate, x1, floor, 600.0)


@pytest.mark.parametrize("rate,floor", PAIRS)
def test_too_short_boundary_equals_the_oracle(program, rate, floor):
    """The shortest slice Praat analyses (three periods of the floor) and the one a sample shorter, which it refuses: the same two lengths here."""
    x1 = 0.5 / rate
    params = O.praat_params(floor, 600.0)

    def analysable(nx):
        try:
            O.pitch_plan(nx, 1.0 / rate, x1, params)
            return True
        except O.PraatError:
            return False

    nx = int(3.0 / floor * rate) - 2
    while not analysable(nx):
        nx += 1
    assert nx <= int(3.0 / floor * rate) + 2 and not analysable(nx - 1)
    got = _plan(program, nx, rate, x1, floor, 600.0)
    _same_as_oracle(got, nx, rate, x1, floor, 600.0)
    assert got["n_frames"] == "1"
    assert _plan(program, nx - 1, rate, x1, floor, 600.0) == {"status": "1"}
