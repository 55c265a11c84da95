"""csrc/pce_sweep_plan.h, the launch plan of pce_ctc_align and pce_wx_align, alone on the CPU: tests/host/sweep_plan_main.cpp is compiled with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into this interpreter; the sanitizer runtimes
are linked into the program itself).  It checks the thread-count class at every boundary of the ladder, the grouping of clips under a budget
(an exact fit, one word over, clips that are not run at the start, middle and end of a group, a clip that alone exceeds the budget, nothing
run) and the id lists and launches of three groups with mixed kinds, on exactly-sized vectors."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_plan_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "sweep_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "sweep_plan_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr}"
