"""csrc/pce_weight_pack.h, the host half of the four model loaders, alone on the CPU: tests/host/weight_pack_main.cpp is compiled with
AddressSanitizer and UndefinedBehaviorSanitizer and run as a child process (nothing is loaded into this interpreter; the sanitizer runtimes
are linked into the program itself).  It packs blobs of float(index) held in exactly-sized heap allocations and checks the fused attention
block with and without a key bias at d = 128 (every element, the zero third of the bias, the offsets, how far the cursor moved) and the
4-float alignment of the vectors."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weight_pack_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "weight_pack"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "prosody-control-french-tts_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "weight_pack_main.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr}"
