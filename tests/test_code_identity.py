"""tools/code_identity.py on the CPU: one small kernel cross-compiled for gfx950 three times -- as it is, with a host-only edit and shifted lines,
and with one constant changed inside the kernel.  The tool must call the first pair identical and name the kernel for the second."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TOOL = os.path.join(ROOT, "tools", "code_identity.py")

SOURCE = """#include <hip/hip_runtime.h>
%(head)s
__global__ void k_scale_probe(const float *__restrict__ x, float *__restrict__ y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = x[i] * %(factor)s + 1.0f;
}
int host_side(float *x, float *y, int n, hipStream_t s)
{
    %(host)s
    hipLaunchKernelGGL(k_scale_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, y, n);
    return (int)hipGetLastError();
}
"""


def _build(tmp_path, name, **parts):
    src, obj = tmp_path / f"{name}.hip", tmp_path / f"{name}.o"
    src.write_text(SOURCE % parts)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-c", str(src), "-o", str(obj)], check=True, capture_output=True, text=True)
    return str(obj)


def _tool(a, b):
    return subprocess.run([sys.executable, TOOL, a, b], capture_output=True, text=True, timeout=120)


def test_host_edit_is_identical_and_kernel_edit_is_named(tmp_path):
    base = _build(tmp_path, "base", head="", factor="3.0f", host="")
    host = _build(tmp_path, "host", head="// a comment\n\n\nstatic int twice(int v) { return 2 * v; }", factor="3.0f",
                  host="if (twice(n) < 0) return -1;")
    kern = _build(tmp_path, "kern", head="", factor="5.0f", host="")
    same = _tool(base, host)
    assert same.returncode == 0, same.stdout + same.stderr
    assert same.stdout.strip().splitlines()[-1] == "1 kernels, 0 differences"
    diff = _tool(base, kern)
    assert diff.returncode == 1, diff.stdout + diff.stderr
    lines = diff.stdout.strip().splitlines()
    assert any("k_scale_probe" in ln and "text differs" in ln for ln in lines[:-1]), diff.stdout
    assert lines[-1].startswith("1 kernels, ") and not lines[-1].endswith(" 0 differences")
