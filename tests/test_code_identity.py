"""tools/code_identity.py on the CPU: one small kernel cross-compiled for gfx950 three times -- as it is, with a host-only edit and shifted lines,
and with one constant changed inside the kernel.  The tool must call the first pair identical and name the kernel for the second.
--pair-demangled: a kernel whose argument struct moves out of an anonymous namespace pairs with itself (and an edit is still named); a pairing
key that two kernels share is an error."""
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


def _tool(*args):
    return subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, timeout=120)


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


STRUCT_SOURCE = """#include <hip/hip_runtime.h>
%(open)s
struct ScaleArgs { float factor; float offset; int n; };
%(close)s
__global__ void k_struct_probe(ScaleArgs a, const float *__restrict__ x, float *__restrict__ y)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n) y[i] = x[i] * a.factor + %(offset)s;
}
%(extra)s
int host_side(float *x, float *y, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_struct_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ScaleArgs{3.0f, 1.0f, n}, x, y);
    return (int)hipGetLastError();
}
"""
# two kernels that differ by an anonymous namespace alone: both demangle to one pairing key
TWINS = """namespace { __attribute__((used)) __global__ void k_twin(float *y) { y[threadIdx.x] = 1.0f; } }
__attribute__((used)) __global__ void k_twin(float *y) { y[threadIdx.x] = 2.0f; }
"""


def _build_struct(tmp_path, name, **parts):
    src, obj = tmp_path / f"{name}.hip", tmp_path / f"{name}.o"
    src.write_text(STRUCT_SOURCE % parts)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-c", str(src), "-o", str(obj)], check=True, capture_output=True, text=True)
    return str(obj)


def test_struct_moved_out_of_an_anonymous_namespace_pairs_by_demangled_name(tmp_path):
    """A kernel that takes a struct by value, with the struct inside and outside an anonymous namespace: the mangled names differ, so the plain
    run reports each kernel as present on one side only; --pair-demangled pairs them and finds the same code, and still names a kernel edit."""
    inside = _build_struct(tmp_path, "inside", open="namespace {", close="}", offset="a.offset", extra="")
    outside = _build_struct(tmp_path, "outside", open="", close="", offset="a.offset", extra="")
    edited = _build_struct(tmp_path, "edited", open="", close="", offset="2.0f * a.offset", extra="")
    plain = _tool(inside, outside)
    assert plain.returncode == 1, plain.stdout + plain.stderr
    only = [ln for ln in plain.stdout.splitlines() if "k_struct_probe" in ln and " only in " in ln]
    assert len(only) == 2 and plain.stdout.strip().splitlines()[-1].startswith("0 kernels, "), plain.stdout
    paired = _tool("--pair-demangled", inside, outside)
    assert paired.returncode == 0, paired.stdout + paired.stderr
    assert paired.stdout.strip().splitlines()[-1] == "1 kernels, 0 differences"
    diff = _tool("--pair-demangled", inside, edited)
    assert diff.returncode == 1, diff.stdout + diff.stderr
    lines = diff.stdout.strip().splitlines()
    assert any("k_struct_probe" in ln and "text differs" in ln for ln in lines[:-1]), diff.stdout
    assert lines[-1].startswith("1 kernels, ") and not lines[-1].endswith(" 0 differences")


def test_pairing_key_that_is_not_unique_is_an_error(tmp_path):
    """Two kernels of one object that differ by an anonymous namespace alone cannot be paired by the demangled name: the option says so and
    exits with 2; without it the run compares as ever."""
    base = _build_struct(tmp_path, "base", open="", close="", offset="a.offset", extra="")
    twins = _build_struct(tmp_path, "twins", open="", close="", offset="a.offset", extra=TWINS)
    r = _tool("--pair-demangled", base, twins)
    assert r.returncode == 2 and "both pair as" in r.stderr and "k_twin" in r.stderr, r.stdout + r.stderr
    assert _tool(twins, twins).returncode == 0
