"""Device-code identity of two builds: the gfx950 code objects of two shared libraries (or object files), kernel by kernel.

For a change that is meant to leave the device code alone (a host-side refactor), build the parent and the new tree with the same compiler and
flags and compare: the set of kernel names per code object, each kernel's AMDGPU metadata (register counts, LDS and scratch sizes, spills, kernarg
size, workgroup size) and the ``llvm-objdump -d`` text of every function with addresses and encodings stripped.  Equality only: nothing is searched for.

usage: python tools/code_identity.py [--pair-demangled] A B
    one line per difference, else "N kernels, 0 differences"; exit code 1 when anything differs

Kernels and functions are paired by their mangled names.  --pair-demangled pairs them by the demangled name (llvm-cxxfilt of the same LLVM
directory; an installation without one: c++filt, which implements the same Itanium rules) with every
"(anonymous namespace)::" removed instead: for a change that moves a kernel, or a type in its signature, into or out of an anonymous namespace,
which renames the symbol and nothing else.  Two symbols of one code object with the same such name are an error (exit code 2), not a guess.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_guard import LLVM_BIN, code_objects  # noqa: E402

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
             "sgpr_spill_count", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack")


def _metadata(notes: str) -> dict:
    """{kernel name: {key: value}} out of the amdhsa.kernels list that ``llvm-readelf --notes`` prints (one `  - ` item per kernel)."""
    out = {}
    start = notes.find("amdhsa.kernels:")
    if start < 0:
        return out
    for item in re.split(r"\n  - ", notes[start:])[1:]:
        item = item.split("\namdhsa.", 1)[0]
        top = dict(re.findall(r"^(?:    |)\.(\w+):\s*(.*)$", item, re.M))       # the item's own keys: its first line, or indented by four
        if "name" in top:
            out[top["name"].strip("'\"")] = {k: top.get(k, "") for k in META_KEYS}
    return out


def _functions(disasm: str) -> dict:
    """{symbol: [instruction text]} with addresses, encodings, the disassembler's comments and trailing fill stripped."""
    parts = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", disasm)
    out = {}
    for i in range(1, len(parts), 2):
        body = []
        for line in parts[i + 1].splitlines():
            line = line.split("//", 1)[0].strip()
            if line and not line.startswith("Disassembly of section"):
                body.append(re.sub(r"\s+", " ", line))
        # what follows the last symbol of the section is the section's fill, not the function's code (how much of it there is depends on the link)
        while body and body[-1] in ("s_nop 0", "s_code_end"):
            body.pop()
        out[parts[i]] = body
    return out


def describe(path: str):
    """-> [(metadata, functions)] per gfx950 code object of ``path``, in the order the file holds them."""
    out = []
    with tempfile.TemporaryDirectory() as td:
        for k, img in enumerate(code_objects(path)):
            elf = os.path.join(td, f"co{k}.elf")
            with open(elf, "wb") as f:
                f.write(img)
            run = lambda tool, *a: subprocess.run([os.path.join(LLVM_BIN, tool), *a, elf], capture_output=True, text=True, check=True).stdout
            out.append((_metadata(run("llvm-readelf", "--notes")), _functions(run("llvm-objdump", "-d"))))
    return out


def _die(message: str):
    print(message, file=sys.stderr)
    sys.exit(2)


def _demangled_keys(names, where: str) -> dict:
    """{mangled: demangled with "(anonymous namespace)::" removed}; exit code 2 when two of ``names`` share a key."""
    names = sorted(names)
    if not names:
        return {}
    filt = os.path.join(LLVM_BIN, "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = shutil.which("c++filt")
    if not filt:
        _die(f"--pair-demangled: neither {os.path.join(LLVM_BIN, 'llvm-cxxfilt')} nor c++filt is installed")
    out = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    if len(out) != len(names):
        _die(f"{where}: llvm-cxxfilt answered {len(out)} lines for {len(names)} names")
    keys, seen = {}, {}
    for name, dem in zip(names, out):
        key = dem.replace("(anonymous namespace)::", "")
        if key in seen:
            _die(f"{where}: {seen[key]} and {name} both pair as {key}")
        seen[key] = name
        keys[name] = key
    return keys


def _rekey(objects, path: str):
    """describe()'s result with every kernel and function under its pairing key."""
    out = []
    for k, (meta, funcs) in enumerate(objects):
        keys = _demangled_keys(set(meta) | set(funcs), f"{path}, object {k}")
        out.append(({keys[n]: v for n, v in meta.items()}, {keys[n]: v for n, v in funcs.items()}))
    return out


def compare(path_a: str, path_b: str, pair_demangled: bool = False):
    """-> (kernels compared, [difference lines])."""
    a, b = describe(path_a), describe(path_b)
    if pair_demangled:
        a, b = _rekey(a, path_a), _rekey(b, path_b)
    diffs, n = [], 0
    if len(a) != len(b):
        diffs.append(f"code objects: {len(a)} against {len(b)}")
    for k, ((ma, fa), (mb, fb)) in enumerate(zip(a, b)):
        for name in sorted(set(ma) | set(mb)):
            if name not in mb or name not in ma:
                diffs.append(f"object {k}: kernel {name} only in {path_a if name in ma else path_b}")
                continue
            n += 1
            for key in META_KEYS:
                if ma[name][key] != mb[name][key]:
                    diffs.append(f"object {k}: kernel {name}: {key} {ma[name][key]} -> {mb[name][key]}")
        for name in sorted(set(fa) & set(fb)):
            if fa[name] != fb[name]:
                at = next((i for i, (x, y) in enumerate(zip(fa[name], fb[name])) if x != y), min(len(fa[name]), len(fb[name])))
                was = fa[name][at] if at < len(fa[name]) else "(end)"
                now = fb[name][at] if at < len(fb[name]) else "(end)"
                diffs.append(f"object {k}: {name}: text differs, {len(fa[name])} -> {len(fb[name])} instructions, first at {at}: {was} | {now}")
        for name in sorted((set(fa) ^ set(fb)) - set(ma) - set(mb)):
            diffs.append(f"object {k}: function {name} only in {path_a if name in fa else path_b}")
    return n, diffs


def main(argv):
    pair_demangled = "--pair-demangled" in argv[1:]
    paths = [a for a in argv[1:] if a != "--pair-demangled"]
    if len(paths) != 2:
        print(__doc__)
        return 2
    n, diffs = compare(paths[0], paths[1], pair_demangled)
    for d in diffs:
        print(d)
    print(f"{n} kernels, {len(diffs)} differences")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
