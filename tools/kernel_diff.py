#!/usr/bin/env python3
"""Compare the GPU kernels of two source trees without a GPU.

    python tools/kernel_diff.py <tree A> <tree B> [--jobs N] [--keep DIR] [--show N]

Every .hip unit of each tree's dlsa_amd/build.py SOURCES is compiled to a plain
device ELF (the flags of build._common_flags() plus --cuda-device-only
--no-gpu-bundle-output -c; a bundled object does not disassemble).  For every
kernel symbol, across all units of a tree, two things are collected:

  * the instructions (llvm-objdump -d) without addresses and encodings; branch
    operands are relative, so the text does not depend on where a kernel lies;
  * the kernel's resources from the ELF's metadata note (llvm-readelf --notes).

Reported: kernels present on one side only, and kernels whose instructions or
resources differ.  Exit status 1 if there is any, else 0.  Nothing is launched
and no instruction is looked for: the two sides are only compared.

--keep DIR keeps the ELFs under DIR/a and DIR/b and reuses one that is newer
than every file of its tree's csrc/ and include/ (a second run after editing
one side recompiles that side only).
"""

from __future__ import annotations

import argparse
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "wavefront_size",
        "kernarg_segment_size", "max_flat_workgroup_size")


def load_build(tree):
    path = os.path.join(tree, "dlsa_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(cmd):
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError(f"{cmd[0]} failed ({res.returncode}): {' '.join(cmd)}")
    return res.stdout


def newest(tree):
    t = 0.0
    for d in (os.path.join(tree, "dlsa_amd", "csrc"), os.path.join(tree, "include")):
        for root, _, files in os.walk(d):
            t = max([t] + [os.path.getmtime(os.path.join(root, f)) for f in files])
    return t


def compile_tree(tree, out_dir, jobs):
    """{unit: device ELF path} of the tree's .hip units."""
    b = load_build(tree)
    os.makedirs(out_dir, exist_ok=True)
    units = [s for s in b.SOURCES if s.endswith(".hip")]
    stamp = newest(tree)

    def one(src):
        elf = os.path.join(out_dir, os.path.splitext(src)[0] + ".elf")
        if not (os.path.exists(elf) and os.path.getmtime(elf) > stamp):
            run([b.hipcc()] + b._common_flags() +
                ["--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(b.CSRC, src),
                 "-o", elf])
        return src, elf

    with ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        return b, dict(ex.map(one, units))


def llvm_tool(b, name):
    """The LLVM tool beside the tree's hipcc (<rocm>/bin/hipcc, <rocm>/llvm/bin/<name>)."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc())))
    return os.path.join(rocm, "llvm", "bin", name)


def kernel_meta(readelf, elf):
    """{kernel symbol: {field: value}} from the AMDGPU metadata note."""
    out, cur = {}, None
    for line in run([readelf, "--notes", elf]).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)  # a kernel's own fields only
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "name":
            out[m.group(3)] = cur
    return {k: {f: v.get(f) for f in META} for k, v in out.items()}


def kernel_text(objdump, elf, names):
    """{kernel symbol: [instruction lines]}."""
    out, cur = {}, None
    for line in run([objdump, "-d", elf]).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
            continue
        if cur is None:
            continue
        ins = " ".join(line.split("//")[0].split())
        if ins:
            cur.append(ins)
    return out


def collect(tree, out_dir, jobs):
    """{kernel symbol: [(unit, meta, text), ...]} of one tree."""
    b, elfs = compile_tree(tree, out_dir, jobs)
    objdump, readelf = (llvm_tool(b, t) for t in ("llvm-objdump", "llvm-readelf"))

    def one(item):
        unit, elf = item
        meta = kernel_meta(readelf, elf)
        text = kernel_text(objdump, elf, set(meta))
        return [(k, unit, meta[k], text.get(k, [])) for k in meta]

    kernels = {}
    with ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        for rows in ex.map(one, sorted(elfs.items())):
            for k, unit, meta, text in rows:
                kernels.setdefault(k, []).append((unit, meta, text))
    for v in kernels.values():  # a symbol of several units: compared in a fixed order
        v.sort(key=lambda e: (e[2], sorted(e[1].items(), key=str)))
    return len(elfs), kernels


def demangle(cxxfilt, name):
    if not cxxfilt:
        return name
    return subprocess.run([cxxfilt, name], capture_output=True, text=True).stdout.strip() or name


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", metavar="DIR", help="keep (and reuse) the device ELFs under DIR")
    ap.add_argument("--show", type=int, default=20, help="diff lines printed per differing kernel")
    a = ap.parse_args(argv)

    with tempfile.TemporaryDirectory(prefix="kernel_diff_") as tmp:
        base = a.keep or tmp
        na, A = collect(os.path.abspath(a.tree_a), os.path.join(base, "a"), a.jobs)
        nb, B = collect(os.path.abspath(a.tree_b), os.path.join(base, "b"), a.jobs)

    cxxfilt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    only_a, only_b = sorted(set(A) - set(B)), sorted(set(B) - set(A))
    for side, names in (("A", only_a), ("B", only_b)):
        for k in names:
            units = (A if side == "A" else B)[k]
            print(f"only in {side}: {demangle(cxxfilt, k)}  [{', '.join(u for u, _, _ in units)}]")
    differing = 0
    for k in sorted(set(A) & set(B)):
        ea, eb = A[k], B[k]
        same = len(ea) == len(eb) and all(x[1] == y[1] and x[2] == y[2] for x, y in zip(ea, eb))
        if same:
            continue
        differing += 1
        print(f"differs: {demangle(cxxfilt, k)}  [{ea[0][0]} | {eb[0][0]}]")
        if len(ea) != len(eb):
            print(f"  defined in {len(ea)} unit(s) of A, {len(eb)} of B")
            continue
        for (_, ma, ta), (_, mb, tb) in zip(ea, eb):
            for f in META:
                if ma[f] != mb[f]:
                    print(f"  {f}: {ma[f]} -> {mb[f]}")
            if ta != tb:
                d = list(difflib.unified_diff(ta, tb, "A", "B", lineterm="", n=1))
                print(f"  instructions: {len(ta)} -> {len(tb)}")
                for line in d[:a.show]:
                    print("    " + line)
    compared = len(set(A) & set(B))
    print(f"units: {na} | {nb}; kernels: {len(A)} | {len(B)}; compared: {compared}; "
          f"only in A: {len(only_a)}; only in B: {len(only_b)}; differing: {differing}")
    return 1 if (only_a or only_b or differing) else 0


if __name__ == "__main__":
    sys.exit(main())
