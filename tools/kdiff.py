#!/usr/bin/env python3
"""Compare the gfx950 kernels of two source trees, instruction for instruction (cross-compiles; no GPU needed).

usage: tools/kdiff.py TREE_A TREE_B

Each tree's HIP sources and flags are taken from its own amplisolve_amd/build.py (HIP_SOURCES, HIPCC_FLAGS) and compiled with
--save-temps into a temporary directory.  Kernels are paired by mangled name, whichever translation unit they live in.  A kernel's
text runs from its entry label to .end_amdhsa_kernel (the resource block included), with comments stripped and the digits of the
compiler's running labels (BB<n>_, func_end<n>, tmp<n>, JTI<n>) dropped: those count through a translation unit and change when
code moves.  One line per kernel; the exit status is 1 when a kernel differs or exists on one side only.
"""
from __future__ import annotations

import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LABEL = re.compile(r"(BB|func_end|func_begin|tmp|JTI)\d+")
RESOURCES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"),
             ("lds", "group_segment_fixed_size"))


def tree_build(tree: str):
    spec = importlib.util.spec_from_file_location("kdiff_build_" + str(abs(hash(tree))), os.path.join(tree, "amplisolve_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree: str, out: str) -> dict[str, tuple[str, dict[str, str], str]]:
    """mangled name -> (normalised text, resources, source file) of every kernel of the tree"""
    b = tree_build(tree)
    flags = [f for f in b.HIPCC_FLAGS if f != "-shared"]

    def one(src: str) -> str:
        d = os.path.join(out, src)
        os.makedirs(d)
        r = subprocess.run([b.hipcc_path(), *flags, "-c", "--save-temps", "-o", "k.o", os.path.join(b.CSRC, src)], cwd=d, capture_output=True,
                           text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{tree}: {src} does not compile\n{r.stderr}")
        return open(glob.glob(os.path.join(d, "*gfx950.s"))[0]).read()

    kernels = {}
    with ThreadPoolExecutor(max_workers=min(len(b.HIP_SOURCES), 16)) as pool:
        for src, asm in zip(b.HIP_SOURCES, pool.map(one, b.HIP_SOURCES)):
            for name in re.findall(r"^\s*\.amdhsa_kernel (\w+)", asm, re.M):
                body = re.search(r"^" + name + r":\s*; @" + name + r"\n(.*?\.end_amdhsa_kernel)", asm, re.S | re.M).group(1)
                lines = (re.sub(r"\s*;.*$", "", x).rstrip() for x in LABEL.sub(r"\1", body).split("\n"))
                text = "\n".join(x for x in lines if x)
                res = {k: re.search(r"\.amdhsa_" + key + r"\s+(\S+)", text).group(1) for k, key in RESOURCES}
                kernels[name] = (text, res, src)
    return kernels


def main() -> int:
    if len(sys.argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    with tempfile.TemporaryDirectory(prefix="kdiff.") as tmp:
        a = compile_tree(os.path.abspath(sys.argv[1]), os.path.join(tmp, "a"))
        b = compile_tree(os.path.abspath(sys.argv[2]), os.path.join(tmp, "b"))
    show = lambda r: " ".join(f"{k} {v}" for k, v in r.items())
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            bad += 1
            print(f"MISSING in {'A' if name not in a else 'B'}  {name}")
            continue
        same = a[name][0] == b[name][0]
        bad += 0 if same else 1
        where = a[name][2] if a[name][2] == b[name][2] else f"{a[name][2]} -> {b[name][2]}"
        print(f"{'identical' if same else 'DIFFERS  '}  {name}  [{where}]  A: {show(a[name][1])} | B: {show(b[name][1])}")
    print(f"{len(a)} kernels in A, {len(b)} in B, {len(set(a) & set(b))} paired, {bad} differing or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
