"""Developer tool (no GPU): is the device code of two trees the same, kernel by kernel?
    python tools/isa_same.py HEAD~1 . --a crispy_amd/csrc/whisper_kernels.hip \\
        --b crispy_amd/csrc/whisper_gemm.hip crispy_amd/csrc/whisper_attn.hip crispy_amd/csrc/whisper_pick.hip
A side is a git revision (its crispy_amd/csrc and include/ are checked out into a temporary directory) or a directory that
holds such a tree ("." = the working tree); --a / --b list the .hip files of each side (--b defaults to --a).  Every file
is cross-compiled to gfx950 assembly with the CXXFLAGS of its own side's Makefile, followed on both sides by what --flags
gives (one string, e.g. --flags "-DRN_PROFILE -DCRISPY_DEV_KNOBS", for the builds the Makefile makes with other defines); the kernels of a side's files are pooled
and compared by mangled name:
  * the instruction stream from the kernel's label to its end, without comments and .loc / .file / .cfi lines, with the
    local labels (.LBB<function>_<n>, .Ltmp<n>, .Lfunc_begin / .Lfunc_end<n>) renumbered per kernel;
  * the kernel descriptor (.amdhsa_next_free_vgpr / _sgpr, group and private segment sizes, and the rest of the block).
It prints a verdict per kernel with the first differing line, the kernels only one side has, and a summary; the exit
status is 0 when both sides hold the same kernels with the same code.  It compares two listings with each other, nothing
else: what the instructions are is isa_census.py's subject."""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOWN = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def materialise(side: str, tmp: str) -> str:
    """-> root directory of the side's tree"""
    if os.path.isdir(side):
        return os.path.abspath(side)
    dst = os.path.join(tmp, re.sub(r"\W", "_", side))
    os.makedirs(dst)
    ar = subprocess.run(["git", "-C", ROOT, "archive", side, "crispy_amd/csrc", "include"], capture_output=True)
    if ar.returncode != 0:
        sys.exit(f"{side}: neither a directory nor a revision: {ar.stderr.decode().strip()}")
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)
    return dst


def assemble(root: str, rel: str, extra: list[str]) -> str:
    csrc = os.path.join(root, "crispy_amd", "csrc")
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, *extra, "--cuda-device-only", "-S", "-x", "hip",
           os.path.join(root, rel), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\nfailed:\n{r.stderr}")
    return r.stdout


def kernels(asm: str) -> dict[str, tuple[list[str], list[str]]]:
    """-> {mangled name: (instruction stream, descriptor lines)}"""
    lines = [l.split(";", 1)[0].rstrip() for l in asm.split("\n")]
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out: dict[str, list[list[str]]] = {n: [[], []] for n in names}
    cur, desc = None, None
    for l in lines:
        s = l.strip()
        if not s:
            continue
        if s.endswith(":") and s[:-1] in names:
            cur = s[:-1]
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            desc = m.group(1)
            continue
        if s == ".end_amdhsa_kernel":
            desc = None
            continue
        if desc:
            out[desc][1].append(s)
        elif cur:
            if re.match(r"\.Lfunc_end\d+:", s):
                cur = None
            elif not s.startswith((".loc", ".file", ".cfi_")):
                out[cur][0].append(s)
    res = {}
    for n, (body, d) in out.items():
        seen: dict[str, str] = {}

        def local(m):
            key = re.sub(r"^\.LBB\d+_", ".LBB_", m.group(0))
            if key.startswith(".LBB_"):
                return key
            return seen.setdefault(key, re.sub(r"\d+$", "", key) + str(len(seen)))

        res[n] = ([re.sub(r"\.(?:LBB\d+_\d+|Ltmp\d+|Lfunc_(?:begin|end)\d+)", local, l) for l in body], d)
    return res


def pooled(root: str, files: list[str], extra: list[str]) -> dict:
    pool = {}
    for f in files:
        ks = kernels(assemble(root, f, extra))
        dup = set(ks) & set(pool)
        if dup:
            sys.exit(f"{f}: kernels already seen in another file of the same side: {sorted(dup)[:3]}")
        print(f"  {f}: {len(ks)} kernels", file=sys.stderr)
        pool.update(ks)
    return pool


def first_difference(a: list[str], b: list[str]) -> str:
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {i + 1}: {x!r} | {y!r}"
    return f"length {len(a)} | {len(b)}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("side_a", help="git revision or directory")
    ap.add_argument("side_b", help="git revision or directory")
    ap.add_argument("--a", nargs="+", required=True, metavar="FILE", help=".hip files of side A, relative to the tree's root")
    ap.add_argument("--b", nargs="+", default=None, metavar="FILE", help=".hip files of side B (default: those of A)")
    ap.add_argument("-q", "--quiet", action="store_true", help="only kernels that differ, and the summary")
    ap.add_argument("--flags", default="", metavar="FLAGS", help="extra compiler flags appended on both sides, one string")
    # `--flags -DX=1`: argparse would take a lone value that begins with '-' for an option, so the pair is joined first
    argv = sys.argv[1:]
    for i in range(len(argv) - 1):
        if argv[i] == "--flags":
            argv[i:i + 2] = ["--flags=" + argv[i + 1]]
            break
    a = ap.parse_args(argv)
    extra = a.flags.split()
    with tempfile.TemporaryDirectory() as tmp:
        print(f"A = {a.side_a}", file=sys.stderr)
        ka = pooled(materialise(a.side_a, tmp), a.a, extra)
        print(f"B = {a.side_b}", file=sys.stderr)
        kb = pooled(materialise(a.side_b, tmp), a.b or a.a, extra)
    same = 0
    for n in sorted(set(ka) & set(kb)):
        (ia, da), (ib, db) = ka[n], kb[n]
        if ia == ib and da == db:
            same += 1
            if not a.quiet:
                print(f"same  {n}  ({len(ia)} lines)")
            continue
        print(f"DIFF  {n}")
        if ia != ib:
            print(f"      instructions, {first_difference(ia, ib)}")
        if da != db:
            fig = lambda d: {k: v for k, v in (l.replace(".amdhsa_", "").split() for l in d if len(l.split()) == 2) if k in SHOWN}
            print(f"      descriptor, {first_difference(da, db)}; A {fig(da)} B {fig(db)}")
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for n in only_a:
        print(f"ONLY A  {n}")
    for n in only_b:
        print(f"ONLY B  {n}")
    print(f"{same} of {len(set(ka) | set(kb))} kernels identical; A has {len(ka)}, B has {len(kb)}; "
          f"only in A: {len(only_a)}, only in B: {len(only_b)}")
    sys.exit(0 if same == len(ka) == len(kb) else 1)


if __name__ == "__main__":
    main()
