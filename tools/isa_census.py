"""Developer tool (no GPU): static instruction census of the kernels of one .hip file.
    python tools/isa_census.py crispy_amd/csrc/rn_kernels.hip [--kernel SUBSTR] [--regions 1256-1398,1408-1460] [--top N]
Cross-compiles the file to gfx950 assembly with the Makefile's CXXFLAGS (plus -gline-tables-only, which changes no
instruction) and counts, per kernel from its label to its last s_endpgm, the instructions by class:
    vector   v_* other than the matrix instructions          matrix   v_mfma_* / v_smfmac_*
    lds      ds_*                                            memory   global_* / buffer_* / flat_* / scratch_*
    scalar   s_*
With --regions the vector / lds / memory counts are also attributed to line ranges of the file itself (by the .loc
directive in force, i.e. the innermost inlined source line); --top lists the source lines with the most vector instructions.
It counts classes only: what an instruction costs is a question for the counters (tools/collect_profiles.sh)."""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("vector", "matrix", "lds", "memory", "scalar")


def makefile_flags(csrc: str) -> list[str]:
    """CXXFLAGS of crispy_amd/csrc/Makefile with $(ARCH) expanded."""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def classify(mn: str) -> str | None:
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "matrix"
    if mn.startswith("v_"):
        return "vector"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "memory"
    if mn.startswith("s_"):
        return "scalar"
    return None


def demangle(names: list[str]) -> dict[str, str]:
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def assemble(path: str, extra: list[str]) -> str:
    csrc = os.path.join(ROOT, "crispy_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + makefile_flags(csrc) + extra + ["-gline-tables-only", "--cuda-device-only", "-S", "-x", "hip", "-I", csrc,
                                                    os.path.abspath(path), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
    if r.returncode != 0:
        sys.exit(f"{' '.join(cmd)}\nfailed:\n{r.stderr}")
    return r.stdout


def census(asm: str, main_file: str):
    """-> {kernel symbol: {"classes": Counter, "mnemonics": Counter, "lines": {line of main_file: Counter by class}}}"""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    files: dict[int, str] = {}
    res = {}
    cur = None
    pending = None       # counts since the last s_endpgm: dropped if no further one follows (padding, literal pools)
    loc = (None, 0)
    base = os.path.basename(main_file)
    for raw in asm.split("\n"):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.file\s+(\d+)\s+(?:\"([^\"]*)\"\s+)?\"([^\"]*)\"", line)
        if m:
            files[int(m.group(1))] = m.group(3)
            continue
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (files.get(int(m.group(1)), ""), int(m.group(2)))
            continue
        m = re.match(r"([A-Za-z_.$][\w.$]*):$", line)
        if m:
            if m.group(1) in kernels:
                cur = res[m.group(1)] = {"classes": collections.Counter(), "mnemonics": collections.Counter(), "lines": {}}
                pending = []
            continue
        if cur is None or line.startswith("."):
            continue
        mn = line.split()[0]
        cls = classify(mn)
        if cls is None:
            continue
        src_line = loc[1] if os.path.basename(loc[0] or "") == base else 0
        pending.append((cls, mn, src_line))
        if mn == "s_endpgm":
            for c, n, sl in pending:
                cur["classes"][c] += 1
                cur["mnemonics"][n] += 1
                cur["lines"].setdefault(sl, collections.Counter())[c] += 1
            pending = []
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("--kernel", default=None, help="only kernels whose demangled name contains this")
    ap.add_argument("--regions", default=None, help="line ranges of the file, a-b,c-d,...")
    ap.add_argument("--top", type=int, default=0, help="list the N source lines with the most vector instructions")
    ap.add_argument("--mnemonics", type=int, default=0, help="list the N most frequent vector mnemonics")
    ap.add_argument("-D", action="append", default=[], help="extra -D definitions")
    a = ap.parse_args()
    res = census(assemble(a.file, ["-D" + d for d in a.D]), a.file)
    names = demangle(list(res))
    for sym, r in res.items():
        name = names[sym]
        if a.kernel and a.kernel not in name:
            continue
        print(f"{name}: " + "  ".join(f"{c} {r['classes'][c]}" for c in CLASSES))
        if a.regions:
            for rg in a.regions.split(","):
                lo, hi = (int(v) for v in rg.split("-"))
                tot = collections.Counter()
                for sl, cnt in r["lines"].items():
                    if lo <= sl <= hi:
                        tot.update(cnt)
                print(f"    lines {lo:5d}-{hi:<5d} " + "  ".join(f"{c} {tot[c]}" for c in CLASSES))
        if a.top:
            for sl, cnt in sorted(r["lines"].items(), key=lambda kv: -kv[1]["vector"])[:a.top]:
                print(f"    line {sl:5d}: vector {cnt['vector']}  lds {cnt['lds']}  memory {cnt['memory']}")
        if a.mnemonics:
            vm = [(n, c) for n, c in r["mnemonics"].most_common() if classify(n) == "vector"][:a.mnemonics]
            print("    " + "  ".join(f"{n} {c}" for n, c in vm))


if __name__ == "__main__":
    main()
