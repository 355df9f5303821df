#!/usr/bin/env python3
"""Per kernel of csrc/*.hip: flat_* instructions, `s_waitcnt vmcnt(0)` inside loops, VGPRs and occupancy.

Each source is compiled for the device only with the Makefile's flags (no object file, no GPU needed) and the
assembly is read.  A flat access means the compiler has lost a pointer's address space; once one is pending it can
no longer count memory waits, and every wait for a load becomes vmcnt(0): a drain of all outstanding loads AND
stores.  A loop is the range between a label and a later branch back to it.  A report, not a test.

    python3 tools/isa_waits.py [--only SUBSTRING] [--all] [source.hip ...]  > profiles/rNN/isa_waits_<tag>.txt

--all lists every kernel; the default lists those with a flat access or a vmcnt(0) in a loop, and totals per file.
"""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "onset_fingerprinting_amd" / "csrc"


def makefile_flags():
    """CXXFLAGS of csrc/Makefile without what belongs to the host side or to object files."""
    text = (CSRC / "Makefile").read_text().replace("\\\n", " ")
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = [f.replace("$(ARCH)", arch) for f in flags if f != "-fPIC" and not f.startswith("-W")]
    return hipcc, flags


def assemble(src, hipcc, flags, outdir):
    out = Path(outdir) / (src.stem + ".s")
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", f"-I{REPO / 'include'}", f"-I{CSRC}", str(src), "-o", str(out)]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out.read_text().splitlines()


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    """`void (anonymous namespace)::k_x<1024, true>(float const*, ...)` -> `k_x<1024, true>`"""
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    depth = 0
    for i, c in enumerate(name):
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            return name[:i]
    return name


LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
WAIT0 = re.compile(r"^\s+s_waitcnt\b.*\bvmcnt\(0\)")
FLAT = re.compile(r"^\s+flat_\w+")


def kernels_of(lines):
    """-> [(name, body lines, info dict)] for every .amdhsa_kernel of the file."""
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    want, start = set(names), {}
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m and m.group(1) in want:
            start.setdefault(m.group(1), i)
    res = []
    for n in names:
        i0 = start[n]
        i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
        info = {}
        for l in lines[i1:i1 + 40]:
            m = re.match(r"^; (NumVgprs|NumAgprs|Occupancy|ScratchSize): (\d+)", l)
            if m:
                info.setdefault(m.group(1), int(m.group(2)))
        res.append((n, lines[i0:i1], info))
    return res


def count(body):
    at = {}
    in_loop = [False] * len(body)
    for i, l in enumerate(body):
        m = LABEL.match(l)
        if m:
            at[m.group(1)] = i
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and at.get(m.group(1), i + 1) <= i:
            for j in range(at[m.group(1)], i + 1):
                in_loop[j] = True
    flat = sum(1 for l in body if FLAT.match(l))
    w_loop = sum(1 for i, l in enumerate(body) if in_loop[i] and WAIT0.match(l))
    w_all = sum(1 for l in body if WAIT0.match(l))
    return flat, w_loop, w_all


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", help="default: every csrc/*.hip")
    ap.add_argument("--only", default="", help="list only kernels whose demangled name contains this")
    ap.add_argument("--all", action="store_true", help="list every kernel")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    srcs = [Path(s).resolve() for s in a.sources] or sorted(CSRC.glob("*.hip"))
    hipcc, flags = makefile_flags()
    print(f"# {Path(hipcc).name} {' '.join(flags)} --cuda-device-only -S")
    print("# flat: flat_* instructions; w0/loop: s_waitcnt with vmcnt(0) inside a loop; w0: anywhere")
    print(f"# {'flat':>4} {'w0/loop':>7} {'w0':>4} {'vgpr':>4} {'agpr':>4} {'occ':>3} {'scratch':>7}  kernel")
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as ex:
        texts = list(ex.map(lambda s: assemble(s, hipcc, flags, tmp), srcs))
    for src, lines in zip(srcs, texts):
        ks = kernels_of(lines)
        names = demangle([k[0] for k in ks])
        rows = []
        for n, body, info in ks:
            flat, wl, wa = count(body)
            rows.append((flat, wl, wa, info.get("NumVgprs", -1), info.get("NumAgprs", -1), info.get("Occupancy", -1),
                         info.get("ScratchSize", -1), short(names[n])))
        print(f"{src.name}: {len(rows)} kernels, {sum(r[0] for r in rows)} flat, "
              f"{sum(1 for r in rows if r[0])} kernels with flat accesses")
        for r in rows:
            if a.only and a.only not in r[7]:
                continue
            if a.all or a.only or r[0] or r[1]:
                print(f"  {r[0]:>4} {r[1]:>7} {r[2]:>4} {r[3]:>4} {r[4]:>4} {r[5]:>3} {r[6]:>7}  {r[7]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
