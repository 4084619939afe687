#!/usr/bin/env python3
"""Does a change to the kernel sources change the device code?  Compiles the device side of every tps_amd/csrc/*.hip unit
to gfx950 assembly twice -- from a temporary copy of <git-rev> and from the working tree, with the flags of build() --
and compares the two symbol by symbol.

    python tools/device_asm_diff.py HEAD                      # every unit (two compiles each: many core-minutes)
    python tools/device_asm_diff.py HEAD~1 --units plasma_3d_n3a.hip,tpsrhs.hip --flags="-DTPSRHS_STAMP=1"

Per unit it prints the number of kernels and the names of the symbols that differ; the exit status is non-zero if any
does.  Only the lines that hold the per-translation-unit symbol __hip_cuid_<hash> are left out of the comparison.  Both
compiles run in their own tree's tps_amd/csrc and name the unit relatively, so that no path differs.

The assembly is read only to compare two builds with each other: a refactor that claims to be neutral shows it here
(DESIGN.md section 5).  Not a test: it needs no GPU, but minutes of every core."""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC, UNIT_FLAGS  # noqa: E402

REST = "<unit-level text>"  # what belongs to no symbol: section directives, the .type / .globl lines ahead of a label
NOTE = "<metadata note>"    # .amdgpu_metadata ... .end_amdgpu_metadata: what the runtime reads about every kernel
LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
DESCRIPTOR = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
SIZE = re.compile(r"^\s*\.size\s+([^,\s]+),")


def symbols(path):
    """{symbol: digest of its lines} and the set of kernel names of one assembly file.  A symbol's lines run from its
    label to its .size directive; a kernel also owns its descriptor block (.amdhsa_kernel ... .end_amdhsa_kernel).
    The unit-level text is compared as a SET of lines: the compiler does not emit the data objects of a unit in the same
    order from one run to the next of the same source (seen with -DTPSRHS_STAMP=2: g_stamp and the section directives
    around it move), so neither the order nor the repetition of those lines says anything about the source."""
    text, kernels, cur, rest = {}, set(), REST, set()
    with open(path, errors="replace") as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            if line.strip() == ".amdgpu_metadata":
                cur = NOTE
            m = DESCRIPTOR.match(line)
            if m:
                cur = m.group(1)
                kernels.add(cur)
            elif not line.startswith(".L") and cur != NOTE:  # (the metadata note is YAML: its keys are no labels)
                m = LABEL.match(line)
                if m:
                    cur = m.group(1)
            if cur == REST:
                rest.add(line)
            else:
                text.setdefault(cur, hashlib.sha256()).update(line.encode())
            m = SIZE.match(line)
            if (m and m.group(1) == cur) or line.strip() in (".end_amdhsa_kernel", ".end_amdgpu_metadata"):
                cur = REST
    text[REST] = hashlib.sha256("".join(sorted(rest)).encode())
    return {k: h.hexdigest() for k, h in text.items()}, kernels


def compile_unit(tree, unit, extra, out):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + list(UNIT_FLAGS.get(unit, [])) + extra + \
          ["--cuda-device-only", "-S", unit, "-o", out]
    p = subprocess.run(cmd, cwd=os.path.join(tree, "tps_amd", "csrc"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"{unit} in {tree}: hipcc failed\n{p.stdout[-2000:]}")
    try:
        return symbols(out)
    finally:
        os.remove(out)


def weight(unit):  # longest compiles first, as in build()
    if unit == "tpsrhs.hip":
        return 0
    for rank, tag in enumerate(("_n8", "_n7", "_n6", "_n5", "_n4", "_n3"), start=1):
        if tag in unit:
            return rank
    return 9


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", help="the commit to compare the working tree with")
    ap.add_argument("--units", default="", help="comma-separated unit names (default: every tps_amd/csrc/*.hip)")
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, joined on with '=': --flags=\"-DTPSRHS_STAMP=1\"")
    args = ap.parse_args()
    extra = shlex.split(args.flags)
    csrc = os.path.join(ROOT, "tps_amd", "csrc")
    units = [u.strip() for u in args.units.split(",") if u.strip()] or sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    units.sort(key=weight)
    rev = subprocess.run(["git", "rev-parse", "--short", args.rev], cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f"device assembly (gfx950) of the working tree against {rev}; extra flags: {args.flags or 'none'}", flush=True)
    bad = 0
    with tempfile.TemporaryDirectory(prefix="device_asm_diff_") as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        ar = subprocess.Popen(["git", "archive", "--format=tar", args.rev], cwd=ROOT, stdout=subprocess.PIPE)
        with tarfile.open(fileobj=ar.stdout, mode="r|") as t:
            t.extractall(old, **({"filter": "data"} if hasattr(tarfile, "data_filter") else {}))
        if ar.wait() != 0:
            raise SystemExit(f"git archive {args.rev} failed")
        for side in ("a", "b"):
            os.makedirs(os.path.join(tmp, side))
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = {u: (pool.submit(compile_unit, old, u, extra, os.path.join(tmp, "a", u[:-4] + ".s")),
                        pool.submit(compile_unit, ROOT, u, extra, os.path.join(tmp, "b", u[:-4] + ".s"))) for u in units}
            total = 0
            for u in units:
                (a, ka), (b, kb) = jobs[u][0].result(), jobs[u][1].result()
                diff = sorted(s for s in set(a) | set(b) if a.get(s) != b.get(s))
                kernels = ka | kb
                total += len(kernels)
                print(f"{u}: {len(kernels)} kernels, {len(diff)} symbols differ", flush=True)
                for s in diff:
                    print(f"    {'kernel' if s in kernels else 'other '} {s}")
                bad += len(diff)
    print(f"{len(units)} units, {total} kernels, {bad} differing symbols: {'IDENTICAL' if bad == 0 else 'DIFFERENT'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
