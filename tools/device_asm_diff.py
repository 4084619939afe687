#!/usr/bin/env python3
"""Does a change to the kernel sources change the device code?  Compiles the device side of every tps_amd/csrc/*.hip unit
to gfx950 assembly twice -- from a temporary copy of <git-rev> and from the working tree, with the flags of build() --
and compares the two symbol by symbol.

    python tools/device_asm_diff.py HEAD                      # every unit (two compiles each: many core-minutes)
    python tools/device_asm_diff.py HEAD~1 --units plasma_3d_n3a.hip,tpsrhs.hip --flags="-DTPSRHS_STAMP=1"

    python tools/device_asm_diff.py HEAD~1 --by-kernel --rev-units tpsrhs.hip --units tpsrhs.hip,time_loop.hip

Per unit it prints the number of kernels and the names of the symbols that differ; the exit status is non-zero if any
does.  Only the lines that hold the per-translation-unit symbol __hip_cuid_<hash> are left out of the comparison.  Both
compiles run in their own tree's tps_amd/csrc and name the unit relatively, so that no path differs.

--by-kernel compares kernels wherever they sit: code that moves from one unit to another, or up and down within one.  The
symbols of all units of a side are pooled and paired by name, and the compiler's per-unit function ordinal in local labels
(normalize_ordinals) is replaced by a placeholder first; basic-block numbers and every instruction stay in the comparison.
A symbol that several units hold must be the same in all of them.  The exit status is non-zero if a symbol exists on one
side only or any two of its copies differ; the unit-level text and the metadata note, which list the kernels of a unit,
are reported and do not decide.

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
# local labels that carry the ordinal of their function within the unit: .LBB<n>_<m> (basic block m of function n),
# .LJTI<n>_<m> (jump table), .Lfunc_begin<n>, .Lfunc_end<n> -- and the loop comments that name a block, "Header=BB<n>_<m>"
ORDINAL = re.compile(r"\.L(BB|JTI|func_begin|func_end)\d+")
COMMENT_BLOCK = re.compile(r"\bBB\d+(?=_\d)")


# the compiler pads the comment behind a label to a fixed column, so its distance depends on the digits of the ordinal
LABEL_COMMENT = re.compile(r"^(\.L(?:BB|JTI|func_begin|func_end)#\w*:)[ \t]+;", re.M)


def normalize_ordinals(text):
    """the assembly text with the function ordinal of every local label replaced by '#': .LBB12_3 -> .LBB#_3, BB12_3 ->
    BB#_3 in a comment, and one blank between such a label and the comment on its line"""
    return LABEL_COMMENT.sub(r"\1 ;", COMMENT_BLOCK.sub("BB#", ORDINAL.sub(r".L\1#", text)))


def symbols(asm):
    """{symbol: digest of its lines} and the set of kernel names of one unit's assembly text.  A symbol's lines run from its
    label to its .size directive; a kernel also owns its descriptor block (.amdhsa_kernel ... .end_amdhsa_kernel).
    The unit-level text is compared as a SET of lines: the compiler does not emit the data objects of a unit in the same
    order from one run to the next of the same source (seen with -DTPSRHS_STAMP=2: g_stamp and the section directives
    around it move), so neither the order nor the repetition of those lines says anything about the source."""
    text, kernels, cur, rest = {}, set(), REST, set()
    for line in asm.splitlines(keepends=True):
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


def pool(units):
    """{unit: symbols(...)[0]} of one side -> {symbol: {digest: [units that hold this copy]}}, the per-unit entries left out"""
    out = {}
    for u, syms in units.items():
        for s, d in syms.items():
            if s not in (REST, NOTE):
                out.setdefault(s, {}).setdefault(d, []).append(u)
    return out


def compare_pools(a, b):
    """-> (symbols on one side only, symbols whose copies differ): what decides --by-kernel"""
    one_sided = sorted(set(a) ^ set(b))
    differ = sorted(s for s in set(a) | set(b) if len(set(a.get(s, {})) | set(b.get(s, {}))) > 1)
    return one_sided, differ


def compile_unit(tree, unit, extra, out, by_kernel=False):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + list(UNIT_FLAGS.get(unit, [])) + extra + \
          ["--cuda-device-only", "-S", unit, "-o", out]
    p = subprocess.run(cmd, cwd=os.path.join(tree, "tps_amd", "csrc"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"{unit} in {tree}: hipcc failed\n{p.stdout[-2000:]}")
    try:
        with open(out, errors="replace") as f:
            asm = f.read()
        return symbols(normalize_ordinals(asm) if by_kernel else asm)
    finally:
        os.remove(out)


def weight(unit):  # longest compiles first, as in build()
    if unit in ("tpsrhs.hip", "sampling.hip", "integrals.hip"):
        return 0
    for rank, tag in enumerate(("_n8", "_n7", "_n6", "_n5", "_n4", "_n3"), start=1):
        if tag in unit:
            return rank
    return 9


def report_by_kernel(old_units, new_units, a, b, ka, kb):
    """prints the pooled comparison; -> the number of symbols that decide the exit status"""
    pa, pb = pool(a), pool(b)
    one_sided, differ = compare_pools(pa, pb)
    kernels = ka | kb
    kind = lambda s: "kernel" if s in kernels else "other "  # noqa: E731
    held = lambda p, s: sum(len(us) for us in p.get(s, {}).values())  # noqa: E731
    print(f"rev: {len(old_units)} units, {len(pa)} symbols, {len(ka)} kernels; working tree: {len(new_units)} units, {len(pb)} symbols, {len(kb)} kernels")
    for s in one_sided:
        where = pa.get(s) or pb.get(s)
        print(f"    only in {'rev' if s in pa else 'the working tree'}: {kind(s)} {s} ({', '.join(sorted(u for us in where.values() for u in us))})")
    for s in differ:
        print(f"    copies differ: {kind(s)} {s}")
        for side, p in (("rev", pa), ("tree", pb)):
            for d, us in sorted(p.get(s, {}).items()):
                print(f"        {side} {d[:12]} {', '.join(sorted(us))}")
    print("units that hold each symbol (rev -> working tree), where either side has more than one:")
    for s in sorted(set(pa) | set(pb)):
        if held(pa, s) > 1 or held(pb, s) > 1:
            print(f"    {held(pa, s)} -> {held(pb, s)}  {kind(s)} {s}")
    n1 = sum(1 for s in set(pa) | set(pb) if held(pa, s) <= 1 and held(pb, s) <= 1)
    print(f"    1 -> 1 (or 0)  the other {n1} symbols")
    # the per-unit entries: they list the kernels of a unit, so they differ when a kernel moves -- reported, not decisive
    for name in (REST, NOTE):
        da, db = sorted({v[name] for v in a.values() if name in v}), sorted({v[name] for v in b.values() if name in v})
        print(f"{name}: {'same' if da == db else 'differs'} (does not decide)")
    return len(one_sided) + len(differ)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", help="the commit to compare the working tree with")
    ap.add_argument("--units", default="", help="comma-separated unit names (default: every tps_amd/csrc/*.hip)")
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, joined on with '=': --flags=\"-DTPSRHS_STAMP=1\"")
    ap.add_argument("--by-kernel", action="store_true", help="pool the symbols of all units of a side and pair them by name")
    ap.add_argument("--rev-units", default="", help="--by-kernel: the units of the commit (default: those of --units)")
    ap.add_argument("--tree", default=ROOT, help="the tree compared with the commit (default: the one this tool sits in)")
    args = ap.parse_args()
    extra = shlex.split(args.flags)
    tree = os.path.abspath(args.tree)
    csrc = os.path.join(tree, "tps_amd", "csrc")
    units = [u.strip() for u in args.units.split(",") if u.strip()] or sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    units.sort(key=weight)
    old_units = sorted([u.strip() for u in args.rev_units.split(",") if u.strip()], key=weight) or units
    if old_units != units and not args.by_kernel:
        raise SystemExit("--rev-units needs --by-kernel: the default mode compares unit with unit")
    rev = subprocess.run(["git", "rev-parse", "--short", args.rev], cwd=ROOT, check=True, stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f"device assembly (gfx950) of {'the working tree' if tree == ROOT else tree} against {rev}; extra flags: {args.flags or 'none'}"
          f"{'; by kernel' if args.by_kernel else ''}", flush=True)
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
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool_:
            ja = {u: pool_.submit(compile_unit, old, u, extra, os.path.join(tmp, "a", u[:-4] + ".s"), args.by_kernel) for u in old_units}
            jb = {u: pool_.submit(compile_unit, tree, u, extra, os.path.join(tmp, "b", u[:-4] + ".s"), args.by_kernel) for u in units}
            total = 0
            if args.by_kernel:
                a, b = {u: j.result() for u, j in ja.items()}, {u: j.result() for u, j in jb.items()}
                ka, kb = set().union(*(k for _, k in a.values())), set().union(*(k for _, k in b.values()))
                total = len(ka | kb)
                bad = report_by_kernel(old_units, units, {u: v[0] for u, v in a.items()}, {u: v[0] for u, v in b.items()}, ka, kb)
            else:
                for u in units:
                    (a, ka), (b, kb) = ja[u].result(), jb[u].result()
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
