"""Static VALU census of one kernel from `hipcc -S` output, whole and per phase:
    python tools/isa_phases.py <file.s> [mangled substring; default: the metric's k_gradient, Cfg<3,3,0> with the ambipolar
                                         single-temperature argon-minimal ternary mixture] [--top]
(tools/isa_mix.py counts the memory and FP64 opcodes of every p = 3 kernel of such a file, tools/kernel_isa.py reads a built
object; this one classifies the VALU instructions of ONE kernel -- FP64 arithmetic, integer / address, moves by source,
selects, compares, conversions -- and splits them at the phase stamps.)
The phases are the text between consecutive s_memtime stamps of a -DTPSRHS_STAMP=1 (k_gradient) or =2 (k_flux) build
(kernels.hpp STAMP / FSTAMP); an unstamped file is one segment.  Counts are of the code, not of executed
instructions: the face-direction loop of the 3-D kernels runs three times, and of its three per-direction copies of the
line stages one runs per trip."""
import collections
import re
import sys

F64 = re.compile(r"^v_(fma|fmac|mul|add)_f64")
INT = re.compile(r"^v_(add|sub|subrev|mul|mad|and|or|xor|not|lshl|lshr|ashr|bfe|bfi|lshlrev|lshrrev|ashrrev|mul_lo|mul_hi|mul_u32|"
                 r"add3|lshl_add|lshl_or|and_or|or3|xad|mad_u64|mad_i32|mad_u32|min|max|addc|subb|subbrev|add_lshl)[a-z0-9_]*_(u|i|b|co)")
CLASSES = ("valu", "f64", "int", "mov0", "mov1", "movlit", "movreg", "cndmask", "rcp", "cmp", "cvt", "lane", "other", "salu", "ds", "vmem")


def classify(op, rest):
    if not op.startswith("v_"):
        if op.startswith("s_"):
            return "salu"
        if op.startswith("ds_"):
            return "ds"
        if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            return "vmem"
        return None
    if F64.match(op):
        return "f64"
    if op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")):
        src = rest.split(",")[-1].strip()
        if re.match(r"^[vsa](\d|\[)", src) or src in ("vcc_lo", "vcc_hi", "exec_lo", "exec_hi", "m0"):
            return "movreg"
        if src in ("0",):
            return "mov0"
        if src in ("1.0",):
            return "mov1"
        return "movlit"
    if op.startswith("v_cndmask"):
        return "cndmask"
    if op.startswith(("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64")):
        return "rcp"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(("v_cvt", "v_ldexp", "v_frexp", "v_rndne", "v_floor", "v_fract", "v_trunc")):
        return "cvt"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if INT.match(op):
        return "int"
    return "other"


def main():
    if len(sys.argv) < 2 or sys.argv[1].startswith("-"):
        raise SystemExit(__doc__)
    lines = open(sys.argv[1]).read().splitlines()
    args = [a for a in sys.argv[2:] if not a.startswith("--")]
    # default: the metric's k_gradient<Cfg<3,3,0>, PlasmaPhys<3,3,3,true,false,ARGON_MINIMAL>> alone
    pat = args[0] if args else "10k_gradientINS_3CfgILi3ELi3ELi0EEENS_10PlasmaPhysILi3ELi3ELi3ELb1ELb0ELi1EEE"
    starts = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_ZN6tpsrhs\S*:", l)]
    for n, (i, name) in enumerate(starts):
        if pat not in name:
            continue
        j = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        segs, ops, others = [collections.Counter()], collections.Counter(), collections.Counter()
        for line in lines[i:j]:
            t = line.split(";")[0].strip()
            if not t or t.startswith(".") or t.endswith(":"):
                continue
            parts = t.split(None, 1)
            op, rest = parts[0], parts[1] if len(parts) > 1 else ""
            if op == "s_memtime":
                segs.append(collections.Counter())
            cl = classify(op, rest)
            if cl is None:
                continue
            segs[-1][cl] += 1
            if op.startswith("v_"):
                segs[-1]["valu"] += 1
                ops[op] += 1
                if cl == "other":
                    others[op] += 1
        print(name[:120])
        print("seg " + " ".join(f"{c:>7s}" for c in CLASSES))
        tot = collections.Counter()
        for k, s in enumerate(segs):
            tot.update(s)
            if len(segs) > 1:
                print(f"{k:3d} " + " ".join(f"{s[c]:7d}" for c in CLASSES))
        print("all " + " ".join(f"{tot[c]:7d}" for c in CLASSES))
        if "--top" in sys.argv:
            for k, v in ops.most_common(45):
                print(f"     {k:28s} {v}")
            print("  other:", dict(others.most_common(20)))


if __name__ == "__main__":
    main()
