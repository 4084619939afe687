"""The record behind tests/test_mms_boundaries.py: observed orders of the residual next to walls, inlets and outlets against
the exact right-hand side of manufactured states that satisfy the boundary conditions.

    python tools/bc_mms_rates.py                 the oracle at the committed resolution pairs, negative controls included
    python tools/bc_mms_rates.py --hip           the same through the HIP operator (needs a GPU)
    python tools/bc_mms_rates.py --scan [name dim order ...]
                                                 the search for the pairs: per case the oracle's rates for growing n until the
                                                 band of the test is met with 0.1 of rate to spare
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import test_mms_boundaries as T  # noqa: E402

ORACLE_ORDERS = [(2, 1), (2, 2), (2, 3), (2, 4), (3, 2), (3, 3)]
N_MAX = {2: 9, 3: 5}  # 2-D stays under 20^2 quads on the fine mesh, 3-D at 10^3 hexes


def scan(run, name, dim, order, lag=1.0):
    for n in range(3 if dim == 3 else (3 if order > 2 else 4), N_MAX[dim] + 1):
        r = T.layer_rates(run, T.CONFIGS[name], dim, order, n)
        ok = T.in_band(r["near"], order, 0.1, lag) and T.in_band(r["inner"], order, 0.1, lag) and r["fine"] < 0.3
        print("%-18s %d-D p=%d n=%d  %s%s" % (name, dim, order, n, T._fmt(r), "  <== smallest n in the band + 0.1" if ok else ""), flush=True)
        if ok:
            return n
    return None


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    run = T.hip_run if "--hip" in sys.argv else T.oracle_run
    if "--scan" in sys.argv:
        if args:
            todo = [(args[i], int(args[i + 1]), int(args[i + 2])) for i in range(0, len(args), 3)]
        else:
            todo = [(name, d, p) for name in T.CONFIGS for d, p in ORACLE_ORDERS
                    if p > 1 and not (name.startswith("ternary") and (d, p) not in ((2, 2), (2, 3), (3, 2), (3, 3)))]
        for name, d, p in todo:
            scan(run, name, d, p)
        sys.exit(0)
    print("# resolution pairs n -> 2 n of tests/test_mms_boundaries.py::RESOLUTION, %s" % ("HIP operator" if "--hip" in sys.argv else "oracle"))
    for (name, d, p), n in T.RESOLUTION.items():
        r = T.layer_rates(run, T.CONFIGS[name], d, p, n)
        print("%-18s %d-D p=%d n=%d  %s" % (name, d, p, n, T._fmt(r)), flush=True)
    print("# the unwarped, unscrambled 2-D case")
    name, d, p, n = T.SANITY
    print("%-18s %d-D p=%d n=%d  %s" % (name, d, p, n, T._fmt(T.layer_rates(run, T.CONFIGS[name], d, p, n, warp=0.0, scramble=False))))
    print("# p = 1, one 2-D case per patch kind")
    for name, n, _, _ in T.P1_CASES:
        print("%-18s %d-D p=%d n=%d  %s" % (name, 2, 1, n, T._fmt(T.layer_rates(run, T.CONFIGS[name], 2, 1, n))), flush=True)
    print("# Navier-Stokes at the reflecting inlet / outlet: no viscous flux on these patches (the reference's behaviour); only the"
          " inner rates and the near-layer continuity rate are asserted")
    d, p, n = T.NS_INOUT
    print("%-18s %d-D p=%d n=%d  %s" % ("inout_ns", d, p, n, T._fmt(T.layer_rates(run, T.CONFIGS["inout_ns"], d, p, n))), flush=True)
    print("# negative controls, 2-D p=2: the near-layer rate of the named equation must be below 0, the inner rates stay in the band")
    for label in T.CONTROLS:
        r = T.control_rates(run, label)
        print("%-18s n=%d  %s" % (label, T.CONTROLS[label][-1], T._fmt(r)), flush=True)
