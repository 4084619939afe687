"""Time of tpsrhs_visualization_fields (run on a GPU box; bench.py does not run this):
    python tools/vis_fields_time.py [--small] [--repeats 5] [--case argon_p3,cfg5]
On the metric's workload (3-D O-grid, 28 x 112 x 16 hexahedra, p = 3, ambipolar argon ternary, 3.2 M nodes) and on BASELINE
configuration 5 (axisymmetric two-temperature argon, 400 x 500 quadrilaterals, p = 3, 3.2 M nodes), per case:
 - device time between two events around 10 back-to-back calls (after 3 warm-up calls), per call, median and spread of
   --repeats such batches, of: the whole tpsrhs_visualization_fields; tpsrhs_update_gradients alone (its first part); their
   difference = the four post-processing passes; and one Mult, the yardstick;
 - the algorithmic bytes of the four passes -- U once per pass, the temperatures of Up in the two source passes, the density
   and species rows of gradUp in the flux pass, nrows written -- and the time they take at the measured copy rate of the
   card (6.29 TB/s), as a fraction of the measured time of the passes.
One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--small", action="store_true", help="tiny meshes: a rehearsal of the tool, not a measurement")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--case", default="argon_p3,cfg5")
args = ap.parse_args()

import torch  # noqa: E402

from tps_amd import cases  # noqa: E402
from tps_amd.rhs_operator import RHSoperator  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("vis_fields_time.py measures on a GPU; there is none here")
HBM = 6.29e12  # bytes / s, the measured copy rate of the card


def build(name):
    if name == "argon_p3":
        return cases.argon_cyl3d(*((4, 12, 3) if args.small else (28, 112, 16)), 3)
    if name == "cfg5":
        return cases.argon_axisym(8, 10, 3, name="cfg5_small") if args.small else cases.config(5)
    raise SystemExit(f"unknown case {name}")


def device_ms(call, calls=10):
    for _ in range(3):
        call()
    out = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            call()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def stat(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


res = {"tool": "vis_fields_time", "device": torch.cuda.get_device_name(0), "small": args.small, "cases": {}}
for name in args.case.split(","):
    c = build(name)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    lay = op.visualizationLayout()
    x = torch.tensor(c.state(seed=1, amp=0.01).ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    out = torch.empty((lay.nrows, op.NDofs), dtype=torch.float64, device=op.device)
    lib, h = op._lib, op._h

    def fields():
        assert lib.tpsrhs_visualization_fields(h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())) == 0

    t_all, t_grad, t_mult = device_ms(fields), device_ms(lambda: op.updateGradients(x)), device_ms(lambda: op.Mult(x, y))
    mx = c.physics.mixture
    nact = mx.num_species - (2 if mx.ambipolar else 1)
    rows_read = 4 * op.num_equation + 2 * (2 if mx.two_temperature else 1) + op.dim * (1 + nact)
    nbytes = 8.0 * op.NDofs * (rows_read + lay.nrows)
    passes = statistics.median(t_all) - statistics.median(t_grad)
    res["cases"][name] = {
        "ndofs": op.NDofs, "num_equation": op.num_equation, "nrows": lay.nrows, "finite": bool(torch.isfinite(out).all()),
        "visualization_fields": stat(t_all), "update_gradients": stat(t_grad), "passes_ms": round(passes, 4),
        "mult": stat(t_mult), "passes_over_mult": round(passes / statistics.median(t_mult), 3),
        "algorithmic_bytes": nbytes, "streaming_bound_ms": round(1e3 * nbytes / HBM, 4),
        "fraction_of_hbm_roofline": round(1e3 * nbytes / HBM / passes, 3) if passes > 0 else None}
    op.close()
print(json.dumps(res))
