"""One Mult of the table gas with two-dimensional (T, rho) tables against one Mult with one-dimensional tables (run on a GPU
box; bench.py does not run this):
    python tools/lte2d_time.py [--small] [--repeats 7] [--out profiles/rNN_lte2d.txt]
Both operators live in one process on the mesh of the lte_torch workload of bench.py (axisymmetric 400 x 500 quadrilaterals,
p = 3, 3.2 M nodes, radiation sink, viscosity-multiplier function, inlet / outlet / isothermal wall / axis) and see the same
state, whose density varies by 5 % around 0.255 kg/m^3.  Per operator: device time between two events around 10
back-to-back Mults after 3 warm-up Mults, per Mult; --repeats such batches, ALTERNATING between the two operators; median and
spread; then the split into the three sweeps from tpsrhs_kernel_times (events around every kernel: a run of its own, after the
timing above).  The model to hold the ratio against: per look-up one more cell search and a 32-byte cell record where the
one-dimensional gas reads two coefficients.
One JSON line at the end; --out also writes the text above it to a file."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--small", action="store_true", help="a tiny mesh: a rehearsal of the tool, not a measurement")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tps_amd import capi, cases, meshgen  # noqa: E402
from tps_amd.rhs_operator import RHSoperator, node_coordinates  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("lte2d_time.py measures on a GPU; there is none here")

nr, nz = (8, 10) if args.small else (400, 500)
mesh = meshgen.annulus_quad_slab(nr, nz, 0, 1, r_in=0.0, r_out=0.05, length_local=0.25)
bcs = cases.lte_axisym(2, 2, 3).bcs
disc = capi.Disc(3, 0, 0, 1, 0)


def physics(table_dim):
    ph = capi.lte2d_physics(capi.NS, radiation=True) if table_dim == 2 else capi.lte_physics(capi.NS, "rho0p255", radiation=True)
    vs = ph.visc_sponge  # [viscosityMultiplierFunction] of test/inputs/plasma.lte1d.ini:52-58 on this tube, as bench.py sets it
    vs.enabled, vs.width, vs.ratio = 1, 0.02, 20.0
    vs.normal[1], vs.point[1] = 1.0, 0.2
    return ph


X = node_coordinates(mesh, 3)
ph = {1: physics(1), 2: physics(2)}
U = cases.lte_state(X, ph[2], seed=12345, amp=0.05)  # rho e = rho e(T, rho) of the two-dimensional table for both
ops = {d: RHSoperator(mesh, disc, ph[d], bcs) for d in (1, 2)}
x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=ops[1].device)
y = {d: torch.empty_like(x) for d in (1, 2)}


def batch(d, calls=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        ops[d].Mult(x, y[d])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


for d in (1, 2):
    for _ in range(3):
        ops[d].Mult(x, y[d])
torch.cuda.synchronize()
ms = {1: [], 2: []}
for _ in range(args.repeats):
    for d in (1, 2):
        ms[d].append(batch(d))
split = {}
for d in (1, 2):
    ops[d].enable_kernel_timing(True)
    for _ in range(10):
        ops[d].Mult(x, y[d])
    torch.cuda.synchronize()
    split[d] = {k: round(v, 4) for k, v in ops[d].kernel_times().items()}
    ops[d].enable_kernel_timing(False)
yy = {d: y[d].cpu().numpy().reshape(U.shape) for d in (1, 2)}
finite = bool(np.isfinite(yy[1]).all() and np.isfinite(yy[2]).all())
med = {d: statistics.median(ms[d]) for d in (1, 2)}
res = {"tool": "lte2d_time", "device": torch.cuda.get_device_name(0), "small": args.small, "nodes": int(X.shape[1]),
       "mult_ms_1d": {"median": round(med[1], 4), "min_max": [round(min(ms[1]), 4), round(max(ms[1]), 4)]},
       "mult_ms_2d": {"median": round(med[2], 4), "min_max": [round(min(ms[2]), 4), round(max(ms[2]), 4)]},
       "ratio_2d_over_1d": round(med[2] / med[1], 4), "kernel_ms_1d": split[1], "kernel_ms_2d": split[2], "finite": finite}
lines = [f"lte2d_time on {res['device']}: {nr} x {nz} quadrilaterals, p = 3, {res['nodes']} nodes, {args.repeats} alternating batches of 10 Mults",
         f"  one-dimensional tables: Mult {res['mult_ms_1d']['median']} ms (min / max {res['mult_ms_1d']['min_max']}), sweeps {split[1]}",
         f"  two-dimensional tables: Mult {res['mult_ms_2d']['median']} ms (min / max {res['mult_ms_2d']['min_max']}), sweeps {split[2]}",
         f"  ratio 2-D / 1-D: {res['ratio_2d_over_1d']}; outputs finite: {finite}"]
print("\n".join(lines))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
for op in ops.values():
    op.close()
