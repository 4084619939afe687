"""Wall-clock time of one step of the device time loop, and of one Mult next to it (run on a GPU box):
    python tools/rk4_time.py [--integrator forwardEuler|rk2|rk3|rk4] [--workload cfg2|argon_p3|...] [--steps N]
rk4 goes through rk4_step, the others through step (tpsrhs_step); every step returns to the host, as a driver's loop does."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from tps_amd import capi, cases, meshgen  # noqa: E402
from tps_amd.rhs_operator import RHSoperator, node_coordinates  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--integrator", default="rk4", choices=sorted(set(capi.INTEGRATORS) - {"rk6"}))
ap.add_argument("--workload", default="cfg2", help="cfg2 (BASELINE configs[1]) or a workload of bench.py, e.g. argon_p3")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--dt", type=float, default=None, help="default: 1e-7 (cfg2), 1e-10 (the others: stiff chemistry)")
args = ap.parse_args()
sys.argv = [sys.argv[0]]

if args.workload == "cfg2":
    c = cases.config(2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    U, dt = c.state(), 1e-7
else:
    import bench  # noqa: E402

    order, physics, make_bcs, make_state, _, _ = bench.workload(args.workload)
    mesh = meshgen.ogrid_cylinder_slab(28, 112, 16, 0, 1)
    U, dt = make_state(node_coordinates(mesh, order), physics), 1e-10
    op = RHSoperator(mesh, capi.Disc(order, 0, 0, 0, 0), physics, make_bcs(physics))
if args.dt is not None:
    dt = args.dt
x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
y = torch.empty_like(x)


def one_step(t):
    return op.rk4_step(x, t, dt) if args.integrator == "rk4" else op.step(x, t, dt, args.integrator)


t = 0.0
for _ in range(3):
    t = one_step(t)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    t = one_step(t)
torch.cuda.synchronize()
el = (time.perf_counter() - t0) / args.steps
finite = bool(torch.isfinite(x).all())
for _ in range(3):
    op.Mult(x, y)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    op.Mult(x, y)
torch.cuda.synchronize()
mult = (time.perf_counter() - t0) / args.steps
nbytes = x.numel() * 8
print(f"{args.workload} {args.integrator} step ms {el * 1e3:.4f}  Mult ms {mult * 1e3:.4f}  step / Mult {el / mult:.3f}  "
      f"state vector MB {nbytes / 1e6:.1f}  finite {finite}")
