"""What the conservative limiter costs on the benchmark's workload (reacting argon, 3-D p = 3, 28 x 112 x 16 hexahedra), where no
element undershoots (run on a GPU box):
    python tools/limiter_time.py [--steps N] [--repeats R]
(a) one k_limit launch (tpsrhs_limit, the default rows) between two events, and (b) ms per step of tpsrhs_advance (RK4, the
captured step graph) and of forward Euler with the limiter off and on, R rounds in turn after a warm-up advance each.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/limiter_time.py --trace
runs forward-Euler steps with the limiter on and nothing else: the final-stage k_rk_stage launch and k_limit in one
process, on the same state;
    python tools/limiter_time.py --kernel-stats DIR
then prints their average durations and achieved bytes / s from the kernel_stats.csv under DIR."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--workload", default="argon_p3")
ap.add_argument("--mesh", type=int, nargs=3, default=[28, 112, 16], metavar=("NR", "NTHETA", "NZ"))
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--dt", type=float, default=1e-10)
ap.add_argument("--trace", action="store_true", help="forward-Euler steps with the limiter on, for rocprofv3 --kernel-trace --stats")
ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="summarise the kernel_stats.csv of such a run")
ap.add_argument("--neq", type=int, default=6, help="--kernel-stats: rows of the state")
ap.add_argument("--ndofs", type=int, default=28 * 112 * 16 * 64, help="--kernel-stats: nodes")
ap.add_argument("--rows", type=int, default=1, help="--kernel-stats: rows the limiter lists")
args = ap.parse_args()
sys.argv = [sys.argv[0]]

if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"limiter_time --kernel-stats: no *kernel_stats.csv under {args.kernel_stats} "
                 "(rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- ...)")
    with open(max(files, key=os.path.getmtime)) as f:
        rows = list(csv.DictReader(f))
    vec = args.ndofs * 8
    model = {"k_rk_stage": 3 * args.neq * vec, "k_limit": (args.rows + 1) * vec}  # x, k read and x written; rows + the weights read
    out = {}
    for r in rows:
        for k, nbytes in model.items():
            if k + "<" in r["Name"] or r["Name"].split("(")[0].endswith(k):
                ms = float(r["AverageNs"]) * 1e-6
                out[k] = {"calls": int(r["Calls"]), "ms_average": round(ms, 5), "ms_min_max": [float(r["MinNs"]) * 1e-6, float(r["MaxNs"]) * 1e-6],
                          "bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 1)}
    if len(out) == 2:
        out["k_limit_over_k_rk_stage_time"] = round(out["k_limit"]["ms_average"] / out["k_rk_stage"]["ms_average"], 3)
        out["k_limit_over_k_rk_stage_bytes_per_s"] = round(out["k_limit"]["GB_per_s"] / out["k_rk_stage"]["GB_per_s"], 3)
    print(json.dumps({"tool": "limiter_time --kernel-stats", **out}))
    sys.exit(0)

import torch  # noqa: E402

import bench  # noqa: E402
from tps_amd import capi, meshgen  # noqa: E402
from tps_amd.rhs_operator import RHSoperator, node_coordinates  # noqa: E402

side = torch.cuda.Stream()  # a capturable stream: advance replays its step graph
torch.cuda.set_stream(side)
order, physics, make_bcs, make_state, _, _ = bench.workload(args.workload)
mesh = meshgen.ogrid_cylinder_slab(*args.mesh, 0, 1)
U = make_state(node_coordinates(mesh, order), physics)
op = RHSoperator(mesh, capi.Disc(order, 0, 0, 0, 0), physics, make_bcs(physics), stream=side)
x0 = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
x = x0.clone()

if args.trace:
    op.configureLimiter()
    op.advance(x, 0.0, args.dt, args.steps, True, integrator="forwardEuler")
    torch.cuda.synchronize()
    print("limiter_time --trace:", op.readLimiter())
    sys.exit(0)


def advance_ms(integrator):
    """ms per step of one advance call of args.steps steps, after a warm-up advance (allocations, the capture)"""
    x.copy_(x0)
    t, _, _ = op.advance(x, 0.0, args.dt, 4, True, integrator=integrator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op.advance(x, t, args.dt, args.steps, True, integrator=integrator)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


res = {"tool": "limiter_time", "device": torch.cuda.get_device_name(0), "workload": args.workload, "ndofs": op.NDofs,
       "neq": op.num_equation, "steps": args.steps, "repeats": args.repeats}
for integrator in ("rk4", "forwardEuler"):
    off, on = [], []
    for _ in range(args.repeats):
        op.configureLimiter(off=True)
        off.append(advance_ms(integrator))
        op.configureLimiter()
        on.append(advance_ms(integrator))
    res[integrator] = {"ms_per_step_off": round(statistics.median(off), 4), "ms_per_step_on": round(statistics.median(on), 4),
                       "off_min_max": [round(min(off), 4), round(max(off), 4)], "on_min_max": [round(min(on), 4), round(max(on), 4)],
                       "difference_ms": round(statistics.median(on) - statistics.median(off), 4)}
op.configureLimiter(off=True)
rep = op.readLimiter(reset=True)
res["elements_limited_or_clamped_in_the_loop"] = int(rep["limited"].sum() + rep["clamped"].sum())
# (a) one k_limit launch between two events
x.copy_(x0)
for _ in range(3):
    op.limit(x)
torch.cuda.synchronize()
ms = []
for _ in range(max(args.steps, 20)):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(side)
    op.limit(x)
    e1.record(side)
    e1.synchronize()
    ms.append(e0.elapsed_time(e1))
nbytes = 2 * op.NDofs * 8  # the species row and the weights; nothing is written
res["k_limit_between_events"] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                 "bytes": nbytes, "GB_per_s": round(nbytes / statistics.median(ms) / 1e6, 1)}
# ... and one Mult with the kernel timing on: the k_traces sweep the unchained RK4 step runs once more
op.enable_kernel_timing(True)
y = torch.empty_like(x)
for _ in range(5):
    op.Mult(x0, y)
torch.cuda.synchronize()
res["kernel_ms_of_one_Mult"] = op.kernel_times()
print(json.dumps(res))
