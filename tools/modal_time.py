"""What the modal filter costs on the benchmark's workload (reacting argon, 3-D p = 3, 28 x 112 x 16 hexahedra; run on a GPU box):
    python tools/modal_time.py [--steps N] [--repeats R]
(a) one k_modal_filter launch (tpsrhs_modal_filter_apply) between two events -- all rows without a sensor, and with a sensor
at a threshold that filters nothing -- and (b) ms per step of tpsrhs_advance (RK4, the captured step graph) with the filter off
and on, R rounds in turn after a warm-up advance each.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/modal_time.py --trace
runs forward-Euler steps with the filter on and nothing else: the final-stage k_rk_stage launch and k_modal_filter in one
process, on the same state;
    python tools/modal_time.py --kernel-stats DIR
then prints their average durations and achieved bytes / s from the kernel_stats.csv under DIR.  The byte model of the
filter: every row read once and written once and the weights read once, 2 * 8 * neq + 8 bytes per node."""
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
ap.add_argument("--trace", action="store_true", help="forward-Euler steps with the filter on, for rocprofv3 --kernel-trace --stats")
ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="summarise the kernel_stats.csv of such a run")
ap.add_argument("--neq", type=int, default=6, help="--kernel-stats: rows of the state")
ap.add_argument("--ndofs", type=int, default=28 * 112 * 16 * 64, help="--kernel-stats: nodes")
args = ap.parse_args()
sys.argv = [sys.argv[0]]
FILTER = dict(cutoff=1, alpha=36.0, exponent=16, conservative=True)


def filter_bytes(neq, ndofs):
    return (2 * neq + 1) * ndofs * 8


if args.kernel_stats:
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"modal_time --kernel-stats: no *kernel_stats.csv under {args.kernel_stats} "
                 "(rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- ...)")
    with open(max(files, key=os.path.getmtime)) as f:
        rows = list(csv.DictReader(f))
    vec = args.ndofs * 8
    model = {"k_rk_stage": 3 * args.neq * vec, "k_modal_filter": filter_bytes(args.neq, args.ndofs)}  # x, k read and x written
    out = {}
    for r in rows:
        for k, nbytes in model.items():
            if k + "<" in r["Name"] or r["Name"].split("(")[0].endswith(k):
                ms = float(r["AverageNs"]) * 1e-6
                out[k] = {"calls": int(r["Calls"]), "ms_average": round(ms, 5), "ms_min_max": [float(r["MinNs"]) * 1e-6, float(r["MaxNs"]) * 1e-6],
                          "bytes": nbytes, "GB_per_s": round(nbytes / ms / 1e6, 1)}
    if len(out) == 2:
        out["k_modal_filter_over_k_rk_stage_time"] = round(out["k_modal_filter"]["ms_average"] / out["k_rk_stage"]["ms_average"], 3)
        out["k_modal_filter_over_k_rk_stage_bytes_per_s"] = round(out["k_modal_filter"]["GB_per_s"] / out["k_rk_stage"]["GB_per_s"], 3)
    print(json.dumps({"tool": "modal_time --kernel-stats", **out}))
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
    op.configureModalFilter(**FILTER)
    op.advance(x, 0.0, args.dt, args.steps, True, integrator="forwardEuler")
    torch.cuda.synchronize()
    print("modal_time --trace:", op.readModalFilter())
    sys.exit(0)


def advance_ms():
    """ms per step of one RK4 advance call of args.steps steps, after a warm-up advance (allocations, the capture)"""
    x.copy_(x0)
    t, _, _ = op.advance(x, 0.0, args.dt, 4, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    op.advance(x, t, args.dt, args.steps, True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


res = {"tool": "modal_time", "device": torch.cuda.get_device_name(0), "workload": args.workload, "ndofs": op.NDofs,
       "neq": op.num_equation, "steps": args.steps, "repeats": args.repeats, "filter": FILTER}
off, on = [], []
for _ in range(args.repeats):
    op.configureModalFilter(off=True)
    off.append(advance_ms())
    op.configureModalFilter(**FILTER)
    on.append(advance_ms())
res["rk4"] = {"ms_per_step_off": round(statistics.median(off), 4), "ms_per_step_on": round(statistics.median(on), 4),
              "off_min_max": [round(min(off), 4), round(max(off), 4)], "on_min_max": [round(min(on), 4), round(max(on), 4)],
              "difference_ms": round(statistics.median(on) - statistics.median(off), 4)}
op.configureModalFilter(off=True)
res["counters_in_the_loop"] = op.readModalFilter(reset=True)


def launch_ms(**kw):
    """one k_modal_filter launch between two events, on the unfiltered state every time"""
    ms = []
    for i in range(max(args.steps, 20) + 3):
        x.copy_(x0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        op.modalFilter(x, **kw)
        e1.record(side)
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return ms


# (a) all rows, no sensor: every row read and written, the weights read
ms = launch_ms(**FILTER)
nbytes = filter_bytes(op.num_equation, op.NDofs)
res["k_modal_filter_all_rows"] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                  "bytes": nbytes, "GB_per_s": round(nbytes / statistics.median(ms) / 1e6, 1)}
# ... and with the sensor of the density at a threshold no element reaches: one row read, nothing written
ms = launch_ms(sensor_row=0, sensor_threshold=0.999999, **FILTER)
nbytes = op.NDofs * 8
res["k_modal_filter_sensor_only"] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                     "bytes": nbytes, "GB_per_s": round(nbytes / statistics.median(ms) / 1e6, 1),
                                     "counters": op.readModalFilter()}
print(json.dumps(res))
