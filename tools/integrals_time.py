"""Time of the device reductions and of the monitor in the time loop (run on a GPU box; bench.py does not run this):
    python tools/integrals_time.py [--small] [--no-monitor] [--repeats 5]
On the O-grid of BASELINE configuration 2 (28 x 112 x 16 hexahedra, p = 3, 3.2 M nodes, Navier-Stokes dry air):
 - tpsrhs_integrate and tpsrhs_nodal_stats of the 5-row state: device time between two events around 20 back-to-back calls
   (after 3 warm-up calls), per call, median of --repeats such batches, next to the streaming bound 8 nrows NDofs bytes at
   6.29 TB/s (the measured copy rate of the card);
 - tpsrhs_advance, 100 RK4 steps at constant dt on a capturable side stream: wall-clock time per step with the monitor off
   and with it on at interval 10 (capacity 16), alternating off / on --repeats times after one warm-up run each; the
   median and the spread (min, max) of each.  --no-monitor: a library without the monitor (the parent commit's, through
   TPSRHS_LIB): only the `off` series.
One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--small", action="store_true", help="a tiny mesh: a rehearsal of the tool, not a measurement")
ap.add_argument("--no-monitor", action="store_true", help="the library has no reductions and no monitor: time the plain loop only")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=100)
args = ap.parse_args()

import torch  # noqa: E402

from tps_amd import cases  # noqa: E402
from tps_amd.rhs_operator import RHSoperator  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("integrals_time.py measures on a GPU; there is none here")
c = cases.cyl3d(*((4, 12, 3) if args.small else (28, 112, 16)), 3)
U = c.state(seed=1)
res = {"tool": "integrals_time", "device": torch.cuda.get_device_name(0), "small": args.small, "steps": args.steps}
side = torch.cuda.Stream()
with torch.cuda.stream(side):
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
    res["ndofs"], res["nrows"] = op.NDofs, op.num_equation
    x0 = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)

    def device_ms(call, calls=20):
        for _ in range(3):
            call()
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            for _ in range(calls):
                call()
            b.record(side)
            b.synchronize()
            out.append(a.elapsed_time(b) / calls)
        return out

    if not args.no_monitor:
        bound_us = 8.0 * op.num_equation * op.NDofs / 6.29e12 * 1e6
        for name, call in (("integrate", lambda: op.integrate(x0)), ("nodal_stats", lambda: op.nodalStats(x0))):
            ms = device_ms(call)
            res[name] = {"us_median": round(1e3 * statistics.median(ms), 2), "us_min_max": [round(1e3 * min(ms), 2), round(1e3 * max(ms), 2)],
                         "streaming_bound_us": round(bound_us, 2), "fraction_of_bound": round(bound_us / (1e3 * statistics.median(ms)), 3)}

    def loop(monitor):
        if not args.no_monitor:
            op.configureMonitor(10 if monitor else 0, 16 if monitor else 0)
        x = x0.clone()
        side.synchronize()
        t0 = time.perf_counter()
        op.advance(x, 0.0, 2.0e-7, args.steps, True)  # returns after the stream synchronise
        return (time.perf_counter() - t0) / args.steps

    series = {"off": []} if args.no_monitor else {"off": [], "on": []}
    for key in series:
        loop(key == "on")  # warm-up: allocations, graph capture
    for _ in range(args.repeats):
        for key in series:
            series[key].append(loop(key == "on"))
    for key, ts in series.items():
        res["advance_monitor_" + key] = {"ms_per_step_median": round(1e3 * statistics.median(ts), 4),
                                         "ms_per_step_min_max": [round(1e3 * min(ts), 4), round(1e3 * max(ts), 4)]}
    if not args.no_monitor:
        rec = op.readMonitor()
        res["records_in_last_run"] = int(len(rec["iters"]))
    side.synchronize()
    op.close()
print(json.dumps(res))
