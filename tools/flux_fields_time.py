"""Time of tpsrhs_get_flux (run on a GPU box; bench.py does not run this):
    python tools/flux_fields_time.py [--workload argon_p3|cfg2] [--small] [--repeats 5]
On the O-grid of the bench's argon_p3 and cfg2 workloads (28 x 112 x 16 hexahedra, p = 3, 3.2 M nodes; the reacting argon
ternary plasma / Navier-Stokes dry air):
 - tpsrhs_get_flux of each part with gradients_current = 1 (the pass alone) and of TOTAL with gradients_current = 0 (the
   gradient sweeps first), next to tpsrhs_mult of the same process: device time between two events around 10 back-to-back
   calls (after 3 warm-up calls), per call, median and spread of --repeats such batches;
 - the bytes of the model, (neq + 2 dim neq) * 8 per node -- the state and the gradient read, the tensor written -- over the
   time of the pass, as a fraction of the 5.8 TB/s streaming rate DESIGN.md section 9 records for this box.
One JSON line per workload at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--workload", action="append", choices=["argon_p3", "cfg2"], help="default: both")
ap.add_argument("--small", action="store_true", help="a tiny mesh: a rehearsal of the tool, not a measurement")
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

import torch  # noqa: E402

from tps_amd import capi, cases  # noqa: E402
from tps_amd.rhs_operator import RHSoperator  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("flux_fields_time.py measures on a GPU; there is none here")
STREAM_RATE = 5.8e12  # bytes / s, DESIGN.md section 9
shape = (4, 12, 3) if args.small else (28, 112, 16)
for wname in args.workload or ["argon_p3", "cfg2"]:
    c = cases.argon_cyl3d(*shape, 3) if wname == "argon_p3" else cases.cyl3d(*shape, 3, capi.NS, capi.VISC_ISOTH)
    U = c.state(seed=12345)
    res = {"tool": "flux_fields_time", "workload": wname, "device": torch.cuda.get_device_name(0), "small": args.small}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        n, neq, dim = op.NDofs, op.num_equation, op.dim
        res["ndofs"], res["neq"] = n, neq
        x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
        y = torch.empty_like(x)

        def device_ms(call, calls=10):
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

        def entry(ms):
            return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}

        res["mult"] = entry(device_ms(lambda: op.Mult(x, y)))
        op.Mult(x, y)  # Up / gradUp of x are held from here on
        model_bytes = (neq + 2 * dim * neq) * 8 * n
        for part in ("total", "convective", "viscous"):
            ms = device_ms(lambda: op.getFlux(x, part, gradients_current=True))
            e = entry(ms)
            e["model_GB_per_s"] = round(model_bytes / (statistics.median(ms) * 1e-3) / 1e9, 1)
            e["fraction_of_streaming_rate"] = round(model_bytes / (statistics.median(ms) * 1e-3) / STREAM_RATE, 3)
            res["get_flux_" + part + "_current"] = e
        res["get_flux_total_with_gradients"] = entry(device_ms(lambda: op.getFlux(x, "total")))
        res["model_bytes"] = model_bytes
        side.synchronize()
        op.close()
    print(json.dumps(res), flush=True)
