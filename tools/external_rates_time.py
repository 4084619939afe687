"""Time of the pass of the reactions with an external rate coefficient (run on a GPU box; bench.py does not run this):
    python tools/external_rates_time.py [--small] [--repeats 5]
On the metric's workload (3-D O-grid, 28 x 112 x 16 hexahedra, p = 3, ambipolar argon ternary, 3.2 M nodes) with BOTH
reactions external (components 0 and 1 of a two-component array):
 - device time between two events around 10 back-to-back Mults (after 3 warm-up calls), per Mult, median and spread of
   --repeats such batches: with the rate array set, and with none (the sweeps alone: they hold no reaction either way); the
   difference is the pass;
 - the same for tpsrhs_boltzmann_fields;
 - the bytes the pass must move -- the state rows read, the rate components read, NACTIVE (+ 1 for two temperatures) rows of y
   read and written -- and the time they take at the card's HBM rates: the spec rate of bench.py's roofline (8.0 TB/s) and
   the measured copy rate (6.29 TB/s).
One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--small", action="store_true", help="a tiny mesh: a rehearsal of the tool, not a measurement")
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

import torch  # noqa: E402

from tps_amd import capi, cases  # noqa: E402
from tps_amd.rhs_operator import RHSoperator  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("external_rates_time.py measures on a GPU; there is none here")
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: bench.py's HBM_PEAK_GBS and the measured copy rate


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


c = cases.argon_cyl3d(*((4, 12, 3) if args.small else (28, 112, 16)), 3)
ph = c.physics
for r in range(2):  # model = bte, bte/index = r
    ph.chemistry.reaction_models[r] = capi.GRIDFUNCTION_RXN
    ph.chemistry.rate_params[0 + r * capi.MAXCHEMPARAMS] = float(r)
op = RHSoperator(c.mesh, c.disc, ph, c.bcs)
x = torch.tensor(c.state(seed=1, amp=0.01).ravel(), dtype=torch.float64, device=op.device)
y = torch.empty_like(x)
rates = torch.full((2, op.NDofs), 1.0e-3, dtype=torch.float64, device=op.device)
t_sweeps = device_ms(lambda: op.Mult(x, y))
op.setReactionRates(rates)
t_with = device_ms(lambda: op.Mult(x, y))
finite = bool(torch.isfinite(y).all())
op.setReactionRates(None)
t_sweeps2 = device_ms(lambda: op.Mult(x, y))
t_push = device_ms(lambda: op.boltzmannFields(x))
mx = ph.mixture
nact = mx.num_species - (2 if mx.ambipolar else 1)
yrows = nact + (1 if mx.two_temperature else 0)
nbytes = 8.0 * op.NDofs * (op.num_equation + 2 + 2 * yrows)
push_bytes = 8.0 * op.NDofs * (op.num_equation + mx.num_species + 2)
base = statistics.median(t_sweeps + t_sweeps2)
pass_ms = statistics.median(t_with) - base
res = {"tool": "external_rates_time", "device": torch.cuda.get_device_name(0), "small": args.small, "ndofs": op.NDofs,
       "num_equation": op.num_equation, "finite": finite,
       "mult_without_array": stat(t_sweeps), "mult_without_array_again": stat(t_sweeps2), "mult_with_array": stat(t_with),
       "pass_ms": round(pass_ms, 4), "pass_bytes": nbytes,
       "pass_bound_ms_at_8.0_TBs": round(1e3 * nbytes / HBM_SPEC, 4), "pass_bound_ms_at_6.29_TBs": round(1e3 * nbytes / HBM_COPY, 4),
       "pass_fraction_of_copy_rate": round(1e3 * nbytes / HBM_COPY / pass_ms, 3) if pass_ms > 0 else None,
       "boltzmann_fields": stat(t_push), "boltzmann_fields_bytes": push_bytes,
       "boltzmann_fields_bound_ms_at_6.29_TBs": round(1e3 * push_bytes / HBM_COPY, 4)}
op.close()
print(json.dumps(res))
