"""Two numbers for the point sampler (run on a GPU box; bench.py does not run this):
    python tools/sample_bench.py [--workload argon_p3] [--n 256] [--probes 64] [--steps 40] [--repeats 3]
 1. one sampling plane of n x n points, all num_equation rows of the state, on the metric's workload mesh (bench.py's
    default O-grid, 28 x 112 x 16 hexahedra at p = 3): device time per tpsrhs_sample next to the bytes such a sample must at
    least move -- the nodal values of the touched elements in every row, once, plus the output;
 2. steps per second of tpsrhs_advance (RK4, constant dt, the captured step graph on a side stream) with and without
    `--probes` probes recorded after every step, the two variants alternating in one process.
Times are host clocks around work that ends in a synchronise, after a warm-up of every shape; one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tps_amd import capi, meshgen  # noqa: E402
from tps_amd.rhs_operator import RHSoperator, node_coordinates, plane_points  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--workload", default="argon_p3", help="a workload of bench.py on the 3-D O-grid")
ap.add_argument("--nr", type=int, default=28)
ap.add_argument("--ntheta", type=int, default=112)
ap.add_argument("--nz", type=int, default=16)
ap.add_argument("--n", type=int, default=256, help="points per side of the plane")
ap.add_argument("--probes", type=int, default=64)
ap.add_argument("--steps", type=int, default=40, help="steps per timed advance call")
ap.add_argument("--repeats", type=int, default=3, help="timed advance calls per variant, alternating")
ap.add_argument("--dt", type=float, default=1.0e-10, help="constant and tiny, as bench.py --full: the state stays put")
args = ap.parse_args()
sys.argv = [sys.argv[0]]
import bench  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("sample_bench.py measures on a GPU; there is none here")
order, physics, make_bcs, make_state, _, _ = bench.workload(args.workload)
mesh = meshgen.ogrid_cylinder(args.nr, args.ntheta, args.nz)
side = torch.cuda.Stream()  # a capturable stream: advance replays its step graph
torch.cuda.set_stream(side)
op = RHSoperator(mesh, capi.Disc(order, 0, 0, 0, 0), physics, make_bcs(physics), stream=side)
neq, ndofs, npe = op.num_equation, op.NDofs, (order + 1) ** 3
U = make_state(node_coordinates(mesh, order), physics)
x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)

# ---- 1. one plane ------------------------------------------------------------------------------------------------------------
X = np.asarray(mesh.elem_coords).reshape(-1, 3)
bb0, bb1 = X.min(axis=0), X.max(axis=0)
t0 = time.perf_counter()
xyz = plane_points((0.0, 0.0, bb0[2] + 0.37 * (bb1[2] - bb0[2])), (0.0, 0.0, 1.0), bb0, bb1, args.n)
plane = op.createSampler(xyz)
locate_s = time.perf_counter() - t0
elem, _, nfound = plane.info()
touched = int(np.unique(elem[elem >= 0]).size)
npts = args.n * args.n
min_bytes = 8.0 * neq * (touched * npe + npts)
for _ in range(5):
    out = plane.sample(x)
torch.cuda.synchronize()
batch, times = 2000, []
for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(batch):
        out = plane.sample(x)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) / batch)
sample_s = statistics.median(times)
plane_result = {"points": npts, "found": int(nfound), "elements_touched": touched, "rows": neq,
                "locate_and_upload_s": round(locate_s, 4), "sample_us_median": round(1e6 * sample_s, 2),
                "sample_us_min_max": [round(1e6 * min(times), 2), round(1e6 * max(times), 2)],
                "min_bytes": min_bytes, "min_bytes_note": "8 * rows * (touched elements * (p+1)^3 + points); the per-point "
                "element id, reference coordinates and permutation (36 bytes a point) are not counted",
                "GB_per_s_of_min_bytes": round(min_bytes / sample_s / 1e9, 1), "finite": bool(torch.isfinite(out).all().item())}
plane.close()

# ---- 2. the time loop with and without probes ----------------------------------------------------------------------------------
rng = np.random.default_rng(1)
e = rng.integers(0, mesh.num_elements, size=args.probes)
xi = rng.uniform(0.05, 0.95, size=(3, args.probes))
corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
pts = np.zeros((3, args.probes))
for v, c in enumerate(corners):
    w = np.ones(args.probes)
    for d in range(3):
        w = w * (xi[d] if c[d] else 1.0 - xi[d])
    pts += np.asarray(mesh.elem_coords)[e, v, :].T * w
probes = op.createSampler(pts)
assert probes.info()[2] == args.probes


def loop(with_probes):
    op.configureProbes(probes if with_probes else None, 1, args.steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, bad = op.advance(x, 0.0, args.dt, args.steps, True)  # synchronises once, at its end
    dt = time.perf_counter() - t0
    if with_probes:
        iters, _, values, dropped = op.readProbes()
        assert len(iters) == args.steps and dropped == 0 and np.isfinite(values).all()
    return args.steps / dt, int(bad)


for w in (False, True):  # warm-up: allocations, the graph capture, the sampling kernel
    loop(w)
rates = {False: [], True: []}
for _ in range(args.repeats):
    for w in (False, True):
        r, bad = loop(w)
        rates[w].append(r)
off, on = statistics.median(rates[False]), statistics.median(rates[True])
loop_result = {"probes": args.probes, "interval": 1, "steps_per_call": args.steps, "calls_per_variant": args.repeats,
               "steps_per_s_without": round(off, 2), "steps_per_s_with": round(on, 2),
               "all_without": [round(r, 2) for r in rates[False]], "all_with": [round(r, 2) for r in rates[True]],
               "cost_percent": round(100.0 * (off / on - 1.0), 2), "nan_entries": bad}
op.close()
print(json.dumps({"tool": "sample_bench", "workload": args.workload, "mesh": [args.nr, args.ntheta, args.nz], "order": order,
                  "ndofs": ndofs, "device": torch.cuda.get_device_name(0), "plane": plane_result, "advance": loop_result}))
