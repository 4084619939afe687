"""Three numbers for the mesh-to-mesh transfer (run on a GPU box; bench.py does not run this):
    python tools/transfer_bench.py [--src 28 112 16] [--dst 42 168 24] [--order 3] [--repeats 5]
The source is the metric's O-grid (bench.py's argon_p3 mesh, 28 x 112 x 16 hexahedra at p = 3) with a 5-row state, the
target the same generator at 42 x 168 x 24.
 1. the FIRST tpsrhs_transfer of a pair: grid build and upload, node coordinates, k_locate, k_sample -- one fresh pair of
    operators per repeat, timed to the synchronisation that num_missing forces;
 2. a REPEATED tpsrhs_transfer of the same pair (the cached sampler: one k_sample launch), batches timed to a synchronise;
 3. the route without the device locator for the same coordinates: tps_amd.rhs_operator.node_coordinates on the host,
    tpsrhs_sampler_create (serial host location, the sort, three uploads) and tpsrhs_sample.
Times are host clocks around work that ends in a synchronise, after a warm-up of every kernel on a small pair; medians with
minimum and maximum; one JSON line at the end."""
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

from tps_amd import capi, cases, meshgen  # noqa: E402
from tps_amd.rhs_operator import RHSoperator, node_coordinates  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--src", type=int, nargs=3, default=[28, 112, 16], help="nr ntheta nz of the source O-grid")
ap.add_argument("--dst", type=int, nargs=3, default=[42, 168, 24], help="nr ntheta nz of the target O-grid")
ap.add_argument("--order", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5, help="first transfers (fresh pairs) and host-route runs")
ap.add_argument("--batch", type=int, default=20, help="repeated transfers per timed batch")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("transfer_bench.py measures on a GPU; there is none here")


def operator(n, order):
    mesh = meshgen.ogrid_cylinder(*n)
    return mesh, RHSoperator(mesh, capi.Disc(order, 0, 0, 0, 0), capi.dry_air_physics(capi.NS), cases.cylinder_bcs())


def spread(ts):
    return {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "n": len(ts)}


# warm-up: every kernel of both routes once, on a small pair (code objects loaded, allocator primed)
m0, a0 = operator((4, 12, 3), args.order)
m1, b0 = operator((5, 14, 4), args.order)
x0 = torch.ones(5 * a0.NDofs, dtype=torch.float64, device=a0.device)
b0.transferFrom(a0, x0)
a0.createSampler(node_coordinates(m1, args.order)).sample(x0)
torch.cuda.synchronize()
a0.close()
b0.close()

src_mesh, src = operator(args.src, args.order)
U = cases.dry_air_state(node_coordinates(src_mesh, args.order), seed=1)
x = torch.tensor(U.ravel(), dtype=torch.float64, device=src.device)
first, missing_dev = [], None
for _ in range(args.repeats):
    src.close()
    src_mesh, src = operator(args.src, args.order)  # a fresh source: no uploaded grid, no cached sampler
    dst_mesh, dst = operator(args.dst, args.order)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, missing_dev = dst.transferFrom(src, x)  # num_missing synchronises
    first.append(time.perf_counter() - t0)
    assert src.transferStats() == (1, 0)
    if _ + 1 < args.repeats:
        dst.close()
repeated = []
for _ in range(3):
    out, _m = dst.transferFrom(src, x)
torch.cuda.synchronize()
lib, h_src, h_dst = capi.load(), src._h, dst._h
import ctypes as C  # noqa: E402

for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(args.batch):  # through the C ABI with num_missing NULL: no synchronisation inside the batch
        assert lib.tpsrhs_transfer(h_src, h_dst, 5, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0.0, 0.0, None) == 0
    torch.cuda.synchronize()
    repeated.append((time.perf_counter() - t0) / args.batch)
dev_values = out.cpu().numpy()

host_total, host_coords, host_create, host_sample = [], [], [], []
for _ in range(args.repeats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X = node_coordinates(dst_mesh, args.order)
    t1 = time.perf_counter()
    s = src.createSampler(X)
    t2 = time.perf_counter()
    got = s.sample(x)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    host_coords.append(t1 - t0)
    host_create.append(t2 - t1)
    host_sample.append(t3 - t2)
    host_total.append(t3 - t0)
    nfound_host = s.info()[2]
    if _ + 1 < args.repeats:
        s.close()
host_values = got.cpu().numpy()
both = np.isfinite(dev_values) & np.isfinite(host_values)
result = {"tool": "transfer_bench", "device": torch.cuda.get_device_name(0), "order": args.order, "rows": 5,
          "src_mesh": args.src, "dst_mesh": args.dst, "src_ndofs": src.NDofs, "dst_ndofs": dst.NDofs,
          "missing_device": int(missing_dev), "missing_host": int(dst.NDofs - nfound_host),
          "max_abs_difference_of_routes": float(np.abs(dev_values - host_values)[both].max()),
          "first_transfer": spread(first), "repeated_transfer": spread(repeated),
          "host_route_total": spread(host_total), "host_route_node_coordinates_numpy": spread(host_coords),
          "host_route_sampler_create": spread(host_create), "host_route_sample": spread(host_sample)}
src.close()
dst.close()
print(json.dumps(result))
