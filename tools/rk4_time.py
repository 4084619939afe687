"""Wall-clock time of one step of the device time loop, and of one Mult next to it (run on a GPU box):
    python tools/rk4_time.py [--integrator forwardEuler|rk2|rk3|rk4] [--workload cfg2|argon_p3|...] [--steps N]
rk4 goes through rk4_step, the others through step (tpsrhs_step); every step returns to the host, as a driver's loop does.
    python tools/rk4_time.py --advance [--stats-interval K] ...
times the steps inside ONE advance call instead (tpsrhs_advance / tpsrhs_advance_with on a side stream, constant dt, the
captured step graph), with the running statistics sampled every K steps (0: off), and one add_sample on its own.
    python tools/rk4_time.py --advance --probe-interval 1 --monitor-interval 1 ...
adds a probe record (8 points) and / or a monitor record every K steps, with room for every record: at K = 1 the
between-step hooks run after every step, the case where their host side shows.
    python tools/rk4_time.py --mesh 4 12 3 ...
takes the O-grid cylinder with that many cells (radial, around, spanwise) instead of 28 x 112 x 16: on a small mesh a step
is bound by its launches, and the host side of the loop shows (TPSRHS_GRAPH=0: the plain launch loop)."""
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
ap.add_argument("--mesh", type=int, nargs=3, default=[28, 112, 16], metavar=("NR", "NTHETA", "NZ"), help="cells of the O-grid cylinder")
ap.add_argument("--dt", type=float, default=None, help="default: 1e-7 (cfg2), 1e-10 (the others: stiff chemistry)")
ap.add_argument("--advance", action="store_true", help="time the steps of one advance call (the device loop)")
ap.add_argument("--stats-interval", type=int, default=0, help="--advance: sample the running statistics every K steps")
ap.add_argument("--probe-interval", type=int, default=0, help="--advance: a probe record of 8 points every K steps")
ap.add_argument("--monitor-interval", type=int, default=0, help="--advance: a monitor record every K steps")
args = ap.parse_args()
sys.argv = [sys.argv[0]]

side = torch.cuda.Stream() if args.advance else None  # a capturable stream: advance replays its step graph
if side is not None:
    torch.cuda.set_stream(side)
if args.workload == "cfg2":
    c = cases.cyl3d(*args.mesh, 3, capi.NS)  # the default mesh: cases.config(2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
    U, dt = c.state(), 1e-7
else:
    import bench  # noqa: E402

    order, physics, make_bcs, make_state, _, _ = bench.workload(args.workload)
    mesh = meshgen.ogrid_cylinder_slab(*args.mesh, 0, 1)
    U, dt = make_state(node_coordinates(mesh, order), physics), 1e-10
    op = RHSoperator(mesh, capi.Disc(order, 0, 0, 0, 0), physics, make_bcs(physics), stream=side)
if args.dt is not None:
    dt = args.dt
x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
y = torch.empty_like(x)


if args.advance:
    if args.stats_interval:
        op.configureStatistics(args.stats_interval)
    if args.probe_interval:
        nodes = op.nodeCoordinates().cpu().numpy()
        sampler = op.createSampler(nodes[:, :: max(1, nodes.shape[1] // 8)][:, :8].copy())
        op.configureProbes(sampler, args.probe_interval, args.steps + 4)
    if args.monitor_interval:
        op.configureMonitor(args.monitor_interval, args.steps + 4)
    t, _, _ = op.advance(x, 0.0, dt, 4, True, integrator=args.integrator)  # allocations, the capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t, _, bad = op.advance(x, t, dt, args.steps, True, integrator=args.integrator)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / args.steps
    line = (f"{args.workload} {args.integrator} advance, statistics every {args.stats_interval or 'never'}, probes every "
            f"{args.probe_interval or 'never'}, monitor every {args.monitor_interval or 'never'}: step ms {el * 1e3:.4f}  "
            f"NaN {bad}  finite {bool(torch.isfinite(x).all())}")
    if args.probe_interval:
        iters, _, values, dropped = op.readProbes()
        line += f"  probe records {len(iters)} dropped {dropped} finite {bool((values == values).all())}"
    if args.monitor_interval:
        rec = op.readMonitor()
        line += f"  monitor records {len(rec['iters'])} dropped {rec['ndropped']}"
    if args.stats_interval:
        for _ in range(3):
            op.addSample(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            op.addSample(x)
        torch.cuda.synchronize()
        one = (time.perf_counter() - t0) / args.steps
        mean, vari, ns, _, it = op.getStatistics()
        vectors = 2 * op.num_equation + (op.num_equation + 1) + (op.num_equation + 1) + 2 * op.num_equation + 2 * vari.shape[0]
        line += (f"  one sample ms {one * 1e3:.4f}  model {vectors} vectors of {op.NDofs * 8 / 1e6:.1f} MB at 5.8 TB/s "
                 f"{vectors * op.NDofs * 8 / 5.8e12 * 1e3:.4f} ms  samples {ns}  iter {it}  finite {bool(torch.isfinite(mean).all())}")
    print(line)
    sys.exit(0)


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
