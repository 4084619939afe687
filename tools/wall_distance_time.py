"""Time of the wall-distance function (run on a GPU box; bench.py does not run this):
    python tools/wall_distance_time.py [--mesh cfg2|tube|both] [--pmc] [--cpu-sample 10000]
Per mesh -- cfg2: the O-grid of BASELINE configuration 2, 28 x 112 x 16 hexahedra at p = 3, 1 792 wall faces; tube: an
axisymmetric 400 x 500 (r, z) block at p = 3, 500 wall faces -- and per setting of TPSRHS_WALLDIST_CULL (1, then 0):
 - the wall-clock time of tpsrhs_wall_distance, which ends in a stream synchronise (it includes the upload of the face
   table): the median of 5 calls after 1 warm-up; pairs (nodes x faces) per second;
 - with --pmc: SQ_INSTS_VALU of the kernel from one `rocprofv3 --pmc` run of its own (a child process that makes one call
   per setting and nothing else).  That counter counts EVERY vector-ALU wave-instruction, FP64 or not: an upper bound for the
   FP64 ones.  Per pair it is counter / pairs; the least time the FP64 vector pipes could take is
   counter x 4 cycles / (1 024 SIMDs x clock), and `fp64_rate_fraction` is that over the measured time (clock: --clock-ghz);
 - the numpy restatement (tests/wall_distance_util.py) on --cpu-sample nodes of the same mesh against all its faces, on one
   CPU core, and that time extrapolated to all nodes: the RESTATEMENT's time, not the TPS binary's.
One JSON line at the end."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--mesh", default="both", choices=["cfg2", "tube", "both"])
ap.add_argument("--pmc", action="store_true", help="also count VALU instructions in a rocprofv3 run of its own")
ap.add_argument("--once", action="store_true", help="(the rocprofv3 child) one call per cull setting, no timing")
ap.add_argument("--cpu-sample", type=int, default=10000, help="nodes of the CPU restatement sample; 0: skip")
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--small", action="store_true", help="tiny meshes: a rehearsal of the tool, not a measurement")
args = ap.parse_args()


def make(name):
    from tps_amd import cases

    if name == "cfg2":
        return cases.cyl3d(*((4, 12, 3) if args.small else (28, 112, 16)), 3)
    return cases.dry_air_axisym(*((8, 10) if args.small else (400, 500)), 3)


def measure(name):
    import torch

    from tps_amd import capi
    from tps_amd.rhs_operator import RHSoperator, node_coordinates

    if not torch.cuda.is_available():
        raise SystemExit("wall_distance_time.py measures on a GPU; there is none here")
    c = make(name)
    faces = capi.wall_faces(c.mesh, c.bcs)  # the reference's rule: the viscous walls of the case
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    pairs = op.NDofs * faces.shape[0]
    res = {"mesh": name, "ndofs": op.NDofs, "faces": int(faces.shape[0]), "pairs": pairs, "order": c.disc.order}
    results = {}
    for cull in ("1", "0"):
        os.environ["TPSRHS_WALLDIST_CULL"] = cull
        d = op.wallDistance(faces=faces)  # warm-up (and, with --once, the one profiled call)
        results[cull] = d.cpu().numpy()
        if args.once:
            continue
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            op.wallDistance(faces=faces)  # returns after the stream synchronise
            times.append(time.perf_counter() - t0)
        t = statistics.median(times)
        res["cull_" + cull] = {"ms_median": round(1e3 * t, 3), "ms_min_max": [round(1e3 * min(times), 3), round(1e3 * max(times), 3)],
                               "pairs_per_s": round(pairs / t, 1)}
    res["bit_equal_with_and_without_cull"] = bool(np.array_equal(results["0"], results["1"]))
    res["max_distance"] = float(results["1"].max())
    op.close()
    if args.cpu_sample and not args.once:
        import wall_distance_util as wd

        X = node_coordinates(c.mesh, c.disc.order)
        pick = np.random.default_rng(1).choice(X.shape[1], size=min(args.cpu_sample, X.shape[1]), replace=False)
        t0 = time.perf_counter()
        ref = wd.wall_distance_np(X[:, pick], faces, chunk=256)
        t = time.perf_counter() - t0
        L = wd.bbox_diagonal(X)
        res["cpu_restatement"] = {"nodes": int(pick.size), "seconds": round(t, 3),
                                  "extrapolated_seconds_all_nodes": round(t * X.shape[1] / pick.size, 1),
                                  "note": "numpy restatement on one CPU core, not the TPS binary",
                                  "device_minus_restatement_eps_L": round(float(np.abs(results["1"][pick] - ref).max() / (wd.EPS * L)), 2)}
    return res


def count_valu(name):
    """SQ_INSTS_VALU of the kernel's two dispatches (cull on, then off), from a child process under rocprofv3"""
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--pmc", "SQ_INSTS_VALU", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--mesh", name, "--once", "--cpu-sample", "0"] + (["--small"] if args.small else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-600:]}
        rows = []
        for f in sorted(glob.glob(out + "/**/*counter_collection.csv", recursive=True)):
            rows += [x for x in csv.DictReader(open(f)) if "k_wall_distance" in x["Kernel_Name"] and x["Counter_Name"] == "SQ_INSTS_VALU"]
        rows.sort(key=lambda x: int(x.get("Dispatch_Id", 0)))
        return {("cull_1" if "true" in x["Kernel_Name"] or "ELb1E" in x["Kernel_Name"] else "cull_0"): float(x["Counter_Value"])
                for x in rows}


out = []
for name in (["cfg2", "tube"] if args.mesh == "both" else [args.mesh]):
    res = measure(name)
    if args.pmc and not args.once:
        counts = count_valu(name)
        res["SQ_INSTS_VALU"] = counts
        for key, n in counts.items():
            if key in res and isinstance(n, float):
                least = n * 4.0 / (1024 * args.clock_ghz * 1e9)
                res[key]["valu_wave_instructions_per_pair"] = round(n / res["pairs"], 4)
                res[key]["valu_lane_instructions_per_pair"] = round(64.0 * n / res["pairs"], 1)
                res[key]["fp64_rate_fraction"] = round(least / (1e-3 * res[key]["ms_median"]), 3)
    out.append(res)
if not args.once:
    import torch

    print(json.dumps({"tool": "wall_distance_time", "device": torch.cuda.get_device_name(0), "clock_ghz": args.clock_ghz,
                      "small": args.small, "results": out}))
