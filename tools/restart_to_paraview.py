"""A restart file as a ParaView collection: the counterpart of the reference's visualization mode (`io/restartMode` with
`M2ulPhyS::visualization`, src/M2ulPhyS.cpp:4098-4153), with the fields evaluated on the device.
    python tools/restart_to_paraview.py MESH RESTART.h5 --order 3 -o OUTDIR [--name vis] [--levels L] [--physics dry_air]
The conserved state of RESTART.h5 (dataset names from tps_amd.restart.variable_names) becomes the fields the reference
registers with its ParaViewDataCollection (tps_amd.paraview.reference_fields: dens, vel, temp, press, and for the argon
mixtures Te, the post-processing fields and sigma) on the closed lattice with --levels intervals per element direction
(default: the order, the reference's SetLevelsOfDetail(order)), written as OUTDIR/NAME/Cycle%06d/proc000000.vtu with its
data.pvtu and OUTDIR/NAME/NAME.pvd.  The cycle and the time are the restart's.  The files have not been opened in ParaView;
their layout is documented in tps_amd/paraview.py.  Without a HIP device: exit status 3 and the status text, no traceback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXIT_USAGE, EXIT_NO_DEVICE = 2, 3
BASES = {"legendre": 0, "lobatto": 1}
PHYSICS = ("dry_air", "argon_ternary", "argon_ternary_2t")


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", help="mesh (MFEM mesh v1.0: quadrilaterals / hexahedra, straight-sided)")
    ap.add_argument("restart", help="restart file (HDF5)")
    ap.add_argument("--order", type=int, required=True, help="polynomial order of the restart")
    ap.add_argument("--basis", choices=sorted(BASES), default="legendre", help="Gauss-Legendre or Gauss-Lobatto nodes")
    ap.add_argument("--physics", choices=PHYSICS, default="dry_air", help="the gas model that turns the state into fields")
    ap.add_argument("--axisymmetric", action="store_true", help="(r, z) mesh with three velocity components")
    ap.add_argument("-o", "--output", required=True, help="directory of the collection (the reference's prefix)")
    ap.add_argument("--name", default="vis", help="name of the collection")
    ap.add_argument("--levels", type=int, default=0, help="lattice intervals per direction, 1..8 (default: the order)")
    ap.add_argument("--float64", action="store_true", help="write Float64 arrays (default: Float32)")
    ap.add_argument("--ascii", action="store_true", help="write ASCII arrays (default: raw appended data)")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import numpy as np
    import torch

    from tps_amd import capi, mesh_io, paraview, restart

    if not torch.cuda.is_available():
        print(f"restart_to_paraview: {capi.STATUS.get(capi.ERR_NO_DEVICE, 'NO_DEVICE')} (status {capi.ERR_NO_DEVICE}): "
              "no HIP device is visible, and the library has no CPU path", file=sys.stderr)
        return EXIT_NO_DEVICE
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    mesh = mesh_io.read_mfem_mesh(args.mesh)
    nvel = 3 if args.axisymmetric else mesh.dim
    two_t = args.physics == "argon_ternary_2t"
    if args.physics == "dry_air":
        physics, species = capi.dry_air_physics(capi.NS), []
    else:
        physics = capi.argon_ternary_physics(two_temperature=two_t)
        species = ["Ar.+1", "E", "Ar"][:physics.mixture.num_species - 2]  # the active species a restart stores
    names = restart.variable_names(nvel, species, two_t)
    b = BASES[args.basis]
    bcs = [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]
    try:
        op = RHSoperator(mesh, capi.Disc(args.order, b, b, 1 if args.axisymmetric else 0, 0), physics, bcs, device=args.device)
    except TpsRhsError as e:
        print(f"restart_to_paraview: {e}", file=sys.stderr)
        return EXIT_NO_DEVICE if e.status == capi.ERR_NO_DEVICE else EXIT_USAGE
    U, info = restart.read(args.restart, names, op.NDofs, args.order)
    x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
    coll = paraview.ParaviewCollection(args.output, args.name, op, levels=args.levels or None,
                                       dtype=np.float64 if args.float64 else np.float32,
                                       encoding="ascii" if args.ascii else "appended")
    fields = paraview.reference_fields(op, x)
    piece = coll.save(info.iteration, info.time, fields)
    print(f"restart_to_paraview: {len(fields)} fields, {op.NDofs} nodes -> {coll.npts} lattice points (levels {coll.levels}), {piece}")
    op.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
