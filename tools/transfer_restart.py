"""One restart file into another on a different mesh, order or basis: the counterpart of the reference's
utils/pfield_interpolate (utils/pfield_interpolate.cpp:36-155), with the point location and the evaluation on the device.
    python tools/transfer_restart.py SRC.mesh SRC.h5 --src-order 2 DST.mesh --dst-order 3 -o DST.h5 [--tol T] [--fill V]
The conserved state of SRC.h5 (dataset names from tps_amd.restart.variable_names) is evaluated at the DG nodes of the target
discretisation (RHSoperator.transferFrom) and written with the source's iteration, time and dt and the target's order.  Target
nodes outside the source mesh get --fill; their number is printed, and the exit status is 1 when there are any unless
--allow-missing is given.  Without a HIP device: exit status 3 and the status text, no traceback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXIT_MISSING, EXIT_USAGE, EXIT_NO_DEVICE = 1, 2, 3
BASES = {"legendre": 0, "lobatto": 1}


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("src_mesh", help="source mesh (MFEM mesh v1.0: quadrilaterals / hexahedra, straight-sided)")
    ap.add_argument("src_restart", help="source restart file (HDF5)")
    ap.add_argument("dst_mesh", help="target mesh")
    ap.add_argument("--src-order", type=int, required=True, help="polynomial order of the source restart")
    ap.add_argument("--src-basis", choices=sorted(BASES), default="legendre", help="Gauss-Legendre or Gauss-Lobatto nodes")
    ap.add_argument("--dst-order", type=int, required=True)
    ap.add_argument("--dst-basis", choices=sorted(BASES), default="legendre")
    ap.add_argument("-o", "--output", required=True, help="target restart file")
    ap.add_argument("--species", default="", help="comma-separated species names of a plasma restart (default: dry air)")
    ap.add_argument("--two-temperature", action="store_true")
    ap.add_argument("--nvel", type=int, default=0, help="velocity components (default: the mesh dimension; 3 for axisymmetric swirl)")
    ap.add_argument("--tol", type=float, default=0.0, help="reference-coordinate tolerance of the location (<= 0: 1e-10)")
    ap.add_argument("--fill", type=float, default=0.0, help="value of target nodes outside the source mesh")
    ap.add_argument("--allow-missing", action="store_true", help="exit 0 although some target nodes were not found")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import torch

    from tps_amd import capi, mesh_io, restart

    if not torch.cuda.is_available():
        # what tpsrhs_create itself reports without a device; nothing has been read or written
        print(f"transfer_restart: {capi.STATUS.get(capi.ERR_NO_DEVICE, 'NO_DEVICE')} (status {capi.ERR_NO_DEVICE}): "
              "no HIP device is visible, and the library has no CPU path", file=sys.stderr)
        return EXIT_NO_DEVICE
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    src_mesh, dst_mesh = mesh_io.read_mfem_mesh(args.src_mesh), mesh_io.read_mfem_mesh(args.dst_mesh)
    if src_mesh.dim != dst_mesh.dim:
        print(f"transfer_restart: the meshes differ in dimension ({src_mesh.dim} and {dst_mesh.dim})", file=sys.stderr)
        return EXIT_USAGE
    dim = src_mesh.dim
    species = [s for s in args.species.split(",") if s]
    names = restart.variable_names(args.nvel or dim, species, args.two_temperature)

    def operator(mesh, order, basis):
        # dry air with walls on every boundary attribute: only geometry, order and basis matter to the transfer
        b = BASES[basis]
        bcs = [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]
        return RHSoperator(mesh, capi.Disc(order, b, b, 0, 0), capi.dry_air_physics(capi.NS), bcs, device=args.device)

    try:
        src = operator(src_mesh, args.src_order, args.src_basis)
        dst = operator(dst_mesh, args.dst_order, args.dst_basis)
    except TpsRhsError as e:
        print(f"transfer_restart: {e}", file=sys.stderr)
        return EXIT_NO_DEVICE if e.status == capi.ERR_NO_DEVICE else EXIT_USAGE
    U, info = restart.read(args.src_restart, names, src.NDofs, args.src_order)
    field = torch.tensor(U.ravel(), dtype=torch.float64, device=src.device)
    out, missing = dst.transferFrom(src, field, tol=args.tol, fill=args.fill)
    restart.write(args.output, names, out.cpu().numpy(), iteration=info.iteration, time=info.time, dt=info.dt,
                  order=args.dst_order, dimension=dim, dofs_global=dst.NDofs)
    print(f"transfer_restart: {len(names)} variables, {src.NDofs} -> {dst.NDofs} nodes, {missing} target nodes not found"
          + (f" (filled with {args.fill})" if missing else ""))
    src.close()
    dst.close()
    return EXIT_MISSING if missing and not args.allow_missing else 0


if __name__ == "__main__":
    sys.exit(main())
