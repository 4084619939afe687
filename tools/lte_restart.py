"""An LTE restart file into a restart file of the species plasma: the reference's `io/restartFromLTE = True`
(src/M2ulPhyS.cpp:1842-1853, 2388-2461; test/inputs/argon.plasma.lte2noneq.ini), with the node loop on the device.
    python tools/lte_restart.py MESH LTE.h5 --order 3 --thermo-table THERMO --e-rev-table EREV -o OUT.h5
           [--levels 3] [--not-ambipolar] [--two-temperature] [--axisymmetric] [--allow-unconverged]
LTE.h5 holds density, rho-u .., rho-E of a solution of the table gas (fluid = lte_table); the species rows are absent.  THERMO and
EREV are flow/lte/thermo_table and flow/lte/e_rev_table in the reference's text format (`nx ny`, then one line per point, x
fastest: columns 0 T, 1 rho, 3 e, 6 R of the thermo file; 0 e, 1 rho, 2 T of the e_rev file), or .npz files with the arrays
thermo_T, thermo_rho, thermo_e, thermo_R and erev_e, erev_rho, erev_T.  OUT.h5 gets the rebuilt state of the argon mixture
[Ar_m, Ar_r, Ar_p][:levels], Ar.+1, E, Ar (RHSoperator.speciesFromLTE) under the names the reference registers: rho-Y_<species> for
the active species and rhoE_e with two temperatures; iteration, time, dt and order are those of LTE.h5.  The report is printed.
Exit status 1 when a node is invalid (the reference would have hit an assert), or when a node's temperature did not converge and
--allow-unconverged is not given; OUT.h5 is written all the same.  Without a HIP device: exit status 3, no traceback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXIT_REPORT, EXIT_USAGE, EXIT_NO_DEVICE = 1, 2, 3
BASES = {"legendre": 0, "lobatto": 1}


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mesh", help="mesh of the restart (MFEM mesh v1.0: quadrilaterals / hexahedra, straight-sided)")
    ap.add_argument("lte_restart", help="restart file of the table gas (HDF5)")
    ap.add_argument("--order", type=int, required=True, help="polynomial order of the restart")
    ap.add_argument("--basis", choices=sorted(BASES), default="legendre", help="Gauss-Legendre or Gauss-Lobatto nodes")
    ap.add_argument("--axisymmetric", action="store_true", help="axisymmetric formulation (three velocity components on a 2-D mesh)")
    ap.add_argument("--thermo-table", required=True, help="flow/lte/thermo_table (text or .npz)")
    ap.add_argument("--e-rev-table", required=True, help="flow/lte/e_rev_table (text or .npz)")
    ap.add_argument("-o", "--output", required=True, help="restart file of the species plasma")
    ap.add_argument("--levels", type=int, default=3, choices=(0, 1, 2, 3), help="excited levels of the neutral the mixture carries")
    ap.add_argument("--not-ambipolar", action="store_true", help="the electrons have an equation of their own")
    ap.add_argument("--two-temperature", action="store_true")
    ap.add_argument("--allow-unconverged", action="store_true", help="exit 0 although some temperatures did not converge")
    ap.add_argument("--device", type=int, default=0)
    return ap.parse_args(argv)


def read_table_file(path, columns):
    """(x, y, [f (ny, nx) per requested column]) of a table file in the reference's text format (src/table.cpp:176-208)"""
    import numpy as np

    with open(path) as f:
        nx, ny = (int(q) for q in f.readline().split()[:2])
        data = np.loadtxt(f, ndmin=2)
    if data.shape[0] != nx * ny:
        raise ValueError(f"{path}: {nx} x {ny} points announced, {data.shape[0]} lines found")
    data = data.reshape(ny, nx, -1)
    return data[0, :, 0].copy(), data[:, 0, 1].copy(), [data[:, :, c].copy() for c in columns]


def read_tables(thermo, e_rev):
    import numpy as np

    if thermo.endswith(".npz"):
        z = np.load(thermo)
        T, rho, e, R = z["thermo_T"], z["thermo_rho"], z["thermo_e"], z["thermo_R"]
    else:
        T, rho, (e, R) = read_table_file(thermo, (3, 6))
    if e_rev.endswith(".npz"):
        z = np.load(e_rev)
        ee, er, eT = z["erev_e"], z["erev_rho"], z["erev_T"]
    else:
        ee, er, (eT,) = read_table_file(e_rev, (2,))
    return (T, rho, e), (T, rho, R), (ee, er, eT)


def main(argv=None):
    args = parse(argv)
    import torch

    from tps_amd import capi, mesh_io, restart

    if not torch.cuda.is_available():
        print(f"lte_restart: {capi.STATUS.get(capi.ERR_NO_DEVICE, 'NO_DEVICE')} (status {capi.ERR_NO_DEVICE}): "
              "no HIP device is visible, and the library has no CPU path", file=sys.stderr)
        return EXIT_NO_DEVICE
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    mesh = mesh_io.read_mfem_mesh(args.mesh)
    if args.axisymmetric and mesh.dim != 2:
        print("lte_restart: the axisymmetric formulation needs a 2-D mesh", file=sys.stderr)
        return EXIT_USAGE
    nvel = 3 if args.axisymmetric else mesh.dim
    physics = capi.argon_lte_restart_physics(args.levels, not args.not_ambipolar, args.two_temperature)
    species = capi.lte_restart_species_names(physics)
    lte_names = restart.variable_names(nvel)
    names = restart.variable_names(nvel, species, args.two_temperature)
    try:
        tables = capi.make_lte_restart(*read_tables(args.thermo_table, args.e_rev_table))
    except (OSError, ValueError, KeyError) as e:
        print(f"lte_restart: {e}", file=sys.stderr)
        return EXIT_USAGE
    # walls on every boundary attribute: only the nodes and the mixture matter to the restart
    b = BASES[args.basis]
    bcs = [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]
    try:
        op = RHSoperator(mesh, capi.Disc(args.order, b, b, 1 if args.axisymmetric else 0, 0), physics, bcs, device=args.device)
    except TpsRhsError as e:
        print(f"lte_restart: {e}", file=sys.stderr)
        return EXIT_NO_DEVICE if e.status == capi.ERR_NO_DEVICE else EXIT_USAGE
    U, info = restart.read(args.lte_restart, lte_names, op.NDofs, args.order)
    x = torch.full((op.num_equation, op.NDofs), float("nan"), dtype=torch.float64, device=op.device)
    x[:nvel + 2] = torch.tensor(U, dtype=torch.float64, device=op.device)
    try:
        rep = op.speciesFromLTE(x.view(-1), tables)
    except TpsRhsError as e:
        print(f"lte_restart: {e}", file=sys.stderr)
        return EXIT_USAGE
    restart.write(args.output, names, x.cpu().numpy(), iteration=info.iteration, time=info.time, dt=info.dt, order=args.order,
                  dimension=mesh.dim, dofs_global=info.dofs_global)
    print(f"lte_restart: {op.NDofs} nodes, variables {', '.join(names)}")
    print(f"lte_restart: num_not_converged {rep.num_not_converged} num_invalid {rep.num_invalid} "
          f"max_density_change {rep.max_density_change:.6e} t_min {rep.t_min:.6f} t_max {rep.t_max:.6f}")
    op.close()
    if rep.num_invalid > 0 or (rep.num_not_converged > 0 and not args.allow_unconverged):
        return EXIT_REPORT
    return 0


if __name__ == "__main__":
    sys.exit(main())
