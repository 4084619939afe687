"""The two-dimensional table gas (``flow/lte/table_dim = 2``) on the host, in a stand-alone program
(tests/lte2d_plan_main.cpp, its own main) built with plain g++: what tps_amd/csrc/operator_plan.hpp accepts and refuses, and the
temperature round trip of the closure in tps_amd/csrc/table2d.hpp that the kernels run.  The expected lines are written out
here from the rules of include/tpsrhs.h:

    a table needs nx >= 2, ny >= 2, strictly increasing finite axes, finite values, no NULL pointer; the energy must
    increase with T on every density line: INVALID_ARGUMENT otherwise
    the gas is built for the axisymmetric formulation with the Gauss-Legendre pair, without sub-grid scale model, Roe flux
    or non-reflecting patches: UNSUPPORTED otherwise (the last three with the messages of the one-dimensional gas)

Round trip: e(T, rho) is linear in T within a cell, so a Newton step taken inside the cell of the solution lands on it; what
is left is rounding, a few ulp times the condition e / (T de/dT) <= 10 of these tables.  1e-13 is the bound the
one-dimensional gas is held to in tests/test_lte.py.

The second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process;
nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "tables", "lte_tables_2d.npz")

SCOPE = "WorkingFluid::LTE_FLUID (two-dimensional tables): built for the axisymmetric formulation, Gauss-Legendre pair"
EXPECT = {
    "fixture": "ok lte 1 lte2d 1 heavy2d 1 nvel 3 neq 5",
    "disabled": "ok lte 1 lte2d 0 heavy2d 1 nvel 3 neq 5",
    "nx_1": "invalid lte2d.sound_speed: nx >= 2 and ny >= 2 (one cell at least)",
    "ny_1": "invalid lte2d.viscosity: nx >= 2 and ny >= 2 (one cell at least)",
    "x_repeats": "invalid lte2d.gas_constant: x must be finite and strictly increasing",
    "y_decreases": "invalid lte2d.temperature: y must be finite and strictly increasing",
    "nan_value": "invalid lte2d.conductivity: non-finite value",
    "inf_abscissa": "invalid lte2d.electric_conductivity: x must be finite and strictly increasing",
    "null_values": "invalid lte2d.energy: NULL pointer",
    "null_axis": "invalid lte2d.temperature: NULL pointer",
    "energy_not_increasing": "invalid lte2d.energy: e(T, rho) must increase with T on every density line",
    "thermo_grids_differ": "unsupported lte2d: energy, gas_constant and sound_speed must share their axes (the columns of one thermo file)",
    "planar_2d": "unsupported " + SCOPE,
    "3d": "unsupported " + SCOPE,
    "gauss_lobatto": "unsupported " + SCOPE,
    "sgs": "unsupported sub-grid scale models: built for dry air in 3-D",
    "roe": "unsupported flow/useRoe: Eval_Roe of the reference is 2-D, single-species, not axisymmetric (src/riemann_solver.cpp:117-206)",
    "non_reflecting": "unsupported non-reflecting inlet/outlet types: perfect gas (dry air), not axisymmetric -- the reference's "
                      "characteristic algebra (src/outletBC.cpp:573-1027)",
    # the temperature and density axes of the thermo file and the energy axis of the e_rev file are uniform; the three
    # density lines the fixture keeps of the transport file are not (0.02, 1.52, 3.0): both searches run
    "axes": "T uniform 1 rho uniform 1 e uniform 1 transport rho uniform 0",
}
ROUND_TRIP_RTOL = 1e-13


def _tables_file(tmp_path):
    """the seven tables of tpsrhs_lte2d as text: `nx ny`, x, y, f row by row (17 significant digits: exact)"""
    z = np.load(FIXTURE)
    th, rev, tr = ("thermo_T", "thermo_rho"), ("erev_e", "erev_rho"), ("trans_T", "trans_rho")
    order = [(th, "thermo_e"), (th, "thermo_R"), (th, "thermo_c"), (rev, "erev_T"), (tr, "trans_mu"), (tr, "trans_kappa"),
             (tr, "trans_sigma")]
    path = str(tmp_path / "tables.txt")
    with open(path, "w") as f:
        for (xn, yn), fn in order:
            x, y, v = z[xn], z[yn], z[fn]
            assert v.shape == (len(y), len(x))
            f.write(f"{len(x)} {len(y)}\n")
            for a in (x, y, v.ravel()):
                f.write(" ".join(repr(float(q)) for q in a) + "\n")
    return path, (len(z["thermo_T"]) - 1) * (len(z["thermo_rho"]) - 1)


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    cmd = ["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-Wno-attributes", "-Wno-unused-parameter",
                             os.path.join(HERE, "lte2d_plan_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _check(exe, tmp_path):
    tables, ncells = _tables_file(tmp_path)
    r = subprocess.run([exe, tables], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "LTE2D_PLAN DONE"
    got = dict(l.split(": ", 1) for l in lines[:-1])
    trip = got.pop("round_trip").split()
    assert got == EXPECT, {k: (got.get(k), v) for k, v in EXPECT.items() if got.get(k) != v}
    f = {trip[i]: trip[i + 1] for i in range(0, len(trip), 2)}
    print("round trip", f)
    assert int(f["cells"]) == ncells and int(f["failed"]) == 0  # every cell once; converged, and in the cell it started from
    assert float(f["worst_rel_err"]) <= ROUND_TRIP_RTOL


def test_plan_and_host_closure(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "lte2d_plan"), tmp_path)


def test_plan_and_host_closure_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "lte2d_plan_sanitize"), tmp_path)
