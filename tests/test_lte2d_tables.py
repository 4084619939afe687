"""Two-dimensional tables of the table gas (``tpsrhs_table2d``, ``flow/lte/table_dim = 2``) on the host, no GPU:

* ``tpsrhs_table2d_eval`` -- the text the kernels look their tables up with -- against a numpy restatement of the contract in
  include/tpsrhs.h (tests/lte2d_util.py), values and both derivatives on the reference's argon thermo table: interior points,
  points exactly on grid lines and corners, the last abscissa, and points outside on each of the four sides (linear
  extrapolation from the end cell, the stated departure from GSL's domain error);
* the numbers of the reference's own unit test (test/test_lte_mixture.cpp:16-30,120-140);
* the fixture script regenerates tests/golden/tables/lte_tables_2d.npz, array for array and bit for bit, where a checkout of
  the reference exists.

Tolerances: values 1e-14 relative (the two evaluations order their operations differently: a few ulp); derivatives 1e-12 of
the largest slope of the cell.  The formula is evaluated in exact rational arithmetic (lte2d_util.bilinear_exact): in float64
its d/dy cancels values of the size of the table, which costs it more than 1e-12 of a small slope."""
import importlib.util
import os

import numpy as np
import pytest

import lte2d_util as L
from tps_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))


def _thermo(name):
    t = capi.lte2d_tables()
    keep = []
    return t["thermo_T"], t["thermo_rho"], t["thermo_" + name], capi.make_table2d(t["thermo_T"], t["thermo_rho"], t["thermo_" + name], keep), keep


def _points(x, y):
    rng = np.random.default_rng(11)
    n = 400
    px, py = [rng.uniform(x[0], x[-1], n)], [rng.uniform(y[0], y[-1], n)]  # interior
    gx, gy = np.meshgrid(x, y)
    px.append(gx.ravel()), py.append(gy.ravel())                              # every node: corners, last abscissae
    px.append(np.repeat(x, 3)), py.append(rng.uniform(y[0], y[-1], 3 * len(x)))  # on the grid lines of x
    px.append(rng.uniform(x[0], x[-1], 3 * len(y))), py.append(np.repeat(y, 3))  # ... and of y
    m = 25
    for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1)):        # outside, each side and two corners
        ox = rng.uniform(x[0], x[-1], m) if sx == 0 else (x[0] - rng.uniform(1.0, 500.0, m) if sx < 0 else x[-1] + rng.uniform(1.0, 500.0, m))
        oy = rng.uniform(y[0], y[-1], m) if sy == 0 else (y[0] - rng.uniform(1e-3, 0.3, m) if sy < 0 else y[-1] + rng.uniform(1e-3, 0.3, m))
        px.append(ox), py.append(oy)
    return np.concatenate(px), np.concatenate(py)


@pytest.mark.parametrize("name", ["e", "R", "c"])
def test_table2d_eval_matches_the_formula(name):
    x, y, f, tab, keep = _thermo(name)
    px, py = _points(x, y)
    got = capi.table2d_eval(tab, px, py, 0)
    want = L.bilinear_exact(x, y, f, px, py, 0)
    assert np.abs(L.bilinear(x, y, f, px, py, 0) - want).max() <= 1e-14 * np.abs(want).max()  # (the float64 restatement the GPU tests use)
    err = np.abs(got - want) / np.abs(want)
    print(name, "value: max rel err", err.max())
    assert err.max() <= 1e-14
    for what in (1, 2):
        got = capi.table2d_eval(tab, px, py, what)
        want = L.bilinear_exact(x, y, f, px, py, what)
        slope = L.largest_slope(x, y, f, px, py, what)  # (zero where the table does not depend on the density: 0 <= 0)
        print(name, "derivative", what, ": max err / largest slope of the cell", (np.abs(got - want)[slope > 0] / slope[slope > 0]).max())
        assert np.all(np.abs(got - want) <= 1e-12 * slope)


def test_cells_follow_gsl_on_grid_lines():
    """on a grid line the point belongs to the cell on its RIGHT (x[i] <= x < x[i+1]) -- where the derivative shows it -- and
    the last abscissa to the last cell"""
    x, y, f, tab, keep = _thermo("e")
    i = 40
    ymid = np.array([0.5 * (y[3] + y[4])])
    right = (0.5 * (f[3, i + 1] + f[4, i + 1]) - 0.5 * (f[3, i] + f[4, i])) / (x[i + 1] - x[i])
    assert capi.table2d_eval(tab, x[i:i + 1], ymid, 1)[0] == pytest.approx(right, rel=1e-13)
    last = (0.5 * (f[3, -1] + f[4, -1]) - 0.5 * (f[3, -2] + f[4, -2])) / (x[-1] - x[-2])
    assert capi.table2d_eval(tab, x[-1:], ymid, 1)[0] == pytest.approx(last, rel=1e-13)


def test_table2d_eval_refuses_malformed_tables():
    x, y, f, tab, keep = _thermo("e")
    bad = capi.make_table2d(x[::-1], y, f, keep)
    with pytest.raises(RuntimeError, match="strictly increasing"):
        capi.table2d_eval(bad, x[:1], y[:1])
    with pytest.raises(RuntimeError, match="one cell"):
        capi.table2d_eval(capi.make_table2d(x[:1], y, f[:, :1], keep), x[:1], y[:1])


def test_reference_spot_values():
    """test/test_lte_mixture.cpp:16-30: R(2000 K, 0.005) = 208.1321372, R(12000 K, 0.255) = 217.82066155; :120-140:
    mu(350 K) = 2.0656339881365003e-05 (the transport file does not depend on the density)"""
    x, y, f, tab, keep = _thermo("R")
    got = capi.table2d_eval(tab, np.array([2000.0, 12000.0]), np.array([0.005, 0.255]))
    assert got[0] == pytest.approx(208.1321372, rel=1e-12)
    assert got[1] == pytest.approx(217.82066155, rel=1e-12)
    ph = capi.lte2d_physics()
    for rho in (0.02, 1.225, 3.0):
        mu = capi.table2d_eval(ph.lte2d.viscosity, np.array([350.0]), np.array([rho]))[0]
        assert mu == pytest.approx(2.0656339881365003e-05, rel=1e-12)


def test_gas_constant_depends_on_the_density():
    """the reason for the second dimension: at 12 000 K the gas constant of the argon table falls from 259 J/(kg K) at
    0.05 kg/m^3 to 211 at 2.3"""
    x, y, f, tab, keep = _thermo("R")
    got = capi.table2d_eval(tab, np.array([12000.0, 12000.0]), np.array([0.05, 2.3]))
    assert round(got[0]) == 259 and round(got[1]) == 211


def test_newton_restatement_converges_everywhere():
    """the restated Newton iteration (what the GPU tests compare the device with) on 20 000 random states inside both
    tables: all converge, in at most 3 iterations, and return the temperature they were built from"""
    t = capi.lte2d_tables()
    rng = np.random.default_rng(5)
    rho, T = rng.uniform(0.02, 2.4, 20000), rng.uniform(200.0, 19500.0, 20000)
    e = L.bilinear(t["thermo_T"], t["thermo_rho"], t["thermo_e"], T, rho)
    back, it, conv = L.temperature(t, e, rho)
    assert conv.all() and it.max() <= 3
    assert np.abs(back - T).max() / T.min() < 1e-12 and (np.abs(back - T) / T).max() < 1e-14


def test_fixture_script_regenerates_the_fixture():
    ref = os.environ.get("TPS_REFERENCE_DIR", "/root/reference")
    if not os.path.exists(os.path.join(ref, "test", "inputs", "argon_lte_thermo_table.dat")):
        pytest.skip("no checkout of the reference here")
    spec = importlib.util.spec_from_file_location("make_lte_tables_2d", os.path.join(HERE, "golden", "tables", "make_lte_tables_2d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh = mod.tables()
    with np.load(os.path.join(HERE, "golden", "tables", "lte_tables_2d.npz")) as z:
        assert sorted(z.files) == sorted(fresh)
        for k in z.files:
            assert z[k].dtype == np.float64 and z[k].shape == fresh[k].shape and z[k].tobytes() == fresh[k].tobytes(), k
    assert os.path.getsize(os.path.join(HERE, "golden", "tables", "lte_tables_2d.npz")) < 316 * 1024


def test_one_dimensional_slices_are_lines_of_the_fixture():
    """the 1-D fixture lte_tables.npz is two density lines of the same thermo file"""
    t, one = capi.lte2d_tables(), capi.lte_tables()
    for j, tag in ((0, "rho0p005"), (1, "rho0p255")):
        s = one["thermo_" + tag]
        assert np.array_equal(s[:, 0], t["thermo_T"]) and float(one["density_" + tag]) == t["thermo_rho"][j]
        assert np.array_equal(s[:, 1], t["thermo_e"][j]) and np.array_equal(s[:, 2], t["thermo_R"][j]) and np.array_equal(s[:, 3], t["thermo_c"][j])
