"""Restart of a species plasma from an LTE solution on the device: tpsrhs_lte_composition and tpsrhs_species_from_lte
(RHSoperator.lteComposition / speciesFromLTE, tools/lte_restart.py) against the numpy restatement of the reference's lines
(tests/lte_restart_util.py, itself tied to the physics and to the header's host build in tests/test_lte_restart_host.py).

Bound: 1e-11, the project's device-against-host bound (parity_util.RHS_RTOL) -- per entry for the composition, per row in the
max-norm for the states.  The device's exp is not libm's, and n_e = -s + sqrt(s^2 + n_0 s) returns the rounding of the root times
A = sqrt(s^2 + n_0 s) / n_e; the inputs keep A <= 100 (asserted on the CPU side and printed), so that a few units in the last
place times A stay two orders below the bound.  The tables are the reference's own argon tables (capi.lte2d_tables())."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lte_restart_util as lu
from parity_util import RHS_RTOL, oracle_mult, rel_maxnorm
from tps_amd import capi, cases, mesh_io, restart
from tps_amd.rhs_operator import RHSoperator, TpsRhsError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "lte_restart.py")
RTOL = RHS_RTOL
assert RTOL == 1e-11

MIXTURES = {
    "ternary_ambipolar": lambda: capi.argon_ternary_physics(transport=capi.CONSTANT, ambipolar=True),
    "ternary": lambda: capi.argon_ternary_physics(two_temperature=True, transport=capi.CONSTANT, ambipolar=False),
    "six_ambipolar": lambda: capi.argon_lte_restart_physics(3, True, False),
    "six": lambda: capi.argon_lte_restart_physics(3, False, True),
}


def _dev(op, a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64).ravel(), dtype=torch.float64, device=op.device)


def _tiny_operator(ph):
    c = cases.argon_axisym(1, 1, 1, physics=ph)
    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs)


@pytest.fixture(scope="module")
def tables():
    keep = []
    return capi.lte2d_tables(), capi.lte_restart_tables(keep), keep


@pytest.fixture(scope="module")
def case270():
    """cases.argon_axisym(5, 6, 2) with the six-species ambipolar mixture: 270 nodes, its LTE rows and the restatement of them,
    computed once"""
    ph = capi.argon_lte_restart_physics(3, True, False)
    c = cases.argon_axisym(5, 6, 2, physics=ph)
    mx = lu.Mixture(ph, 3)
    t = capi.lte2d_tables()
    rows, T, rho = lu.lte_inputs(t, 270, 3, seed=21)
    U, Up, info = lu.species_from_lte(mx, t, rows)
    for a in (rows, U, Up):
        a.setflags(write=False)
    return c, mx, rows, U, Up, info


def _composition_inputs(mx, n, seed):
    """T log-uniform in [300, 19500], p log-uniform in [2e3, 2e5]; a pair whose amplification exceeds 100 is drawn again"""
    rng = np.random.Generator(np.random.MT19937(seed))
    T, p = np.zeros(0), np.zeros(0)
    while T.size < n:
        Tn = np.exp(rng.uniform(np.log(300.0), np.log(19500.0), 2 * n))
        pn = np.exp(rng.uniform(np.log(2e3), np.log(2e5), 2 * n))
        ok = lu.composition(mx, Tn, pn)[1]["amplification"] <= 100.0
        T, p = np.append(T, Tn[ok]), np.append(p, pn[ok])
    return T[:n], p[:n]


# ---- tpsrhs_lte_composition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MIXTURES))
def test_composition_against_restatement(name):
    ph = MIXTURES[name]()
    mx = lu.Mixture(ph, 3)
    op = _tiny_operator(ph)
    for n in (1, 257):  # neither a multiple of a wave; 257: two blocks
        T, p = _composition_inputs(mx, n, seed=31 + n)
        want, info = lu.composition(mx, T, p)
        assert info["amplification"].max() <= 100.0 and not info["invalid"].any()
        got = op.lteComposition(_dev(op, T), _dev(op, p)).cpu().numpy()
        assert got.shape == want.shape == (mx.ns, n)
        err = np.abs(got - want) / np.abs(want)
        print(f"{name} n={n}: amplification <= {info['amplification'].max():.3g}, max |got - want| / |want| = {err.max():.3e}")
        assert (np.abs(got - want) <= RTOL * np.abs(want)).all(), err.max()
    op.close()


def test_composition_where_the_exponential_underflows():
    ph = MIXTURES["six_ambipolar"]()
    mx = lu.Mixture(ph, 3)
    op = _tiny_operator(ph)
    p = np.array([2e3, 101325.0, 2e5])
    T = np.full(3, 150.0)
    got = op.lteComposition(_dev(op, T), _dev(op, p)).cpu().numpy()
    assert np.isfinite(got).all()
    assert (got[mx.iElectron] <= 1e-300).all() and (got[mx.iElectron] >= 0.0).all() and (got[mx.iIon1] <= 1e-300).all()
    assert np.abs(got[mx.iBackground] / (p / (lu.R * T)) - 1).max() <= 1e-14
    op.close()


# ---- tpsrhs_species_from_lte -----------------------------------------------------------------------------------------------------
def _restart(op, mx, rows, tab):
    """the LTE rows in a state whose other rows are NaN (they are not read) -> (x, up, report)"""
    x = torch.full((mx.neq, rows.shape[1]), float("nan"), dtype=torch.float64, device=op.device)
    x[:mx.nvel + 2] = torch.tensor(rows, dtype=torch.float64, device=op.device)
    rep, up = op.speciesFromLTE(x.view(-1), tab, want_primitives=True)
    return x.cpu().numpy(), up.cpu().numpy(), rep


def _check_report(rep, info):
    want = lu.report(info)
    assert (rep.num_not_converged, rep.num_invalid) == (want["num_not_converged"], want["num_invalid"])
    for k in ("max_density_change", "t_min", "t_max"):
        assert abs(getattr(rep, k) - want[k]) <= RTOL * abs(want[k]), (k, getattr(rep, k), want[k])


def test_species_from_lte_270_nodes(case270, tables):
    c, mx, rows, U, Up, info = case270
    assert info["converged"].all() and not info["invalid"].any()  # no node is left out of the comparison
    assert info["amplification"].max() <= 100.0
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    assert op.NDofs == 270 and op.num_equation == mx.neq
    x, up, rep = _restart(op, mx, rows, tables[1])
    eU, eUp = rel_maxnorm(x, lu.clamp(mx, U)), rel_maxnorm(up, Up)
    print("six species, ambipolar, 270 nodes: U", eU, "Up", eUp, "report", rep.num_not_converged, rep.num_invalid,
          rep.max_density_change, rep.t_min, rep.t_max)
    assert np.isfinite(x).all() and np.isfinite(up).all()
    assert eU.max() <= RTOL and eUp.max() <= RTOL
    _check_report(rep, info)
    # up_out = NULL: the same state
    x2 = torch.full((mx.neq, 270), float("nan"), dtype=torch.float64, device=op.device)
    x2[:5] = torch.tensor(rows, dtype=torch.float64, device=op.device)
    rep2 = op.speciesFromLTE(x2.view(-1), tables[1])
    assert np.array_equal(x2.cpu().numpy(), x) and rep2.max_density_change == rep.max_density_change
    op.close()


def test_species_from_lte_ternary_two_temperature(tables):
    ph = MIXTURES["ternary"]()
    c = cases.argon_axisym(3, 3, 1, physics=ph)
    mx = lu.Mixture(ph, 3)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    assert mx.neq == op.num_equation == 8  # rho, three momenta, rho E, ion, electron, rhoE_e
    rows, _, _ = lu.lte_inputs(tables[0], op.NDofs, 3, seed=22)
    U, Up, info = lu.species_from_lte(mx, tables[0], rows)
    assert info["converged"].all() and not info["invalid"].any() and info["amplification"].max() <= 100.0
    x, up, rep = _restart(op, mx, rows, tables[1])
    eU, eUp = rel_maxnorm(x, lu.clamp(mx, U)), rel_maxnorm(up, Up)
    print("ternary, two temperatures, not ambipolar,", op.NDofs, "nodes: U", eU, "Up", eUp)
    assert np.isfinite(x).all() and np.isfinite(up).all()
    assert eU.max() <= RTOL and eUp.max() <= RTOL
    assert np.array_equal(up[7], up[4])  # T_e = T
    _check_report(rep, info)
    op.close()


def test_unconverged_nodes_keep_their_last_iterate(case270, tables):
    c, mx, rows, _, _, _ = case270
    rows = np.array(rows)
    at = (17, 203)
    for i, (e, rho) in zip(at, lu.UNCONVERGED_STATES):
        vel = rows[1:4, i] / rows[0, i]
        rows[0, i], rows[1:4, i], rows[4, i] = rho, rho * vel, rho * e + 0.5 * rho * (vel * vel).sum()
    U, Up, info = lu.species_from_lte(mx, tables[0], rows)
    assert np.array_equal(np.where(~info["converged"])[0], at)  # checked on the CPU: these two, and only they
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x, up, rep = _restart(op, mx, rows, tables[1])
    assert rep.num_not_converged == 2 == lu.report(info)["num_not_converged"]
    assert rep.num_invalid == lu.report(info)["num_invalid"]
    want = lu.clamp(mx, U)
    node = np.abs(x[:, at] - want[:, at]) / np.maximum(np.abs(want[:, at]), 1e-300)
    print("unconverged nodes: T", up[4, at], "entry by entry", node.max(), "rows", rel_maxnorm(x, want).max())
    assert np.isfinite(x[:, at]).all() and np.isfinite(up[:, at]).all()  # values, not NaN
    assert node.max() <= RTOL and rel_maxnorm(x, want).max() <= RTOL and rel_maxnorm(up, Up).max() <= RTOL
    op.close()


def test_clamp_leaves_exact_zeros_alone(case270, tables):
    """T = 150 K: the exponentials underflow, the ion, the electrons and the levels are exactly zero, and the species clamp of
    the time loop (the same device function) changes nothing: the state is the restatement's, unclamped"""
    c, mx, _, _, _, _ = case270
    t = tables[0]
    rows, _, _ = lu.lte_inputs(t, 270, 3, seed=23, T_range=(150.0, 150.0 + 1e-9))
    U, Up, info = lu.species_from_lte(mx, t, rows)
    assert info["converged"].all() and not info["invalid"].any()
    sp = slice(5, 5 + mx.nact)
    assert (U[sp] == 0.0).all()
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x, up, rep = _restart(op, mx, rows, tables[1])
    assert (x[sp] == 0.0).all() and (up[sp] == 0.0).all()
    assert rel_maxnorm(x[:5], U[:5]).max() <= RTOL and rep.num_invalid == 0
    op.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(fn, status, text):
    with pytest.raises(TpsRhsError) as e:
        fn()
    assert e.value.status == status and text in str(e.value), str(e.value)


def test_refusals_leave_the_stream_usable(case270, tables):
    c, mx, rows, _, _, _ = case270
    t, good, _ = tables
    lib = capi.load()
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.zeros(op.Height(), dtype=torch.float64, device=op.device)
    one = torch.ones(1, dtype=torch.float64, device=op.device)
    UNS, INV = capi.ERR_UNSUPPORTED, capi.ERR_INVALID_ARGUMENT

    # the fluid
    for make, word in ((lambda: cases.dry_air_axisym(1, 1, 1), "dry air"), (lambda: cases.lte_axisym(1, 1, 1, table_dim=2), "table gas")):
        cc = make()
        o = RHSoperator(cc.mesh, cc.disc, cc.physics, cc.bcs)
        xx = torch.zeros(o.Height(), dtype=torch.float64, device=o.device)
        _refused(lambda: o.speciesFromLTE(xx, good), UNS, word)
        st = lib.tpsrhs_lte_composition(o._h, 1, C.c_void_p(one.data_ptr()), C.c_void_p(one.data_ptr()), C.c_void_p(one.data_ptr()))
        assert st == UNS and word in lib.tpsrhs_last_error().decode()
        o.close()

    # the mixture: the ion first; no +1 ion where the routine looks for it; no electron there
    def other(ph):
        cc = cases.argon_axisym(1, 1, 1, physics=ph)
        return RHSoperator(cc.mesh, cc.disc, cc.physics, cc.bcs)

    ph = capi.argon_levels_physics(3, True, two_temperature=False)
    o = other(ph)
    xx = torch.zeros(o.Height(), dtype=torch.float64, device=o.device)
    _refused(lambda: o.speciesFromLTE(xx, good), UNS, "species 0 carries a charge")
    _refused(lambda: o.lteComposition(one, one), UNS, "species 0 carries a charge")
    o.close()
    ph = capi.argon_lte_restart_physics(3, True, False)
    ph.mixture.gas_params[3 + capi.SPECIES_CHARGES * 6] = 2.0
    o = other(ph)
    _refused(lambda: o.speciesFromLTE(xx, good), UNS, "species 3 (numSpecies - 3) must be the ion of charge +1")
    o.close()
    ph = capi.argon_lte_restart_physics(3, False, False)
    ph.mixture.gas_params[4 + capi.SPECIES_CHARGES * 6] = 0.0
    o = other(ph)
    xx7 = torch.zeros(o.Height(), dtype=torch.float64, device=o.device)
    _refused(lambda: o.speciesFromLTE(xx7, good), UNS, "species 4 (numSpecies - 2) must be the electron")
    o.close()

    # the tables
    def with_table(**kw):
        d = dict(t)
        d.update(kw)
        return capi.make_lte_restart((d["thermo_T"], d["thermo_rho"], d["thermo_e"]), (d.get("R_T", d["thermo_T"]), d["thermo_rho"], d["thermo_R"]),
                                     (d["erev_e"], d["erev_rho"], d["erev_T"]))

    e = t["thermo_e"].copy()
    e[2, 7] = np.nan
    _refused(lambda: op.speciesFromLTE(x, with_table(thermo_e=e)), INV, "lte_restart.energy: non-finite value")
    rho = t["erev_rho"].copy()
    rho[3] = rho[2]
    _refused(lambda: op.speciesFromLTE(x, with_table(erev_rho=rho)), INV, "lte_restart.temperature: y must be finite and strictly increasing")
    e = t["thermo_e"].copy()
    e[10, 41] = e[10, 40]
    _refused(lambda: op.speciesFromLTE(x, with_table(thermo_e=e)), INV, "must increase with T on every density line")
    Tg = t["thermo_T"].copy()
    Tg[7] += 1.0
    _refused(lambda: op.speciesFromLTE(x, with_table(R_T=Tg)), UNS, "energy and gas_constant must share their axes")
    nul = with_table()
    nul.gas_constant.f = None
    _refused(lambda: op.speciesFromLTE(x, nul), INV, "lte_restart.gas_constant: NULL pointer")

    # NULL arguments and n < 0
    vp = C.c_void_p
    rep = capi.LteRestartReport()
    for st in (lib.tpsrhs_species_from_lte(None, C.byref(good), vp(x.data_ptr()), None, C.byref(rep)),
               lib.tpsrhs_species_from_lte(op._h, None, vp(x.data_ptr()), None, C.byref(rep)),
               lib.tpsrhs_species_from_lte(op._h, C.byref(good), None, None, C.byref(rep)),
               lib.tpsrhs_lte_composition(None, 1, vp(one.data_ptr()), vp(one.data_ptr()), vp(one.data_ptr())),
               lib.tpsrhs_lte_composition(op._h, -1, vp(one.data_ptr()), vp(one.data_ptr()), vp(one.data_ptr())),
               lib.tpsrhs_lte_composition(op._h, 1, None, vp(one.data_ptr()), vp(one.data_ptr())),
               lib.tpsrhs_lte_composition(op._h, 1, vp(one.data_ptr()), None, vp(one.data_ptr())),
               lib.tpsrhs_lte_composition(op._h, 1, vp(one.data_ptr()), vp(one.data_ptr()), None)):
        assert st == INV and lib.tpsrhs_last_error().decode().startswith("tpsrhs_")
    assert lib.tpsrhs_lte_composition(op._h, 0, vp(one.data_ptr()), vp(one.data_ptr()), vp(one.data_ptr())) == 0  # n = 0: nothing to do

    # the stream is as it was: one Mult against the oracle
    U = c.state(seed=4, amp=0.01)
    y = torch.empty_like(x)
    op.Mult(_dev(op, U), y)
    torch.cuda.synchronize()
    ref = oracle_mult(c.mesh, c.disc, c.physics, c.bcs, U)
    err = rel_maxnorm(y.cpu().numpy().reshape(U.shape), ref["y"])
    print("Mult after the refusals, rel max-norm err per equation", err)
    assert err.max() < 5 * RHS_RTOL
    op.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_restart_then_one_mult(case270, tables):
    """a SMOOTH LTE solution on the 270 nodes (5000 to 13000 K): the states of the comparisons above are drawn node by node, and
    a polynomial through such nodes is negative at some face point -- the frozen oracle refuses them ("Negative background
    density"), no Mult is defined on them"""
    c, mx, _, _, _, _ = case270
    from tps_amd.rhs_operator import node_coordinates

    w = cases._waves(node_coordinates(c.mesh, 2), 9, kmax=1)
    rows = lu.lte_rows(tables[0], 9000.0 + 4000.0 * w(), 0.255 * (1.0 + 0.3 * w()), [1.0 + 0.5 * w(), 20.0 + 2.0 * w(), 3.0 + 0.5 * w()])
    info = lu.species_from_lte(mx, tables[0], rows)[2]
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x, up, rep = _restart(op, mx, rows, tables[1])
    assert rep.num_invalid == 0 and rep.num_not_converged == 0
    xd = _dev(op, x)
    y = torch.empty_like(xd)
    op.Mult(xd, y)
    torch.cuda.synchronize()
    y = y.cpu().numpy().reshape(x.shape)
    assert np.isfinite(y).all()
    # the same operator without chemistry: the difference is the chemistry source.  The state is in the routine's equilibrium,
    # the reference's rate set (Arrhenius fits, one detailed-balance constant) is not the Saha model: no bound can be derived,
    # the ratio is printed
    ph0 = capi.argon_lte_restart_physics(3, True, False, reactions=False)
    op0 = RHSoperator(c.mesh, c.disc, ph0, c.bcs)
    y0 = torch.empty_like(xd)
    op0.Mult(xd, y0)
    torch.cuda.synchronize()
    y0 = y0.cpu().numpy().reshape(x.shape)
    hot = info["T"] > 8000.0
    sp = slice(5, 5 + mx.nact)
    ratio = np.abs(y[sp][:, hot] - y0[sp][:, hot]).max(axis=1) / np.abs(y0[sp][:, hot]).max(axis=1)
    print("chemistry source / convective and diffusive terms, species rows, T > 8000 K (", int(hot.sum()), "nodes ):", ratio)
    assert hot.sum() > 10 and np.isfinite(ratio).all()
    op.close()
    op0.close()


# ---- the command-line tool -------------------------------------------------------------------------------------------------------
def test_lte_restart_tool_end_to_end(case270, tables, tmp_path):
    c, mx, rows, _, _, info = case270
    t = tables[0]
    paths = {k: str(tmp_path / k) for k in ("tube.mesh", "lte.h5", "out.h5", "thermo.dat", "erev.npz")}
    mesh_io.write_mfem_mesh(paths["tube.mesh"], c.mesh)
    restart.write(paths["lte.h5"], restart.variable_names(3), rows, iteration=1200, time=0.375, dt=1.5e-6, order=2, dimension=2,
                  dofs_global=270)
    # the thermo file in the reference's text format (nine columns, x fastest: T, rho, -, e, -, -, R, -, c), the e_rev file as .npz
    nT, nr = len(t["thermo_T"]), len(t["thermo_rho"])
    with open(paths["thermo.dat"], "w") as f:
        f.write(f"{nT} {nr}\n")
        for j in range(nr):
            for i in range(nT):
                col = [t["thermo_T"][i], t["thermo_rho"][j], 0.0, t["thermo_e"][j, i], 0.0, 0.0, t["thermo_R"][j, i], 0.0, t["thermo_c"][j, i]]
                f.write(" ".join(repr(float(q)) for q in col) + "\n")
    np.savez(paths["erev.npz"], erev_e=t["erev_e"], erev_rho=t["erev_rho"], erev_T=t["erev_T"])
    argv = [sys.executable, TOOL, paths["tube.mesh"], paths["lte.h5"], "--order", "2", "--axisymmetric", "--thermo-table",
            paths["thermo.dat"], "--e-rev-table", paths["erev.npz"], "-o", paths["out.h5"]]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "num_not_converged 0 num_invalid 0" in r.stdout, r.stdout
    # the names and attributes the reference registers (src/M2ulPhyS.cpp:1825-1853)
    names = ["density", "rho-u", "rho-v", "rho-w", "rho-E", "rho-Y_Ar_m", "rho-Y_Ar_r", "rho-Y_Ar_p", "rho-Y_Ar.+1"]
    assert restart.variable_names(3, capi.lte_restart_species_names(c.physics), False) == names
    got, meta = restart.read(paths["out.h5"], names, 270, order=2)
    assert (meta.iteration, meta.time, meta.dt, meta.order, meta.dimension, meta.dofs_global) == (1200, 0.375, 1.5e-6, 2, 2, 270)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x, _, _ = _restart(op, mx, rows, tables[1])
    op.close()
    assert np.array_equal(got, x)  # bit for bit the direct call
    # two nodes that do not converge: exit status 1, 0 with --allow-unconverged; the file is written either way
    rows = np.array(rows)
    for i, (e, rho) in zip((17, 203), lu.UNCONVERGED_STATES):
        vel = rows[1:4, i] / rows[0, i]
        rows[0, i], rows[1:4, i], rows[4, i] = rho, rho * vel, rho * e + 0.5 * rho * (vel * vel).sum()
    restart.write(paths["lte.h5"], restart.variable_names(3), rows, order=2, dimension=2, dofs_global=270)
    import importlib.util

    spec = importlib.util.spec_from_file_location("lte_restart_tool", TOOL)  # (in this process: the child above is the tool's test)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.main(argv[2:]) == 1
    assert tool.main(argv[2:] + ["--allow-unconverged"]) == 0
    got, _ = restart.read(paths["out.h5"], names, 270, order=2)
    assert np.isfinite(got).all()
