"""The table gas with two-dimensional (T, rho) tables (``flow/lte/table_dim = 2``, ``tpsrhs_physics::lte2d``) on the device.

The frozen oracle has one-dimensional tables only, so the assembled ``Mult`` is pinned where the two gases coincide:

* point closures and the conductivity side output at strongly varying densities against a numpy restatement of the
  reference's Newton iteration and the bilinear look-ups (tests/lte2d_util.py), rel 1e-12;
* ``Mult`` at an exactly uniform density, where the bilinear tables ARE linear tables in T -- the blend
  ``(1-u) f_j + u f_{j+1}`` of two density lines, which the oracle gets through the existing ``lte`` field;
* ``Mult`` at a density varying by +-60 % on tables that do not depend on the density (the 0.255 line copied to all
  lines): every cell search and every pair of offsets at every call site, with the result of the one-dimensional gas;
* two densities in one state, each half against the oracle on its own blend, away from the interface;
* refusals.

What stays unpinned: a face whose two sides have different densities, as an assembled ``Mult``."""
import ctypes as C

import numpy as np
import pytest

import lte2d_util as L
from parity_util import RHS_RTOL, rel_maxnorm
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu


def _cons(t, prim):
    """(5, n) conserved states from primitives (rho, u, v, w, T): rho e(T, rho) + kinetic energy"""
    rho, T = prim[0], prim[4]
    U = prim.copy()
    U[1:4] *= rho
    U[4] = rho * L.bilinear(t["thermo_T"], t["thermo_rho"], t["thermo_e"], T, rho) + 0.5 * rho * (prim[1:4] ** 2).sum(axis=0)
    return U


# ---- 5. point closures, varying density -------------------------------------------------------------------------------------
def test_point_closures_at_varying_density():
    import torch
    from tps_amd.rhs_operator import RHSoperator

    t = capi.lte2d_tables()
    rng = np.random.default_rng(7)
    n = 257
    prim = np.stack([rng.uniform(0.02, 2.4, n), rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-30, 30, n),
                     rng.uniform(200.0, 19500.0, n)])
    prim[:, 0] = [0.005, 0.0, 0.0, 0.0, 2000.0]    # the reference's spot checks (test/test_lte_mixture.cpp:16-30)
    prim[:, 1] = [0.255, 0.0, 0.0, 0.0, 12000.0]
    U = _cons(t, prim)
    rho = U[0]
    T, it, conv = L.temperature(t, (U[4] - 0.5 * (U[1:4] ** 2).sum(axis=0) / rho) / rho, rho)
    assert conv.all()  # the restated reference leaves no state out, so the comparison leaves none out
    th = (t["thermo_T"], t["thermo_rho"])
    p_ref = rho * L.bilinear(*th, t["thermo_R"], T, rho) * T
    c_ref = L.bilinear(*th, t["thermo_c"], T, rho)
    want = {0: np.concatenate([rho[None], U[1:4] / rho, T[None]]), 1: p_ref, 2: c_ref,
            3: np.sqrt((U[1:4] ** 2).sum(axis=0)) / rho + c_ref}
    c = cases.lte_axisym(3, 3, 1, table_dim=2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    lib = capi.load()
    xd = torch.tensor(np.ascontiguousarray(U), device="cuda")
    for quantity, ref in want.items():
        out = torch.empty(ref.size, dtype=torch.float64, device="cuda")
        st = lib.tpsrhs_eval_pointwise(op._h, quantity, n, C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()))
        assert st == 0, lib.tpsrhs_last_error().decode()
        got = out.cpu().numpy().reshape(ref.shape)
        err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("quantity", quantity, "max rel err", err.max())
        assert err.max() <= 1e-12
        if quantity == 1:
            assert got[0] == pytest.approx(0.005 * 208.1321372 * 2000.0, rel=1e-12)
            assert got[1] == pytest.approx(0.255 * 217.82066155 * 12000.0, rel=1e-12)
    op.close()


# ---- 6. conductivity side output, varying density -----------------------------------------------------------------------
def test_plasma_conductivity_at_varying_density():
    import torch
    from tps_amd.rhs_operator import RHSoperator

    t = capi.lte2d_tables()
    c = cases.lte_axisym(5, 6, 3, table_dim=2, transport="synthetic")
    X = node_coordinates(c.mesh, 3)
    U = cases.lte_state(X, c.physics, seed=8, amp=0.6, rho0=1.2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    got = op.getPlasmaConductivity(x).cpu().numpy()
    op.close()
    rho = U[0]
    T, _, conv = L.temperature(t, (U[4] - 0.5 * (U[1:4] ** 2).sum(axis=0) / rho) / rho, rho)
    assert conv.all()
    _, _, sigma = capi.synthetic_transport_2d(t["trans_T"], t["trans_rho"], (t["trans_mu"], t["trans_kappa"]))  # SYNTHETIC
    raw = L.bilinear(t["trans_T"], t["trans_rho"], sigma, T, rho)
    assert (raw < 1.0).sum() > 10 and (raw > 1.0).sum() > 10  # both branches of the floor
    assert rho.max() / rho.min() > 3.0
    want = np.maximum(raw, 1.0)
    err = np.abs(got - want) / want
    print("sigma: max rel err", err.max(), "floored", (raw < 1.0).sum(), "of", raw.size)
    assert err.max() <= 1e-12


# ---- 7. Mult against the unchanged oracle, uniform density --------------------------------------------------------------
def _wall_distance(c):
    X = node_coordinates(c.mesh, c.disc.order)
    return np.ascontiguousarray(X[0].max() - X[0])


def _pair(rho, nr, nz, order, eq, wall, r_in=0.0, warp=0.0, radiation=False, transport="reference", tweak=None):
    """the case with the two-dimensional gas and the physics of the one-dimensional gas it is at the uniform density rho"""
    c = cases.lte_axisym(nr, nz, order, eq, wall, r_in=r_in, warp=warp, radiation=radiation, table_dim=2, transport=transport)
    c.bcs[0] = capi.make_bc(1, capi.INLET, capi.SUB_DENS_VEL, [rho, 0.0, 20.0, 2.0])  # the ghost state of the inlet has ITS density
    ph1 = L.blended_1d_physics(rho, eq, radiation, transport)
    for ph in (c.physics, ph1):
        if tweak:
            tweak(ph)
    return c, ph1


def _compare(c, ph1, U, distance=None, ml=None, keep=None, speed=True):
    """one Mult of the device operator (c.physics) against the oracle (ph1), as _compare of tests/test_lte.py: Up at 1e-12,
    gradUp, y and the largest characteristic speed at RHS_RTOL; `keep`: the nodes that are compared (default all)"""
    import torch
    from oracle_lib import Oracle
    from tps_amd.rhs_operator import RHSoperator

    o = Oracle(c.mesh, c.disc, ph1, c.bcs)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    if distance is not None:
        o.set_mixing_length(distance, **ml)
        op.setMixingLength(torch.tensor(distance, dtype=torch.float64, device=op.device), **ml)
    ref = o.mult(U)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    op.Mult(x, y, want_max_char_speed=True)
    torch.cuda.synchronize()
    got = y.cpu().numpy().reshape(U.shape)
    sel = slice(None) if keep is None else keep
    up, up_ref = op.getPrimitives().cpu().numpy().reshape(5, -1), np.asarray(o.primitives()).reshape(5, -1)
    g, g_ref = op.getGradients().cpu().numpy().reshape(10, -1), np.asarray(o.gradients()).reshape(10, -1)
    e_up = rel_maxnorm(up[:, sel], up_ref[:, sel])
    e_g = np.abs(g[:, sel] - g_ref[:, sel]).max() / np.abs(g_ref[:, sel]).max()
    e_y = rel_maxnorm(got[:, sel], ref[:, sel])
    print("rel err Up", e_up.max(), "gradUp", e_g, "y", e_y)
    assert e_up.max() <= 1e-12
    assert e_g < RHS_RTOL
    assert e_y.max() < RHS_RTOL
    if speed:
        assert abs(op.max_char_speed - o.max_char_speed) < RHS_RTOL * o.max_char_speed
    op.close()
    return ref, got


def _uniform_state(c, rho, seed):
    X = node_coordinates(c.mesh, c.disc.order)
    return cases.lte_state(X, c.physics, seed=seed, rho0=np.full(X.shape[1], rho))


def _torch_combination(ph):
    vs = ph.visc_sponge
    vs.enabled, vs.width, vs.ratio = 1, 0.02, 20.0  # test/inputs/plasma.lte1d.ini:52-58
    vs.normal[1], vs.point[1] = 1.0, 0.15


@pytest.mark.parametrize("rho", [0.255, 0.4])  # a grid line of the density axis; between two lines
@pytest.mark.parametrize("name", ["p3_isoth_radiation", "p2_adiab_warped", "p1_euler_inviscid", "p4_ns", "torch_combination",
                                  "p3_synthetic_transport"])
def test_mult_at_uniform_density(name, rho):
    distance = ml = None
    if name == "p3_isoth_radiation":
        c, ph1 = _pair(rho, 6, 9, 3, capi.NS, capi.VISC_ISOTH, radiation=True)
    elif name == "p2_adiab_warped":
        c, ph1 = _pair(rho, 6, 9, 2, capi.NS, capi.VISC_ADIAB, r_in=0.01, warp=0.06)
    elif name == "p1_euler_inviscid":
        c, ph1 = _pair(rho, 6, 9, 1, capi.EULER, capi.INV, r_in=0.02, warp=0.06)
    elif name == "p4_ns":
        c, ph1 = _pair(rho, 6, 9, 4, capi.NS, capi.INV)
    elif name == "torch_combination":  # test/inputs/plasma.lte1d.ini: useBCinGrad, mixing length, viscosity multiplier function
        c, ph1 = _pair(rho, 6, 9, 3, capi.NS, capi.VISC_ISOTH, radiation=True, warp=0.05, tweak=_torch_combination)
        c.disc.use_bc_in_grad = 1
        distance, ml = _wall_distance(c), dict(max_mixing_length=0.01, pr_ratio=0.0, bulk_multiplier=0.0)
    else:
        c, ph1 = _pair(rho, 6, 9, 3, capi.NS, capi.VISC_ISOTH, transport="synthetic")
    _compare(c, ph1, _uniform_state(c, rho, seed=3 + c.disc.order), distance=distance, ml=ml)


@pytest.mark.parametrize("rho", [0.255, 0.4])
def test_rk4_step_at_uniform_density(rho):
    """One tpsrhs_rk4_step (four Mults and the update on the device) against the oracle's, at RHS_RTOL.  Only the first stage
    sees a uniform density: the later ones see it moved by dt * d(rho)/dt, and there the two gases differ by that much of
    the density dependence of the tables -- a difference of the two MODELS, not of the code, which falls with dt^2.  For
    this state, far from steady, it is 1.3e-5 of the radial momentum at dt = 2e-8 (measured on the MI355X; the density moves
    by 6e-5 per step, the radial momentum by five times its size); dt = 2e-12 puts it at 1e-13, below the tolerance,
    and the step still moves every row by far more than the tolerance (asserted).  Time steps of a useful size are compared
    in test_advance_on_density_free_tables, where the two models agree at any density."""
    import torch
    from oracle_lib import Oracle
    from tps_amd.rhs_operator import RHSoperator

    c, ph1 = _pair(rho, 5, 7, 2, capi.NS, capi.VISC_ISOTH)
    U = _uniform_state(c, rho, seed=9)
    o = Oracle(c.mesh, c.disc, ph1, c.bcs)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    dt = 2.0e-12
    ref, _, _, _ = o.rk4_step(np.ascontiguousarray(U).copy(), 0.0, dt)
    op.rk4_step(x, 0.0, dt)
    torch.cuda.synchronize()
    got = x.cpu().numpy().reshape(U.shape)
    err = rel_maxnorm(got, ref.reshape(U.shape))
    change = rel_maxnorm(got, U)
    print("rel err after one RK4 step", err, "change of the state", change)
    assert err.max() < RHS_RTOL
    assert change.min() > 1e2 * RHS_RTOL  # the step moved every row by far more than the tolerance
    op.close()


def test_advance_on_density_free_tables():
    """three RK4 steps of the device time loop (tpsrhs_advance, constant dt) at a strongly varying density on tables without
    density dependence (_flatten below), where the gas IS the one-dimensional one whatever the density does: against three
    steps of the oracle at RHS_RTOL"""
    import torch
    from oracle_lib import Oracle
    from tps_amd.rhs_operator import RHSoperator

    c = cases.lte_axisym(5, 7, 2, capi.NS, capi.VISC_ISOTH, table_dim=2)
    _flatten(c.physics)
    ph1 = capi.lte_physics(capi.NS, "rho0p255")
    U = cases.lte_state(node_coordinates(c.mesh, 2), c.physics, seed=9, amp=0.6, rho0=1.2)
    o = Oracle(c.mesh, c.disc, ph1, c.bcs)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    ref = np.ascontiguousarray(U).copy()
    dt, t = 2.0e-8, 0.0
    for _ in range(3):
        ref, t, _, _ = o.rk4_step(ref, t, dt)
    op.advance(x, 0.0, dt, 3, constant_dt=True)
    torch.cuda.synchronize()
    got = x.cpu().numpy().reshape(U.shape)
    err = rel_maxnorm(got, ref.reshape(U.shape))
    print("rel err after 3 RK4 steps", err, "change of the state", rel_maxnorm(got, U))
    assert err.max() < RHS_RTOL
    op.close()


# ---- 8. strongly varying density on tables without density dependence ------------------------------------------------------
def _flatten(ph):
    """every density line of the thermodynamic tables and of T(e, rho) replaced by the 0.255 line (line 1)"""
    t = capi.lte2d_tables()
    l2 = ph.lte2d
    for field, axes, name in (("energy", ("thermo_T", "thermo_rho"), "thermo_e"), ("gas_constant", ("thermo_T", "thermo_rho"), "thermo_R"),
                              ("sound_speed", ("thermo_T", "thermo_rho"), "thermo_c"), ("temperature", ("erev_e", "erev_rho"), "erev_T")):
        f = np.repeat(t[name][1:2], t[name].shape[0], axis=0)
        setattr(l2, field, capi.make_table2d(t[axes[0]], t[axes[1]], f, ph._keep))


@pytest.mark.parametrize("order,eq,wall,radiation", [(3, capi.NS, capi.VISC_ISOTH, True), (3, capi.NS, capi.VISC_ADIAB, False),
                                                     (4, capi.NS, capi.INV, False), (3, capi.EULER, capi.INV, False)])
def test_mult_at_varying_density_on_density_free_tables(order, eq, wall, radiation):
    """rho = 1.2 (1 +- 0.6) spans six cells of the density axis of the thermodynamic tables and both cells of the
    transport tables' (three lines, not uniformly spaced: the bisection).  (p >= 3: on this 6 x 9 mesh a density wave of that
    size is not resolved at p = 1, 2 -- the states extrapolated to the faces leave the tables, and the oracle, like the
    reference, asserts T > 0.)"""
    c = cases.lte_axisym(6, 9, order, eq, wall, radiation=radiation, warp=0.05, table_dim=2)
    _flatten(c.physics)
    ph1 = capi.lte_physics(eq, "rho0p255", radiation=radiation)
    X = node_coordinates(c.mesh, order)
    U = cases.lte_state(X, c.physics, seed=5, amp=0.6, rho0=1.2)
    assert U[0].min() < 0.5 and U[0].max() > 1.9
    _compare(c, ph1, U)


# ---- 9. two densities in one state -------------------------------------------------------------------------------------------
def test_two_densities_in_one_state():
    """rho = 0.255 in the lower half of the tube, 1.2 in the upper half; T and the velocity vary smoothly.  y of an element
    reads its neighbours' gradients, which read theirs: the elements at least two layers from the interface see the other
    half not at all, and equal the oracle's on the blend of their own density."""
    nr, nz, order, length = 5, 8, 2, 0.25
    lo, hi = 0.255, 1.2
    c, ph_lo = _pair(lo, nr, nz, order, capi.NS, capi.VISC_ISOTH)  # (the tube of cases.lte_axisym is `length` long)
    ph_hi = L.blended_1d_physics(hi, capi.NS)
    X = node_coordinates(c.mesh, order)
    npe = (order + 1) ** 2
    zc = X[1].reshape(-1, npe).mean(axis=1)  # centroid of every element
    layer = np.floor(zc / (length / nz)).astype(int)
    assert layer.min() == 0 and layer.max() == nz - 1
    rho = np.where(X[1] < 0.5 * length, lo, hi)
    U = cases.lte_state(X, c.physics, seed=4, rho0=rho)
    far_lo, far_hi = layer <= nz // 2 - 3, layer >= nz // 2 + 2
    assert (far_lo.sum() + far_hi.sum()) * 3 >= layer.size and far_lo.any() and far_hi.any()
    for ph1, far in ((ph_lo, far_lo), (ph_hi, far_hi)):
        _compare(c, ph1, U, keep=np.repeat(far, npe), speed=False)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_and_status_texts():
    import torch
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    scope = "two-dimensional tables.*axisymmetric formulation, Gauss-Legendre pair"
    c = cases.lte_axisym(3, 3, 2, table_dim=2)
    with pytest.raises(TpsRhsError, match="TPSRHS_ERR_UNSUPPORTED.*" + scope):  # planar
        RHSoperator(c.mesh, capi.Disc(2, 0, 0, 0, 0), c.physics, c.bcs)
    with pytest.raises(TpsRhsError, match="TPSRHS_ERR_UNSUPPORTED.*" + scope):  # 3-D
        RHSoperator(meshgen.box_hex(3, 3, 3), capi.Disc(2, 0, 0, 0, 0), c.physics, [])
    with pytest.raises(TpsRhsError, match="TPSRHS_ERR_UNSUPPORTED.*" + scope):  # Gauss-Lobatto pair
        RHSoperator(c.mesh, capi.Disc(2, 1, 1, 1, 0), c.physics, c.bcs)
    c.physics.sgs.model_type = capi.SGS_SMAGORINSKY
    with pytest.raises(TpsRhsError, match="TPSRHS_ERR_UNSUPPORTED.*sub-grid scale models"):
        RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    c.physics.sgs.model_type = 0
    t = capi.lte2d_tables()
    bad = t["thermo_c"].copy()
    bad[3, 17] = np.nan
    c.physics.lte2d.sound_speed = capi.make_table2d(t["thermo_T"], t["thermo_rho"], bad, c.physics._keep)
    with pytest.raises(TpsRhsError, match="TPSRHS_ERR_INVALID_ARGUMENT.*lte2d.sound_speed: non-finite value"):
        RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    c.physics.lte2d.sound_speed = capi.make_table2d(t["thermo_T"], t["thermo_rho"], t["thermo_c"], c.physics._keep)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(c.state(seed=1)).ravel(), dtype=torch.float64, device=op.device)
    out = torch.empty(64 * op.NDofs, dtype=torch.float64, device=op.device)
    lib = capi.load()
    st = lib.tpsrhs_visualization_fields(op._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
    assert lib.tpsrhs_status_string(st).decode() == "TPSRHS_ERR_UNSUPPORTED"
    assert "not for the table gas" in lib.tpsrhs_last_error().decode()
    op.close()
