"""tpsrhs_get_flux / tpsrhs_surface_loads on the device (tps_amd/csrc/flux_fields.hpp).

(a) Parity with the oracle's POINT closures: the device's own clamped x and getGradients() are read back and fed node by
    node to Oracle.convective_flux / viscous_flux / viscous_flux_at / viscous_flux_dist, so that only the closure differs
    between the two sides.  Bound: per row (direction, equation) rel_maxnorm <= RHS_RTOL (1e-11, tests/parity_util.py), the
    bound tests/test_gpu_reference_point.py holds the transport rows of these closures to; a row the oracle has identically
    zero must be exactly 0.0.
(b) Every built plasma instantiation of the pass once, same comparison, p = 1 on the smallest mesh of its geometry.
(c) Known answers without the oracle: Couette flow and a fluid at rest in a pressure gradient, the six faces of the centre
    element of a 3 x 3 x 3 box.
(d) Composition and hygiene.

With TPSRHS_FLUX_FIELDS_RATIOS=<file> the worst achieved error / bound per case of (a) is written there."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import surface_util as sfu
from parity_util import RHS_RTOL
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PARTS = ("convective", "viscous", "total")
_RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    path = os.environ.get("TPSRHS_FLUX_FIELDS_RATIOS")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("worst per-row rel_maxnorm of tpsrhs_get_flux against the oracle's point closures, as a fraction of RHS_RTOL = 1e-11\n")
            for name, r in _RATIOS:
                f.write(f"{name:70s} " + "  ".join(f"{p} {v:.3e}" for p, v in zip(PARTS, r)) + "\n")


def _operator(c, **kw):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs, **kw)


def _dev(op, a):
    import torch

    return torch.tensor(np.ascontiguousarray(a).ravel(), dtype=torch.float64, device=op.device)


def _nactive(c):
    if c.physics.working_fluid != capi.USER_DEFINED:
        return 0
    mx = c.physics.mixture
    return mx.num_species - 2 if mx.ambipolar else mx.num_species - 1


def _clamped(c, U, nvel):
    Uc = np.array(U, dtype=np.float64)
    na = _nactive(c)
    Uc[nvel + 2:nvel + 2 + na] = np.maximum(Uc[nvel + 2:nvel + 2 + na], 0.0)
    return Uc


def _oracle_parts(o, Uc, G, axisym, X, mode="plain", delta=None, dist=None):
    """C, V [dim, neq, n] of the oracle's point closures at the device's own state and gradient"""
    from oracle_lib import lib

    dim, neq, n = G.shape
    Cf, Vf = np.zeros((dim, neq, n)), np.zeros((dim, neq, n))
    L = lib()
    dp = C.POINTER(C.c_double)
    L.tpsoracle_point_viscous_flux_dist.argtypes = [C.c_void_p, dp, dp, C.c_double, C.c_double, dp]
    x3 = np.zeros(3)
    for i in range(n):
        s, g = np.ascontiguousarray(Uc[:, i]), np.ascontiguousarray(G[:, :, i])
        radius = float(X[0, i]) if axisym else -1.0
        Cf[:, :, i] = o.convective_flux(s)
        if mode == "plain":
            Vf[:, :, i] = o.viscous_flux(s, g, radius)
        elif mode == "at":
            x3[:X.shape[0]] = X[:, i]
            Vf[:, :, i] = o.viscous_flux_at(s, g, x3, float(delta[i])).reshape(dim, neq)
        else:
            out = np.zeros(neq * dim)
            L.tpsoracle_point_viscous_flux_dist(o.h, s.ctypes.data_as(dp), g.ctypes.data_as(dp), radius, float(dist[i]), out.ctypes.data_as(dp))
            Vf[:, :, i] = out.reshape(dim, neq)
    return Cf, Vf


def _row_errors(got, ref):
    """per row (d, eq): max |got - ref| / max |ref|; a row that is identically zero in ref must be exactly zero in got"""
    g, r = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    den = np.abs(r).max(axis=1)
    zero = den == 0.0
    assert np.all(g[zero] == 0.0), "a row the oracle has identically zero is not exactly 0.0"
    return np.abs(g - r).max(axis=1)[~zero] / den[~zero]


def _compare(name, c, U, mode="plain", distance=None, ml=None, euler=False, oracle_physics=None):
    """getFlux of the three parts against the oracle's closures; -> the device tensors.  oracle_physics: what the oracle is
    created with where it cannot take the operator's own (the two-dimensional table gas)"""
    import torch

    from oracle_lib import Oracle

    order, basis, axisym = c.disc.order, c.disc.basis_type, bool(c.disc.axisymmetric)
    op = _operator(c)
    o = Oracle(c.mesh, c.disc, oracle_physics or c.physics, c.bcs)
    if distance is not None:
        o.set_mixing_length(distance, **ml)
        op.setMixingLength(_dev(op, distance), **ml)
    x = _dev(op, U)
    nvel = 3 if (axisym or c.mesh.dim == 3) else 2
    got = {p: op.getFlux(x, p).cpu().numpy() for p in PARTS}
    G = op.getGradients().cpu().numpy()
    torch.cuda.synchronize()
    n = op.NDofs
    assert n > 256 and n % 256 != 0, "at least two blocks, the last one partly filled"
    assert got["total"].shape == (c.mesh.dim, U.shape[0], n)
    op.close()
    X = node_coordinates(c.mesh, order, basis)
    delta = np.repeat(o.element_sizes(), n // c.mesh.num_elements) if mode == "at" else None
    Cf, Vf = _oracle_parts(o, _clamped(c, U, nvel), G, axisym, X, mode, delta, distance)
    worst = []
    for p, ref in (("convective", Cf), ("viscous", Vf), ("total", Cf - Vf)):
        assert np.isfinite(got[p]).all()
        if p == "viscous" and euler:
            assert not got[p].any(), "VISCOUS is all zeros for Euler"
            worst.append(0.0)
            continue
        err = _row_errors(got[p], ref)
        print(f"{name}: {p}: worst row rel_maxnorm {err.max():.3e} (bound {RHS_RTOL:.0e}); rows above the bound: "
              f"{int((err > RHS_RTOL).sum())} of {err.size}")
        worst.append(float(err.max()) / RHS_RTOL)
    _RATIOS.append((name, worst))
    assert max(worst) <= 1.0, (name, dict(zip(PARTS, worst)))
    if euler:
        assert np.array_equal(got["total"], got["convective"])
    else:
        assert np.abs(Vf).max() > 0.0
    return got


def _boost(ph, third_order=False):
    """transport multiplied as tests/test_gpu_parity.py does it, so that the viscous terms are no rounding noise of the sum"""
    ph.gas_transport.multiply = 1
    for k in range(4):
        ph.gas_transport.flux_trns_multiplier[k] = 30.0
    if third_order:
        ph.gas_transport.flux_trns_multiplier[3] = 1.0
    ph.gas_transport.diff_mult = ph.gas_transport.mobil_mult = 30.0
    return ph


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
def test_dry_air_ns_3d():
    c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)  # 3 888 nodes
    c.physics.dry_air.visc_mult = 300.0
    _compare("dry air NS 3-D p2", c, c.state(seed=1))


def test_dry_air_euler_3d():
    c = cases.cyl3d(4, 12, 3, 2, capi.EULER)
    _compare("dry air Euler 3-D p2", c, c.state(seed=2), euler=True)


def test_dry_air_sigma_model_and_sponge_3d():
    """The state carries a linear velocity field u = G0 x whose gradient has three well separated singular values.  The
    sigma model takes the singular values of grad u through acos(r) / 3 (src/fluxes.cpp:584-587, physics_dryair.hpp::
    sgs_sigma), whose error amplification is 1 / sqrt(1 - r^2): where two singular values nearly coincide (the smooth
    sinusoidal states of tps_amd.cases have such nodes) one ulp of acos or cos is worth 1e-9 of the eddy viscosity, on
    either side, and no comparison of two correctly rounded implementations holds 1e-11 there.  Measured with
    c.state(seed=3): viscous rows 3.6e-10 at amp = 0.05, 1.4e-9 at amp = 0.1, the other rows below 1e-15."""
    c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
    ph = c.physics
    ph.dry_air.visc_mult = 300.0
    ph.sgs.model_type = capi.SGS_SIGMA
    vs = ph.visc_sponge
    vs.enabled, vs.width, vs.ratio = 1, 0.3, 12.0
    vs.normal[0], vs.normal[1], vs.point[0], vs.point[1] = 1.0, 0.4, 0.5, 0.2
    X = node_coordinates(c.mesh, 2, 0)
    U = c.state(seed=3, amp=0.01)
    G0 = np.array([[1.0, 0.5, 0.0], [0.2, -0.3, 0.1], [0.05, 0.15, 0.6]])  # singular values 1.13, 0.61, 0.37
    assert np.diff(np.linalg.svd(G0, compute_uv=False)).max() < -0.2
    vel = U[1:4] / U[0] + (40.0 / (X.max(axis=1) - X.min(axis=1)).max()) * (G0 @ (X - X.mean(axis=1, keepdims=True)))
    p = 0.4 * (U[4] - 0.5 * (U[1:4] ** 2).sum(axis=0) / U[0])
    U[1:4] = U[0] * vel
    U[4] = p / 0.4 + 0.5 * U[0] * (vel ** 2).sum(axis=0)
    _compare("dry air sigma + sponge 3-D p2", c, U, mode="at")


def test_dry_air_2d_gauss_lobatto():
    attrs = {(0, 0): 1, (0, 1): 2, (1, 0): 3, (1, 1): 3}
    mesh = meshgen.scramble_orientations(meshgen.box_quad(5, 7, lengths=(1.0, 0.7), periodic=(False, False), bdr_attr=attrs, warp=0.06), 5)
    bcs = [capi.make_bc(1, capi.INLET, capi.SUB_DENS_VEL, [1.2, 20.0, 0.0, 0.0]), capi.make_bc(2, capi.OUTLET, capi.SUB_P, [101300.0]),
           capi.make_bc(3, capi.WALL, capi.VISC_ADIAB)]
    c = cases.Case("box2d", mesh, capi.Disc(3, 1, 1, 0, 0), capi.dry_air_physics(capi.NS, visc_mult=300.0, bulk_visc_mult=0.4), bcs)
    _compare("dry air 2-D Gauss-Lobatto p3", c, cases.dry_air_state(node_coordinates(mesh, 3, 1), seed=4, nvel=2))


def test_dry_air_axisym_with_a_mixing_length():
    c = cases.dry_air_axisym(5, 7, 3, r_in=0.0)
    c.physics.dry_air.visc_mult = 300.0
    X = node_coordinates(c.mesh, 3, 0)
    distance = 0.002 + 0.5 * (0.05 - X[0]) * (1.0 + 0.2 * np.sin(40.0 * X[1]))  # synthetic: positive, smooth, not the true distance
    _compare("dry air axisymmetric + mixing length p3", c, c.state(seed=5, amp=0.02), mode="dist", distance=distance,
             ml=dict(max_mixing_length=0.004, pr_ratio=0.9, bulk_multiplier=0.5))


@pytest.mark.parametrize("table_dim", [1, 2])
def test_table_gas_axisym(table_dim):
    """table_dim = 2: the oracle has the one-dimensional table gas only, so -- as tests/test_gpu_lte2d.py does -- the state has a
    uniform density (0.4, between two lines of the density axis) and the oracle gets the one-dimensional gas the
    two-dimensional one is at that density (lte2d_util.blended_1d_physics)"""
    c = cases.lte_axisym(5, 7, 3, r_in=0.0, table_dim=table_dim)
    if table_dim == 1:
        _compare("table gas axisymmetric, table_dim 1, p3", c, c.state(seed=6, amp=0.02))
        return
    import lte2d_util

    rho = 0.4
    X = node_coordinates(c.mesh, 3, 0)
    U = cases.lte_state(X, c.physics, seed=6, rho0=np.full(X.shape[1], rho))
    _compare("table gas axisymmetric, table_dim 2, p3", c, U, oracle_physics=lte2d_util.blended_1d_physics(rho, capi.NS, False, "reference"))


def test_argon_ternary_3d_coulomb_table_configuration():
    """The configuration carries Devoto's third-order electron conductivity, which is ill-conditioned in double precision:
    one ulp of log(T_e), device against glibc, moves k_e by 4e-10 (tests/test_gpu_parity.py::_boost_transport;
    tests/test_gpu_visualization.py holds thermal_cond_elec of these closures to a bound derived for that cancellation, not
    to 1e-11).  With every transport coefficient at its physical value the case measures, on one MI355X: convective rows
    5.7e-16, total rows 4.6e-13, viscous rows 3.7e-11 -- the three energy rows, the twelve others at most 1.4e-15.  Taken
    apart on the same state: k_e of the device and of the oracle differ by 5.0e-10 of k_e, (k_e device - k_e oracle) grad T
    alone is 3.3 - 3.7e-11 of the energy rows, and 8e-16 is left without it; k_e grad T is 8.2 % of those rows.
    So the transport is multiplied as tests/test_gpu_parity.py multiplies it where k_e is of third order: viscosity, bulk
    viscosity, heavy conductivity and diffusion times 30, k_e left alone.  k_e grad T then weighs 0.082 / (30 * 0.918 + 0.082)
    = 0.30 % of the energy rows and its 5e-10 is worth 1.5e-12 of them: the row bound of 1e-11 holds every other term to
    1e-11 and k_e to 3e-9 of itself, six times its conditioning, instead of asking of k_e what no two libm's give."""
    c = cases.argon_cyl3d(3, 10, 3, 3)  # 5 760 nodes; ambipolar, argon-minimal, p = 3: the sweeps of this operator read the Coulomb table
    assert c.physics.gas_transport.third_order_k_electron
    _boost(c.physics, third_order=True)
    _compare("argon ternary 3-D argon-minimal p3", c, c.state(seed=7, amp=0.01))


def test_argon_six_species_axisym_two_temperatures_mixture_transport():
    ph = _boost(capi.argon_six_species_physics(capi.NS, capi.ARGON_MIXTURE, True, True, third_order_ke=False))
    c = cases.argon_axisym(5, 7, 2, physics=ph, r_in=0.0)
    _compare("argon six species axisymmetric 2-T mixture p2", c, c.state(seed=8, amp=0.01))


def test_four_species_planar_with_the_viscous_sponge():
    ph = _boost(capi.argon_levels_physics(1, False, capi.NS, capi.CONSTANT, True, True, third_order_ke=False))
    vs = ph.visc_sponge
    vs.enabled, vs.width, vs.ratio = 1, 0.04, 15.0
    vs.normal[0], vs.normal[1], vs.point[0], vs.point[1] = 0.3, 1.0, 0.1, 0.05
    mesh = meshgen.scramble_orientations(meshgen.box_quad(5, 7, lengths=(0.2, 0.1), warp=0.08), 7)
    c = cases.Case("box2d", mesh, capi.Disc(3, 0, 0, 0, 0), ph, [])
    U = cases.plasma_state(node_coordinates(mesh, 3, 0), ph, nvel=2, seed=9, amp=0.01)
    _compare("four species planar non-ambipolar constant + sponge p3", c, U, mode="at")


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
def _instantiations(nsp):
    for two_t in (False, True):
        for tr in [capi.CONSTANT] + ([capi.ARGON_MIXTURE] if nsp <= 7 else []) + ([capi.ARGON_MINIMAL] if nsp == 3 else []):
            yield two_t, tr


@pytest.mark.parametrize("ambi", [1, 0])
@pytest.mark.parametrize("nsp", [3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("geo", ["3d", "2d", "axi"])
def test_every_plasma_instantiation_of_the_pass(geo, nsp, ambi):
    """the enumeration of tools/sweep_instantiations.py (geometry x species count x ambipolar x 1-T / 2-T x transport):
    the gate against a miscompiled instantiation"""
    count = 0
    for two_t, tr in _instantiations(nsp):
        if nsp == 3:
            ph = capi.argon_ternary_physics(capi.NS, two_t, tr, "arrhenius", ambipolar=bool(ambi), third_order_ke=False)
        else:
            ph = capi.argon_levels_physics(nsp - 3, bool(ambi), capi.NS, tr, two_t, True, third_order_ke=False)
        _boost(ph)
        if geo == "3d":
            c = cases.argon_cyl3d(4, 12, 3, 1, physics=ph, wall_type=capi.VISC_ISOTH)
            nvel = 3
        elif geo == "axi":
            c = cases.argon_axisym(7, 11, 1, physics=ph, r_in=0.0)
            nvel = 3
        else:
            mesh = meshgen.scramble_orientations(meshgen.box_quad(7, 11, lengths=(0.2, 0.1), warp=0.08), 7)
            c = cases.Case("box2d", mesh, capi.Disc(1, 0, 0, 0, 0), ph, [])
            nvel = 2
        U = cases.plasma_state(node_coordinates(c.mesh, 1, 0), ph, nvel=nvel, seed=11, amp=0.005,
                               vel0=(1.0, 20.0, 3.0) if geo == "axi" else (20.0, 0.0, 0.0))
        _compare(f"{geo} nsp={nsp} ambi={ambi} 2T={int(two_t)} tr={tr} p1", c, U)
        count += 1
    assert count == (6 if nsp == 3 else (2 if nsp == 8 else 4))


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
GAMMA, RGAS = 1.4, 287.058


def _centre_box(warp):
    mesh = meshgen.scramble_orientations(meshgen.box_hex(3, 3, 3, lengths=(0.9, 0.6, 1.2), periodic=(False, False, False), warp=warp), 13)
    bcs = [capi.make_bc(int(a), capi.WALL, capi.VISC_ADIAB) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]
    c = cases.Case("box3", mesh, capi.Disc(2, 0, 0, 0, 0), capi.dry_air_physics(capi.NS), bcs)
    ex = np.asarray(mesh.elem_coords)
    centre = ex.reshape(-1, 3).min(axis=0) * 0.5 + ex.reshape(-1, 3).max(axis=0) * 0.5
    e = int(np.argmin(np.linalg.norm(ex.mean(axis=1) - centre, axis=1)))
    faces = (np.full(6, e, dtype=np.int32), np.arange(6, dtype=np.int32), np.arange(6, dtype=np.int32))
    return c, e, faces


def _sutherland(T, visc_mult=1.0):
    """DryAirTransport::ComputeFluxTransportProperties, src/transport_properties.cpp:224-266: mu = C1 T^1.5 / (T + S0)"""
    return visc_mult * 1.458e-6 * T ** 1.5 / (T + 110.4)


def test_couette_loads_on_the_centre_element():
    """rho, p constant, u = (a y, 0, 0) on an affine box: tau_xy = tau_yx = mu a is the only stress and there is no
    conduction.  VISCOUS loads (int F_v . n dS, n out of the element) of the six faces of the centre element, one patch each:
      x-momentum  +- mu a A on the two y-faces;   y-momentum  +- mu a A on the two x-faces (the stress is symmetric);
      energy      +- mu a^2 y_face A on the two y-faces (tau_xy u);   every other entry 0.
    All fields are polynomials the p = 2 space holds, so only rounding remains.  Bound: 1e-11 of mu a A.
    The shear rate: T = p / (rho R) is constant, but it is computed from E - rho u^2 / 2 and carries K eps T of rounding, which
    the nodal derivative turns into a conduction flux k K eps T / h, k = mu cp / Pr.  For that to stay below 1e-11 mu a the
    shear rate has to exceed (cp / Pr) K eps T / (1e-11 h) = 46 K per second (T = 294 K, h = 0.2 m); K = 10 for the three-term
    derivative of a p = 2 element gives 460, and a = 1000 is used.  (Measured at a = 37: 4.5e-11 of mu a A, all of it in the
    energy row.)"""
    c, e, faces = _centre_box(warp=0.0)
    X = node_coordinates(c.mesh, 2, 0)
    rho, p, a = 1.2, 101300.0, 1000.0
    U = np.zeros((5, X.shape[1]))
    U[0] = rho
    U[1] = rho * a * X[1]
    U[4] = p / (GAMMA - 1.0) + 0.5 * rho * (a * X[1]) ** 2
    mu = _sutherland(p / (rho * RGAS))
    op = _operator(c)
    surf = op.createSurface(faces=faces + (6,))
    got = surf.loads(_dev(op, U), "viscous").cpu().numpy()
    surf.close()
    op.close()
    ex = np.asarray(c.mesh.elem_coords)[e]
    want = np.zeros((6, 5))
    area_max = 0.0
    for f in range(6):
        fv = ex[sfu.face_vertices(3, f)]
        ctr = fv.mean(axis=0)
        out = ctr - ex.mean(axis=0)
        axis = int(np.argmax(np.abs(out)))
        sign = np.sign(out[axis])
        ext = fv.max(axis=0) - fv.min(axis=0)
        A = np.prod([ext[k] for k in range(3) if k != axis])
        area_max = max(area_max, A)
        if axis == 1:
            want[f, 1] = sign * mu * a * A
            want[f, 4] = sign * mu * a * a * ctr[1] * A
        elif axis == 0:
            want[f, 2] = sign * mu * a * A
    err = np.abs(got - want).max()
    print(f"Couette: mu = {mu:.6e}, worst |load - exact| = {err:.3e} = {err / (mu * a * area_max):.3e} of mu a A")
    assert np.abs(want).max() > 0.0
    assert err <= 1e-11 * mu * a * area_max, (got, want)


def test_pressure_gradient_loads_on_the_warped_centre_element():
    """fluid at rest, p = p0 + g . x on the WARPED box (p is trilinear in the reference coordinates: in the space): the
    CONVECTIVE momentum loads summed over the six faces of the centre element are int p n dS = g V, V the element's volume
    from tpsrhs_integrate of its indicator.  Bound: 1e-11 of |g| V."""
    c, e, faces = _centre_box(warp=0.07)
    X = node_coordinates(c.mesh, 2, 0)
    p0, g = 101300.0, np.array([3.0e4, -2.0e4, 1.0e4])
    U = np.zeros((5, X.shape[1]))
    U[0] = 1.2
    U[4] = (p0 + g @ X) / (GAMMA - 1.0)
    op = _operator(c)
    surf = op.createSurface(faces=faces + (6,))
    loads = surf.loads(_dev(op, U), "convective").cpu().numpy()
    ind = np.zeros(X.shape[1])
    ind[e * 27:(e + 1) * 27] = 1.0
    V = float(op.integrate(_dev(op, ind))[0].cpu().numpy()[0])
    surf.close()
    op.close()
    total = loads.sum(axis=0)
    err = np.abs(total[1:4] - g * V).max()
    print(f"pressure gradient: V = {V:.6e}, worst |sum of loads - g V| = {err:.3e} = {err / (np.linalg.norm(g) * V):.3e} of |g| V")
    assert V > 0.0
    assert err <= 1e-11 * np.linalg.norm(g) * V, (total, g * V)
    assert total[0] == 0.0 and total[4] == 0.0  # no mass and no energy crosses a face of a fluid at rest


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ns_case():
    c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 300.0
    return c, c.state(seed=21)


def test_composition_and_hygiene():
    import torch

    c, U = _ns_case()
    op = _operator(c)
    x = _dev(op, U)
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    op.Mult(x, y0)
    cur = {p: op.getFlux(x, p, gradients_current=True) for p in PARTS}  # Up / gradUp of x are held after Mult(x)
    op.Mult(x, y1)
    assert torch.equal(y0, y1), "Mult(x) before and after getFlux(x) gives the same bytes"
    fresh = {p: op.getFlux(x, p) for p in PARTS}
    again = {p: op.getFlux(x, p) for p in PARTS}
    for p in PARTS:
        assert torch.equal(cur[p], fresh[p]), f"{p}: gradients_current=True after Mult(x) is bit-equal to False"
        assert torch.equal(fresh[p], again[p]), f"{p}: two calls give the same bytes"
    Cf, Vf, Tf = (fresh[p].cpu().numpy() for p in PARTS)
    # one subtraction per entry, which the compiler may contract with the last multiply of either part
    assert np.all(np.abs(Tf - (Cf - Vf)) <= 2 * EPS * (np.abs(Cf) + np.abs(Vf)))
    assert not Vf[:, 0].any(), "the density row of VISCOUS is exactly 0"
    surf = op.createSurface(attributes=[1, 2, 3])
    for p in PARTS:
        loads = surf.loads(x, p)
        F = op.getFlux(x, p)
        n = op.NDofs
        ref = surf.integrate(F, "flux", row_stride=n, comp_stride=op.num_equation * n)
        assert loads.shape == (3, op.num_equation) and torch.equal(loads, ref), f"{p}: loads = getFlux, then integrate(flux)"
        assert torch.equal(loads, surf.loads(x, p, gradients_current=True))
    op.Mult(x, y1)
    assert torch.equal(y0, y1)
    with pytest.raises(ValueError):
        op.getFlux(x, "inviscid")
    surf.close()
    op.close()


_POISON_CHILD = """
import sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {tests!r}]
from tps_amd import capi, cases
from tps_amd.rhs_operator import RHSoperator
c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
U = c.state(seed=21)
op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
surf = op.createSurface(attributes=[3])
bad = 0
for p in ("total", "convective", "viscous"):
    bad += int(torch.isnan(op.getFlux(x, p)).sum()) + int(torch.isnan(surf.loads(x, p)).sum())
print("NAN", bad)
"""


def test_no_nan_under_poisoned_allocations():
    """a fresh child process with TPSRHS_POISON=1 (every device buffer of the library starts as NaN): every entry of out
    is written"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TPSRHS_POISON="1")
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD.format(root=root, tests=os.path.join(root, "tests"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "NAN 0" in r.stdout, r.stdout[-500:]
