"""tpsrhs_visualization_fields on the device against the CPU oracle, node by node (tests/visualization_util.py).

Tolerance: the project's HIP-vs-oracle bound, relative 1e-11, per row in the max-norm, every row scaled by its own magnitude
max_n |reference| -- with these exceptions:
 - a diffusion velocity is asked 0.5e-11 of its own magnitude: the issue scales by the largest term of the sum before the
   flux correction, and V = V0 - sum Y V0 gives |V| <= 2 max |V0|, so half the tolerance on the row's own magnitude asks no
   less (achieved: at most 1.4e-12, 4.7e-12 in the state below 2 000 K);
 - a progress rate is scaled by kf (prod n^nu' + prod n^nu'' / kC), the species-source identity by M sum_r |nu'' - nu'| |q_r|:
   the net values vanish at equilibrium;
 - thermal_cond_elec of the third-order collision-integral closures and the momentum-transfer frequency of a neutral
   species cannot meet 1e-11 of their own magnitude (2e-11 ... 9e-11 and up to 2e-11 on an MI355X): both hang on the
   electron-argon collision integrals, polynomials in log T_e whose terms cancel to 1e-5 of their sum of magnitudes, so
   the 4 ulp of fastmath.hpp's logarithm come back a hundred-thousandfold.  Their bound is DERIVED from the accuracies
   tests/test_gpu_fastmath.py pins -- 51 ulp of the polynomial's sum of magnitudes, 1.5e-14 of a Coulomb fit -- and
   carried through the closure: visualization_util.POLY_BOUND / FIT_BOUND (the derivation) and
   electron_conductivity_bound / momentum_transfer_bound.  It follows the cancellation and nothing else: the factors
   around the polynomial get 16 ulp.
The achieved error of every group is printed.

Shapes: the smallest at which each path can go wrong -- 486 nodes (two 256-lane blocks, the last one ragged), 24 nodes
(less than a block), and one mixture per kernel shape that differs."""
import functools

import numpy as np
import pytest

import visualization_util as vu
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
RTOL = vu.RTOL


def _gll_planar():
    mesh = meshgen.box_quad(3, 3, lengths=(1.0, 0.8), warp=0.05)
    return cases.Case("gll_planar_p2", mesh, capi.Disc(2, 1, 1, 0, 0), capi.argon_ternary_physics(), [])


CASES = {
    # 3-D ambipolar ternary, one temperature, argon-minimal transport: the benchmark's family; 18 hexes x 27 nodes = 486
    "bench3d": lambda: cases.argon_cyl3d(2, 3, 3, 2),
    # axisymmetric two-temperature ternary with the mixture transport (nvel = 3 != dim), 6 quads x 4 nodes = 24
    "axisym_mixture": lambda: cases.argon_axisym(2, 3, 1, True, capi.ARGON_MIXTURE),
    # six species, not ambipolar, two temperatures, constant transport (the torch mixture)
    "torch6": lambda: cases.argon_axisym(3, 4, 2, physics=capi.argon_six_species_physics()),
    # eight species, 3-D: the register-heaviest family
    "levels5_3d": lambda: cases.argon_cyl3d(2, 3, 3, 1, physics=capi.argon_levels_physics(levels=5)),
    # seven species with the mixture transport
    "seven_mixture": lambda: cases.argon_axisym(3, 3, 2, physics=capi.argon_levels_physics(levels=4, transport=capi.ARGON_MIXTURE)),
    # Gauss-Lobatto pair, planar, p = 2
    "gll_planar": _gll_planar,
    # the other rate laws on the small axisymmetric mesh (two temperatures, constant transport)
    "balance": lambda: cases.argon_axisym(2, 3, 1, reactions="balance"),
    "tabulated": lambda: cases.argon_axisym(2, 3, 1, reactions="tabulated"),
    "tabulated_loglog": lambda: cases.argon_axisym(2, 3, 1, reactions="tabulated_loglog"),
    "hoffertlien": lambda: cases.argon_axisym(2, 3, 1, reactions="hoffertlien"),
    # the benchmark's family BELOW Chemistry's minimum temperature: the floor decides every rate
    "bench3d_cold": lambda: cases.argon_cyl3d(2, 3, 3, 2),
}


def _state(name, c, seed=7):
    if name == "bench3d_cold":
        return vu.cold_state(c)
    if name == "gll_planar":
        from tps_amd.rhs_operator import node_coordinates

        return c.state(seed=seed, coords=node_coordinates(c.mesh, 2, 1))
    return c.state(seed=seed)


@functools.lru_cache(maxsize=None)
def _setup(name):
    """(case, state, oracle reference): computed once per case, shared by the tests and left unchanged"""
    c = CASES[name]()
    U = _state(name, c)
    ref = vu.reference(c, U)
    ref.pop("oracle")
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    U.setflags(write=False)
    return c, U, ref


def _check_rates(name, c, ref, got):
    lay, ph = ref["layout"], c.physics
    R = lay.num_reactions
    if not R:
        return
    q = got[lay.rxn:lay.rxn + R]
    assert np.all(np.isfinite(q))
    # every active species row: M_sp sum_r (nu'' - nu') q_r == point_source
    lhs, scale, src = vu.species_source_identity(ph, lay.nvel, q, ref["src"])
    err = vu.row_errors(lhs, src, scale)
    print(f"{name}: species-source identity, error / un-cancelled magnitude per species row = {err}")
    assert err.max() < RTOL
    # Arrhenius reactions: Chemistry's closed form on the oracle's number densities and temperatures
    scales, closed = vu.rate_scale_and_closed_form(ph, ref["n_sp"], ref["Th"], ref["Te"])
    for r in range(R):
        if closed[r] is None:
            continue
        e = vu.row_errors(q[r], closed[r], scales[r])[0]
        print(f"{name}: rxn_rate_{r + 1} against the closed form, error / kf (fwd + bwd / kC) = {e:.3e}")
        assert e < RTOL
    if name == "balance":  # one reaction: q_1 = (source of Ar+) / M_Ar+
        _, mw, _ = vu.mixture(ph)
        e = vu.row_errors(q[0], ref["src"][lay.nvel + 2] / mw[0], scales[0])[0]
        print(f"{name}: q_1 against point_source / M, error / kf (fwd + bwd / kC) = {e:.3e}")
        assert e < RTOL


@pytest.mark.parametrize("name", list(CASES))
def test_fields_match_the_oracle(name):
    c, U, ref = _setup(name)
    fields, got = vu.device_fields(c, U)
    lay = ref["layout"]
    assert got.shape == ref["rows"].shape == (lay.nrows, U.shape[1])
    assert np.all(np.isfinite(got))
    if name == "bench3d":
        assert U.shape[1] > 256 and U.shape[1] % 256 != 0
    if name == "bench3d_cold":
        assert ref["Th"].max() < c.physics.chemistry.minimum_temperature
    ke_bound = vu.electron_conductivity_bound(c.physics, ref)
    mt_bound = vu.momentum_transfer_bound(c.physics, ref)
    for gname, first, rows in vu.groups(lay):
        if gname == "rxn_rate":
            continue
        err = vu.row_errors(got[first:first + rows], ref["rows"][first:first + rows])
        print(f"{name}: {gname}: max relative row error {err.max():.3e}")
        tol = np.full(rows, RTOL / 2 if gname == "diff_vel" else RTOL)  # in units of the row's own magnitude
        diff = np.abs(got[first:first + rows] - ref["rows"][first:first + rows]).max(axis=1)
        if gname == "flux transport" and ke_bound is not None:  # thermal_cond_elec: the derived bound
            print(f"{name}: thermal_cond_elec: {err[3]:.3e} of its own magnitude, {diff[3] / ke_bound.max():.3e} of the derived bound")
            assert diff[3] <= ke_bound.max(), (diff[3], ke_bound.max())
            err[3] = 0.0
        if gname == "mt_freq" and mt_bound is not None:  # the neutrals' rows: the derived bound
            for sp in np.flatnonzero(np.isfinite(mt_bound[:, 0])):
                print(f"{name}: mt_freq of neutral species {sp}: {err[sp]:.3e} of its own magnitude, "
                      f"{diff[sp] / mt_bound[sp].max():.3e} of the derived bound")
                assert diff[sp] <= mt_bound[sp].max(), (sp, diff[sp], mt_bound[sp].max())
                err[sp] = 0.0
        assert np.all(err < tol), (gname, err)
    _check_rates(name, c, ref, got)
    # the dict: the reference's names in row order, views of the one array
    names = capi.visualization_names(lay)
    assert list(fields) == [n for n, _, _ in names]
    for n, first, rows in names:
        assert np.array_equal(fields[n], got[first] if rows == 1 else got[first:first + rows])
    nsp = lay.num_species
    assert fields["diff_vel_sp0"].shape == (lay.nvel, U.shape[1])
    if lay.nvel == 3 and c.mesh.dim == 2:  # the azimuthal component: no gradient in that direction
        assert all(np.all(fields[f"diff_vel_sp{sp}"][2] == 0.0) for sp in range(nsp))
    if name == "bench3d":  # a one-temperature mixture: the frequencies are filled all the same
        assert np.all(fields["momentum_tranfer_freq_sp0"] > 0) and np.all(fields["momentum_tranfer_freq_sp2"] > 0)


def test_fields_are_those_of_x_not_of_a_stale_up_and_repeat_bitwise():
    import torch

    from tps_amd.rhs_operator import RHSoperator

    c, U, _ = _setup("axisym_mixture")
    U2 = c.state(seed=99)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x1 = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    x2 = torch.tensor(U2.ravel(), dtype=torch.float64, device=op.device)
    _, a = op.visualizationFields(x1, return_array=True)
    a = a.cpu().numpy()
    y = torch.empty_like(x2)
    op.Mult(x2, y)  # leaves Up and gradUp of x2 in the operator
    _, b = op.visualizationFields(x1, return_array=True)
    b = b.cpu().numpy()
    _, d = op.visualizationFields(x2, return_array=True)
    d = d.cpu().numpy()
    lay = op.visualizationLayout()
    op.close()
    assert np.array_equal(a, b)
    for first in (lay.nsp_, lay.FluxTrns, lay.diffVel, lay.SrcTrns, lay.rxn):
        assert not np.array_equal(a[first], d[first])


def test_rates_compose_to_the_species_source_of_mult_on_the_device():
    """Ties progress_rates (the post-processing copy of the rate loop) to `source` (the one the sweeps inline), both on the
    device: for a UNIFORM state on a periodic box every flux is constant, so the species row of Mult is the chemical source
    M_sp sum_r (nu'' - nu') q_r alone, up to the rounding of the divergence of a constant flux.  Bound: 1e-11 of the
    un-cancelled source M sum_r |nu'' - nu'| |q_r|, plus that rounding -- per node 2 dim sums (volume and faces) of p + 1
    products of a differentiation weight <= (p + 1)^2 / h with the flux |rho_sp u|, each rounded: 4 dim (p + 1)^3 / h ulp
    of the flux."""
    import torch

    from tps_amd.rhs_operator import RHSoperator, node_coordinates

    order, ncell = 2, 3
    mesh = meshgen.box_quad(ncell, ncell)
    c = cases.Case("uniform_box", mesh, capi.Disc(order, 0, 0, 0, 0), capi.argon_ternary_physics(), [])
    N = node_coordinates(mesh, order).shape[1]
    _, mw, _ = vu.mixture(c.physics)
    one = np.ones(N)
    Th, alpha = 9000.0, 2.0e-3
    nh = 101300.0 / (vu.R_U * Th * (1.0 + alpha))
    ni = alpha * nh
    rho = ni * mw[0] + ni * mw[1] + (nh - ni) * mw[2]
    vel = (20.0, -7.0)
    U = cases.plasma_conserved(c.physics, 2, rho * one, [v * one for v in vel], Th * one, [ni * one], None)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    op.Mult(x, y)
    fields = op.visualizationFields(x)
    lay = op.visualizationLayout()
    q = np.stack([fields[f"rxn_rate_{r + 1}"].cpu().numpy() for r in range(lay.num_reactions)])
    src = y.cpu().numpy().reshape(U.shape)
    op.close()
    lhs, scale, got = vu.species_source_identity(c.physics, lay.nvel, q, src)
    flux = ni * mw[0] * max(abs(v) for v in vel)
    noise = 4 * 2 * (order + 1) ** 3 * ncell * vu.EPS * flux
    err = np.abs(lhs - got).max()
    print(f"species source of Mult {np.abs(got).max():.3e}, un-cancelled {scale.max():.3e}, difference {err:.3e}, "
          f"allowed {RTOL * scale.max() + noise:.3e} (divergence rounding {noise:.3e})")
    assert np.abs(got).max() > 1e-3 * scale.max()  # a state away from equilibrium: the source is there to compare
    assert err <= RTOL * scale.max() + noise


def test_rows_compose_with_integrate_and_a_sampler():
    """The same device operations on the device's row and on the oracle's row: both are linear in the field, so the results
    differ by at most (operator norm) x RTOL x max |row| -- the integral by the measure of the domain (the integral of 1,
    with the radial weight here), a sample by the Lebesgue constant of the tensor Gauss-Legendre nodes, below 2 per
    direction for p <= 3 inside the element."""
    import torch

    from tps_amd.rhs_operator import PointSampler, RHSoperator

    c, U, ref = _setup("torch6")
    lay = ref["layout"]
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    fields = op.visualizationFields(x)
    rows = ["thermal_cond_heavy", "electric_cond", "n_sp4", "momentum_tranfer_freq_sp0"]
    idx = {n: first for n, first, _ in capi.visualization_names(lay)}
    rng = np.random.Generator(np.random.MT19937(5))
    corners = c.mesh.elem_coords.reshape(-1, c.mesh.dim)
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    pts = (lo[:, None] + (hi - lo)[:, None] * rng.uniform(0.05, 0.95, size=(2, 9)))
    sampler = PointSampler(op, pts)
    ones = torch.ones(op.NDofs, dtype=torch.float64, device=op.device)
    measure = float(op.integrate(ones)[0][0])
    for n in rows:
        r = torch.tensor(np.ascontiguousarray(ref["rows"][idx[n]]), dtype=torch.float64, device=op.device)
        top = float(np.abs(ref["rows"][idx[n]]).max())
        gi, ri = float(op.integrate(fields[n])[0][0]), float(op.integrate(r)[0][0])
        gs, rs = sampler.sample(fields[n]).cpu().numpy(), sampler.sample(r).cpu().numpy()
        print(f"{n}: integral {gi!r} vs {ri!r}; samples differ by {np.abs(gs - rs).max():.3e} of {top:.3e}")
        assert abs(gi - ri) <= RTOL * top * measure
        assert np.abs(gs - rs).max() <= 4.0 * RTOL * top
        mn, mx, _ = op.nodalStats(fields[n])
        assert float(mn[0]) == float(fields[n].min()) and float(mx[0]) == float(fields[n].max())
    sampler.close()
    op.close()


def test_unsupported_physics_and_a_set_mixing_length_are_refused():
    import torch

    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    for c in (cases.cyl3d(2, 3, 3, 1, capi.EULER), cases.lte_axisym(3, 3, 2)):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
        x = torch.tensor(c.state(seed=1).ravel(), dtype=torch.float64, device=op.device)
        with pytest.raises(RuntimeError) as e:
            op.visualizationFields(x)
        assert getattr(e.value, "status", None) == capi.ERR_UNSUPPORTED
        out = torch.empty(64 * op.NDofs, dtype=torch.float64, device=op.device)
        assert vu.raw_fields(op, x, out) == capi.ERR_UNSUPPORTED
        op.close()
    c, U, _ = _setup("axisym_mixture")
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    op.setMixingLength(torch.full((op.NDofs,), 0.01, dtype=torch.float64, device=op.device), max_mixing_length=0.005)
    with pytest.raises(TpsRhsError) as e:
        op.visualizationFields(x)
    assert e.value.status == capi.ERR_UNSUPPORTED and "mixing length" in str(e.value)
    op.setMixingLength(None)
    assert set(op.visualizationFields(x)) >= {"electric_cond"}
    op.close()


@pytest.mark.parametrize("name", ["axisym_mixture", "levels5_3d"])
def test_every_row_of_every_node_is_written(name, monkeypatch):
    """the pattern of tests/test_gpu_poison.py: the library's allocations and `out` itself start as NaN"""
    import torch

    from tps_amd.rhs_operator import RHSoperator

    monkeypatch.setenv("TPSRHS_POISON", "1")
    c, U, ref = _setup(name)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    out = torch.full((ref["layout"].nrows + 1, op.NDofs), float("nan"), dtype=torch.float64, device=op.device)
    assert vu.raw_fields(op, x, out) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    op.close()
    assert np.all(np.isfinite(got[:-1]))
    assert np.all(np.isnan(got[-1]))  # ... and nothing past the last row
    lay = ref["layout"]  # (the values themselves: test_fields_match_the_oracle; here the species rows, which are exact to a few ulp)
    assert vu.row_errors(got[:lay.FluxTrns], ref["rows"][:lay.FluxTrns]).max() < RTOL
