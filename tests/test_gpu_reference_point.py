"""tpsrhs_visualization_fields on the device against RECORDED values of the reference's own compiled point physics
(tests/golden/reference_point/*.npz, written by tests/golden/make_reference_point.py from oracle/_ref/libtpsref_point.so).
Only the committed fixtures are read: neither that library nor a checkout of the reference, and no oracle value enters a
comparison.  The kernel is a pure point map built from the physics_plasma.hpp functions k_gradient and k_flux use.

Setup: the fixture's 64 states sit on the 64 nodes of a 4 x 4 periodic quad mesh at p = 1, every node its own state; one
launch per configuration.  Compared, per row relative to the row's max norm (visualization_util.row_errors), bound
visualization_util.RTOL = 1e-11: mole and mass fractions, number densities, the four flux-transport coefficients, the
electric conductivity, the momentum-transfer frequencies and the progress rate of every reaction.  As in
tests/test_gpu_visualization.py, and for the reason written there (the electron-argon collision integrals cancel to 1e-5
of their terms), thermal_cond_elec of the third-order closures and the momentum-transfer frequency of a neutral species
are held to the bounds DERIVED in visualization_util (POLY_BOUND / FIT_BOUND carried through the closure), and a progress
rate is scaled by its un-cancelled magnitude kf (prod n^nu' + prod n^nu'' / kC); nothing else is widened.

The diffusion velocities are NOT compared here: they are linear in the primitive gradient, the fixture's gradients are
random per state, and the device computes its own DG gradient of the nodal field -- 64 unrelated nodal states on 16
bilinear elements with jump terms cannot reproduce 64 prescribed gradients (4 nodal values per element and variable
against 8 prescribed gradient components).  They are compared with the reference on the CPU
(tests/test_reference_point.py: flux_diffusion_velocity, source_diffusion_velocity, bit for bit)."""
import functools
import os

import numpy as np
import pytest

import visualization_util as vu
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
RTOL = vu.RTOL
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_point")
# key -> physics of the fixture (tests/ref_point_lib.py::make_physics, restated here so that this file imports nothing that
# loads the reference library)
PHYSICS = {
    "2d_n3_ambi_2T_constant": lambda: capi.argon_ternary_physics(capi.NS, True, capi.CONSTANT, "balance", ambipolar=True,
                                                                third_order_ke=False, radiation=True),
    "2d_n3_ambi_1T_minimal_ke3": lambda: capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL, "arrhenius", ambipolar=True,
                                                                   third_order_ke=True, radiation=True),
    "2d_n3_ambi_1T_minimal_ke1": lambda: capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL, "arrhenius", ambipolar=True,
                                                                   third_order_ke=False, radiation=True),
    "2d_n5_1T_mixture": lambda: capi.argon_levels_physics(2, False, capi.NS, capi.ARGON_MIXTURE, False, True, third_order_ke=False,
                                                          radiation=True),
    "2d_n6_2T_mixture_ke3": lambda: capi.argon_levels_physics(3, False, capi.NS, capi.ARGON_MIXTURE, True, True, third_order_ke=True,
                                                              radiation=True),
}


@functools.lru_cache(maxsize=None)
def _setup(key):
    """(case, state [neq, 64], reference rows [nrows, 64] with NaN where the fixture holds nothing, helper dict)"""
    with np.load(os.path.join(FIXTURE_DIR, key + ".npz")) as f:
        fx = {k: f[k] for k in f.files}
    assert str(fx["key"]) == key
    ph = PHYSICS[key]()
    c = cases.Case(key, meshgen.box_quad(4, 4), capi.Disc(1, 0, 0, 0, 0), ph, [])
    U = np.ascontiguousarray(fx["U"].T)  # node i carries state i
    assert U.shape[1] == 64
    lay = capi.visualization_layout(ph, 2, False)
    nsp, R = lay.num_species, lay.num_reactions
    rows = np.full((lay.nrows, 64), np.nan)
    rows[lay.Xsp:lay.Xsp + nsp] = fx["mole_fractions"].T
    rows[lay.Ysp:lay.Ysp + nsp] = fx["mass_fractions"].T
    rows[lay.nsp_:lay.nsp_ + nsp] = fx["species_number_densities"].T
    rows[lay.FluxTrns:lay.FluxTrns + 4] = fx["flux_transport"].T
    rows[lay.SrcTrns] = fx["electric_conductivity"][:, 0]
    rows[lay.SpeciesTrns:lay.SpeciesTrns + nsp] = fx["mt_frequency"].T
    if R:
        rows[lay.rxn:lay.rxn + R] = fx["progress_rates"].T
    nvel = lay.nvel
    Th = fx["prim"][:, nvel + 1]
    Te = fx["prim"][:, -1] if ph.mixture.two_temperature else Th
    ref = dict(rows=rows, layout=lay, n_sp=np.ascontiguousarray(fx["number_densities"].T), Th=Th, Te=Te)
    for v in (rows, U):
        v.setflags(write=False)
    return c, U, ref


def _row_bounds(key, c, ref, got):
    """-> list of (row name, error, allowed) for every compared row"""
    lay, ph = ref["layout"], c.physics
    rows = ref["rows"]
    ke_bound = vu.electron_conductivity_bound(ph, ref)
    mt_bound = vu.momentum_transfer_bound(ph, ref)
    out = []
    for gname, first, n in vu.groups(lay):
        if gname == "diff_vel":
            continue  # CPU leg only: see the module docstring
        if gname == "rxn_rate":
            scales, _ = vu.rate_scale_and_closed_form(ph, ref["n_sp"], ref["Th"], ref["Te"])
            for r in range(n):
                e = vu.row_errors(got[first + r], rows[first + r], scales[r])[0]
                out.append((f"rxn_rate_{r + 1}", e, RTOL))
            continue
        err = vu.row_errors(got[first:first + n], rows[first:first + n])
        diff = np.abs(got[first:first + n] - rows[first:first + n]).max(axis=1)
        for k in range(n):
            if gname == "flux transport" and k == 3 and ke_bound is not None:
                out.append(("thermal_cond_elec (derived bound)", diff[k] / ke_bound.max(), 1.0))
            elif gname == "mt_freq" and mt_bound is not None and np.isfinite(mt_bound[k, 0]):
                out.append((f"mt_freq_{k} (derived bound)", diff[k] / mt_bound[k].max(), 1.0))
            else:
                out.append((f"{gname}_{k}", err[k], RTOL))
    return out


@pytest.mark.parametrize("key", list(PHYSICS))
def test_fields_match_the_recorded_reference(key):
    c, U, ref = _setup(key)
    _, got = vu.device_fields(c, U)
    assert got.shape == ref["rows"].shape
    assert np.all(np.isfinite(got))
    res = _row_bounds(key, c, ref, got)
    for name, e, tol in res:
        print(f"{key}: {name}: {e:.3e} (allowed {tol:.1e})")
    bad = [(n, e) for n, e, tol in res if not e <= tol]
    assert not bad, bad


def test_a_permuted_fixture_row_fails():
    """layout control: with two rows of the recorded values exchanged the comparison must turn red in exactly those rows --
    a mix-up that compared a row with itself, or the wrong pair of rows, would stay green"""
    key = "2d_n6_2T_mixture_ke3"
    c, U, ref = _setup(key)
    _, got = vu.device_fields(c, U)
    lay = ref["layout"]
    a, b = lay.nsp_ + 1, lay.SpeciesTrns + 1  # a number density and a momentum-transfer frequency
    rows = ref["rows"].copy()
    rows[[a, b]] = rows[[b, a]]
    bad = dict(ref, rows=rows)
    names = {n for n, e, tol in _row_bounds(key, c, bad, got) if not e <= tol}
    assert names == {"n_sp_1", "mt_freq_1 (derived bound)"}, names
    assert not [n for n, e, tol in _row_bounds(key, c, ref, got) if not e <= tol]
