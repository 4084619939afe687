"""tpsrhs_visualization_layout (host only, no device): the rows of tpsrhs_visualization_fields follow the registration
order of the reference's visualisation fields (src/M2ulPhyS.cpp:1690-1787) -- X_sp, Y_sp, n_sp, the four flux-transport
coefficients, diff_vel_<sp> (nvel rows per species), electric_cond, the momentum-transfer frequencies, rxn_rate_1..R."""
import ctypes as C

import pytest

from tps_amd import capi

PHYSICS = {
    "ternary": lambda: capi.argon_ternary_physics(),
    "ternary_balance": lambda: capi.argon_ternary_physics(reactions="balance"),
    "ternary_no_reactions": lambda: capi.argon_ternary_physics(reactions=None),
    "six_species": lambda: capi.argon_six_species_physics(),
    "levels5": lambda: capi.argon_levels_physics(levels=5),
}
GEOMETRY = {"planar": (2, 0, 2), "axisymmetric": (2, 1, 3), "3d": (3, 0, 3)}


@pytest.mark.parametrize("geometry", list(GEOMETRY))
@pytest.mark.parametrize("physics", list(PHYSICS))
def test_rows_follow_the_registration_order(physics, geometry):
    ph = PHYSICS[physics]()
    dim, axi, nvel = GEOMETRY[geometry]
    lay = capi.visualization_layout(ph, dim, bool(axi))
    nsp, R = ph.mixture.num_species, ph.chemistry.num_reactions
    assert (lay.num_species, lay.nvel, lay.num_reactions) == (nsp, nvel, R)
    assert lay.nrows == 4 * nsp + nsp * nvel + 5 + R
    assert (lay.Xsp, lay.Ysp, lay.nsp_) == (0, nsp, 2 * nsp)
    assert lay.FluxTrns == 3 * nsp
    assert lay.diffVel == 3 * nsp + 4
    assert lay.SrcTrns == lay.diffVel + nsp * nvel
    assert lay.SpeciesTrns == lay.SrcTrns + 1
    if R:
        assert lay.rxn == lay.SpeciesTrns + nsp and lay.rxn + R == lay.nrows
    else:
        assert lay.rxn == -1 and lay.SpeciesTrns + nsp == lay.nrows


def test_names_are_the_references_and_cover_every_row_once():
    ph = capi.argon_ternary_physics()
    lay = capi.visualization_layout(ph, 2, True)
    names = capi.visualization_names(lay, ["Ar.+1", "E", "Ar"])
    assert [n for n, _, _ in names] == [
        "X_Ar.+1", "X_E", "X_Ar", "Y_Ar.+1", "Y_E", "Y_Ar", "n_Ar.+1", "n_E", "n_Ar",
        "viscosity", "bulk_viscosity", "thermal_cond_heavy", "thermal_cond_elec",
        "diff_vel_Ar.+1", "diff_vel_E", "diff_vel_Ar", "electric_cond",
        "momentum_tranfer_freq_Ar.+1", "momentum_tranfer_freq_E", "momentum_tranfer_freq_Ar", "rxn_rate_1", "rxn_rate_2"]
    covered = [r for _, first, rows in names for r in range(first, first + rows)]
    assert covered == list(range(lay.nrows))
    assert dict((n, rows) for n, _, rows in names)["diff_vel_E"] == 3
    assert [n for n, _, _ in capi.visualization_names(lay)][:3] == ["X_sp0", "X_sp1", "X_sp2"]
    with pytest.raises(ValueError):
        capi.visualization_names(lay, ["Ar"])


@pytest.mark.parametrize("physics", [lambda: capi.dry_air_physics(), lambda: capi.lte_physics()], ids=["dry_air", "lte_table"])
def test_dry_air_and_the_table_gas_are_refused(physics):
    lib = capi.load()
    out = capi.VisLayout()
    assert lib.tpsrhs_visualization_layout(C.byref(physics()), 2, 1, C.byref(out)) == capi.ERR_UNSUPPORTED
    assert b"visualization" in lib.tpsrhs_last_error()


def test_invalid_arguments_are_refused():
    lib = capi.load()
    ph, out = capi.argon_ternary_physics(), capi.VisLayout()
    bad = capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_visualization_layout(None, 3, 0, C.byref(out)) == bad
    assert lib.tpsrhs_visualization_layout(C.byref(ph), 3, 0, None) == bad
    assert lib.tpsrhs_visualization_layout(C.byref(ph), 1, 0, C.byref(out)) == bad
    assert lib.tpsrhs_visualization_layout(C.byref(ph), 3, 1, C.byref(out)) == bad  # no axisymmetric 3-D
    ph.chemistry.num_reactions = -1
    assert lib.tpsrhs_visualization_layout(C.byref(ph), 3, 0, C.byref(out)) == bad
    assert lib.tpsrhs_visualization_fields(None, None, None) == bad
