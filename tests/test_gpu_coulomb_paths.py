"""One Mult of the 3-D p = 3 argon-minimal sweeps with the Coulomb fits from the polynomial table (coulomb_table.hpp):
(a) against the CPU oracle at the bound of tests/test_gpu_lean_one_hex.py -- third-order k_e on and off (eight rows of the
table, or att11 and rep22 alone), both kernel families (ambipolar or not), isothermal wall, scrambled orientations;
(b) against the same library with TPSRHS_COULOMB_TABLE=0 (the formulas): y and gradUp within the same bound, Up -- which
no transport coefficient enters -- bit for bit;
(c) a cold, half-ionised gas whose ln Tp straddles the table's lower end, so that the lanes of one wave split between the
table and the formulas: table on against table off."""
import numpy as np
import pytest

from parity_util import hip_mult, rel_maxnorm
from test_gpu_parity import _boost_transport, _compare, _tol
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu

AMP = 0.01
X0 = -4.0  # tps_amd/csrc/coulomb_table.hpp (tests/test_coulomb_table.py::test_layout checks it)


def _case(ambipolar=True, third_order=True):
    ph = capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL, "arrhenius", ambipolar=ambipolar, third_order_ke=third_order)
    _boost_transport(ph)
    c = cases.argon_cyl3d(3, 11, 3, 3, wall_type=capi.VISC_ISOTH, physics=ph)
    c.mesh = meshgen.scramble_orientations(c.mesh, 5)
    return c


def _on_off(c, U, monkeypatch):
    monkeypatch.delenv("TPSRHS_COULOMB_TABLE", raising=False)
    on = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U)
    monkeypatch.setenv("TPSRHS_COULOMB_TABLE", "0")
    off = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U)
    monkeypatch.delenv("TPSRHS_COULOMB_TABLE")
    return on, off


def _assert_close(on, off, neq, tol):
    e_y = rel_maxnorm(on["y"], off["y"])
    e_g = np.abs(on["gradUp"] - off["gradUp"]).max() / np.abs(off["gradUp"]).max()
    print("table on against off: rel err y", e_y, "gradUp", e_g)
    assert np.all(np.isfinite(on["y"])) and np.all(np.isfinite(off["y"]))
    assert np.array_equal(np.ascontiguousarray(on["Up"]).view(np.int64), np.ascontiguousarray(off["Up"]).view(np.int64))
    assert e_g < tol
    assert e_y.max() < tol


@pytest.mark.parametrize("ambipolar", [True, False])
@pytest.mark.parametrize("third_order", [True, False])
def test_table_against_oracle(ambipolar, third_order, monkeypatch):
    monkeypatch.delenv("TPSRHS_COULOMB_TABLE", raising=False)
    c = _case(ambipolar, third_order)
    _compare(c.mesh, c.disc, c.physics, c.bcs, c.state(seed=21, amp=AMP), tol=_tol(AMP))


@pytest.mark.parametrize("third_order", [True, False])
def test_table_against_formulas(third_order, monkeypatch):
    c = _case(True, third_order)
    U = c.state(seed=21, amp=AMP)
    on, off = _on_off(c, U, monkeypatch)
    _assert_close(on, off, U.shape[0], _tol(AMP))


def test_cold_half_ionised_straddles_the_table_end(monkeypatch):
    c = _case(True, True)
    ph = c.physics
    X = node_coordinates(c.mesh, 3)
    w = cases._waves(X, 21, kmax=1)
    Th = 600.0 + 300.0 * w()
    alpha = 0.5 * np.ones_like(Th)
    p = 101300.0 * (1.0 + 0.01 * w())
    R = capi.UNIVERSALGASCONSTANT
    nh = p / (R * Th * (1.0 + alpha))
    ni = alpha * nh
    nsp = 3
    mw = [ph.mixture.gas_params[sp + capi.SPECIES_MW * nsp] for sp in range(nsp)]
    rho = ni * mw[0] + ni * mw[1] + (nh - ni) * mw[2]
    vel = [20.0 + 0.2 * w(), 0.2 * w(), 0.2 * w()]
    U = cases.plasma_conserved(ph, 3, rho, vel, Th, [ni], None)
    # ln Tp of the nodes (PlasmaPhys::debye: the constants of physics_plasma.hpp), n_e = n_i, T_e = T_h
    NA, qe, eps0 = 6.0221409e+23, 1.60218e-19, 8.8541878128e-12
    dfac = (8.3144598 / NA) * eps0 / qe / qe
    x = np.log(4.0 * np.pi * dfac * np.sqrt(dfac / NA / (2.0 * ni / Th)) * Th)
    below = float((x < X0).mean())
    print(f"ln Tp in [{x.min():.2f}, {x.max():.2f}], {100 * below:.0f} % of the nodes below the table")
    assert 0.1 < below < 0.9
    on, off = _on_off(c, U, monkeypatch)
    _assert_close(on, off, U.shape[0], _tol(AMP))
