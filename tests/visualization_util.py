"""Reference of tpsrhs_visualization_fields (tests/test_gpu_visualization.py): the rows of
M2ulPhyS::updateVisualizationVariables (src/M2ulPhyS.cpp:4156-4263) from the CPU oracle, node by node.

Up and gradUp are the oracle operator's own (update_primitives / compute_gradients) for the same state; per node
point_flux_transport, point_source_transport and point_source; X, Y and n in numpy from the number densities the
oracle returns.  The progress rates, which the oracle does not expose, are restated here in closed form for the Arrhenius
law and otherwise pinned through the species-source identity (see rates_closed_form / species_source_identity)."""
import ctypes as C
import functools
import os

import numpy as np

from tps_amd import capi, cases
from tps_amd.rhs_operator import node_coordinates

RTOL = 1e-11  # the project's HIP-vs-oracle bound (parity_util.RHS_RTOL)
R_U = capi.UNIVERSALGASCONSTANT


def mixture(ph):
    mx = ph.mixture
    nsp = mx.num_species
    mw = np.array([mx.gas_params[sp + capi.SPECIES_MW * nsp] for sp in range(nsp)])
    z = np.array([mx.gas_params[sp + capi.SPECIES_CHARGES * nsp] for sp in range(nsp)])
    return nsp, mw, z


def stoichiometry(ph):
    nsp, R = ph.mixture.num_species, ph.chemistry.num_reactions
    re_ = np.array([[ph.chemistry.reactant_stoich[sp + r * nsp] for sp in range(nsp)] for r in range(R)]).reshape(R, nsp)
    pr = np.array([[ph.chemistry.product_stoich[sp + r * nsp] for sp in range(nsp)] for r in range(R)]).reshape(R, nsp)
    return re_, pr


def reference(case, U):
    """dict(rows=[nrows, NDofs] of the oracle, layout, n_sp [nsp, N], Th, Te [N], src [neq, N] = point_source, Up, gradUp)"""
    from oracle_lib import Oracle, _p, lib

    ph, disc, mesh = case.physics, case.disc, case.mesh
    o = Oracle(mesh, disc, ph, case.bcs)
    U = np.ascontiguousarray(U, dtype=np.float64)
    lib().tpsoracle_update_primitives(o.h, _p(U))
    Up = o.primitives()
    g = o.compute_gradients()  # (dim, neq, N)
    N, neq, dim = o.ndofs, o.neq, o.dim
    nsp, mw, z = mixture(ph)
    lay = capi.visualization_layout(ph, dim, bool(disc.axisymmetric))
    nvel = lay.nvel
    rows = np.zeros((lay.nrows, N))
    n_sp = np.zeros((nsp, N))
    src = np.zeros((neq, N))
    for i in range(N):
        u, up = np.ascontiguousarray(U[:, i]), np.ascontiguousarray(Up[:, i])
        gi = np.ascontiguousarray(g[:, :, i])  # gradUp[eq + d * neq]
        tb, V = o.flux_transport(u, gi)
        rows[lay.FluxTrns:lay.FluxTrns + 4, i] = tb
        for sp in range(nsp):
            for v in range(nvel):  # dataVis[diffVel + sp][n + v * ndofs] = diffVel[sp + v * numSpecies]
                rows[lay.diffVel + sp * nvel + v, i] = V[sp + v * nsp]
        sigma, mt, _, ns = o.source_transport(u, up, gi)
        rows[lay.SrcTrns, i] = sigma
        rows[lay.SpeciesTrns:lay.SpeciesTrns + nsp, i] = mt[:nsp]
        n_sp[:, i] = ns[:nsp]
        src[:, i] = o.source(u, up, gi)
    # computeSpeciesPrimitives (src/equation_of_state.cpp:882-927) from its number densities: X = n / sum n, Y = n M / rho
    if ph.mixture.ambipolar:  # the electron closure: n_e = sum_active Z n, not clamped here
        ne = (z[:nsp - 2, None] * n_sp[:nsp - 2]).sum(axis=0)
        assert np.abs(ne - n_sp[nsp - 2]).max() <= 4e-16 * np.abs(n_sp[nsp - 2]).max()
    rows[lay.nsp_:lay.nsp_ + nsp] = n_sp
    rows[lay.Xsp:lay.Xsp + nsp] = n_sp / n_sp.sum(axis=0)
    rows[lay.Ysp:lay.Ysp + nsp] = n_sp * mw[:, None] / U[0]
    Th = Up[nvel + 1]
    Te = Up[neq - 1] if ph.mixture.two_temperature else Th
    return dict(rows=rows, layout=lay, n_sp=n_sp, Th=Th, Te=Te, src=src, Up=Up, gradUp=g, oracle=o)


def rate_scale_and_closed_form(ph, n_sp, Th, Te):
    """(scale [R, N], q [R, N] or None per reaction).  scale = kf (prod n^nu' + prod n^nu'' / kC): the un-cancelled
    magnitude of the progress rate (the net value vanishes at equilibrium).  q: Chemistry's closed form for Arrhenius
    reactions, with its temperature floor (src/chemistry.cpp:161-299); None for the other rate laws (no numpy form here --
    kf is then taken from nowhere: scale is None too and the caller uses the species-source identity alone)."""
    ch = ph.chemistry
    re_, pr = stoichiometry(ph)
    R = ch.num_reactions
    Thl, Tel = np.maximum(Th, ch.minimum_temperature), np.maximum(Te, ch.minimum_temperature)
    scale, q = [], []
    for r in range(R):
        el = ch.electron_index >= 0 and re_[r, ch.electron_index] != 0
        T = Tel if el else Thl
        if ch.reaction_models[r] != capi.ARRHENIUS:
            scale.append(None)
            q.append(None)
            continue
        A, b, E = (ch.rate_params[k + r * capi.MAXCHEMPARAMS] for k in range(3))
        kf = A * T ** b * np.exp(-E / R_U / T)
        fwd = np.prod(n_sp ** re_[r][:, None], axis=0)
        bwd = 0.0
        if ch.detailed_balance[r]:
            kA, kb, kE = (ch.equilibrium_constant_params[k + r * capi.MAXCHEMPARAMS] for k in range(3))
            bwd = np.prod(n_sp ** pr[r][:, None], axis=0) / (kA * T ** kb * np.exp(-kE / T))
        scale.append(kf * (fwd + bwd))
        q.append(kf * (fwd - bwd))
    return scale, q


def species_source_identity(ph, nvel, q_rows, src):
    """(lhs, scale) [nactive, N]: lhs = M_sp sum_r (nu'' - nu') q_r must equal point_source's species rows; scale =
    M_sp sum_r |nu'' - nu'| |q_r|, the un-cancelled magnitude of that sum."""
    nsp, mw, _ = mixture(ph)
    re_, pr = stoichiometry(ph)
    nact = nsp - 2 if ph.mixture.ambipolar else nsp - 1
    d = (pr - re_).astype(float)  # [R, nsp]
    lhs = mw[:nact, None] * np.einsum("rs,rn->sn", d[:, :nact], q_rows)
    scale = mw[:nact, None] * np.einsum("rs,rn->sn", np.abs(d[:, :nact]), np.abs(q_rows))
    return lhs, scale, src[nvel + 2:nvel + 2 + nact]


def row_errors(got, ref, scale=None):
    """per row max_n |got - ref| / max_n scale (scale defaults to |ref|: the row's own magnitude).  A reference row that is
    identically zero (bulk viscosity, the azimuthal diffusion velocity, the electron's own frequency) admits only zeros."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    s = np.abs(ref) if scale is None else np.atleast_2d(scale)
    return np.abs(got - ref).max(axis=1) / np.maximum(s.max(axis=1), 1e-300)


def groups(lay):
    nsp, nvel, R = lay.num_species, lay.nvel, lay.num_reactions
    g = [("X_sp", lay.Xsp, nsp), ("Y_sp", lay.Ysp, nsp), ("n_sp", lay.nsp_, nsp), ("flux transport", lay.FluxTrns, 4),
         ("diff_vel", lay.diffVel, nsp * nvel), ("electric_cond", lay.SrcTrns, 1), ("mt_freq", lay.SpeciesTrns, nsp)]
    return g + ([("rxn_rate", lay.rxn, R)] if R else [])


def cold_state(case, t0=1500.0, dt=300.0):
    """A valid smooth state of an ambipolar ternary single-temperature mixture whose temperature lies BELOW Chemistry's
    minimum_temperature everywhere: the floor of the rate coefficients decides every rate."""
    ph = case.physics
    X = node_coordinates(case.mesh, case.disc.order, case.disc.basis_type)
    nvel = 3 if (case.disc.axisymmetric or X.shape[0] == 3) else 2
    nsp, mw, _ = mixture(ph)
    assert nsp == 3 and ph.mixture.ambipolar and not ph.mixture.two_temperature
    L = np.maximum(X.max(axis=1) - X.min(axis=1), 1e-12)
    w = np.sin(2 * np.pi * X[0] / L[0] + 0.3) * np.cos(2 * np.pi * X[1] / L[1] + 1.1)
    if X.shape[0] == 3:  # (every direction carries a gradient: no row of the diffusion velocities is rounding noise)
        w = w * np.cos(2 * np.pi * X[2] / L[2] + 0.2)
    Th = t0 + dt * w
    assert Th.max() < ph.chemistry.minimum_temperature
    alpha = 10.0 ** (-5.0 + w)
    nh = 101300.0 / (R_U * Th * (1.0 + alpha))
    ni = alpha * nh
    rho = ni * mw[0] + ni * mw[1] + (nh - ni) * mw[2]
    vel = [20.0 + w, 1.0 - w, 0.5 * w][:nvel]
    return cases.plasma_conserved(ph, nvel, rho, vel, Th, [ni], None)


def device_fields(case, U, op=None):
    """(fields dict of numpy arrays, the whole [nrows, NDofs] array) of RHSoperator.visualizationFields"""
    import torch

    from tps_amd.rhs_operator import RHSoperator

    own = op is None
    if own:
        op = RHSoperator(case.mesh, case.disc, case.physics, case.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    fields, arr = op.visualizationFields(x, return_array=True)
    torch.cuda.synchronize()
    out = ({k: v.cpu().numpy() for k, v in fields.items()}, arr.cpu().numpy())
    if own:
        op.close()
    return out


def raw_fields(op, x, out):
    """tpsrhs_visualization_fields straight through the C ABI into the caller's tensor -> status"""
    return op._lib.tpsrhs_visualization_fields(op._h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))


EPS = 2.0 ** -52  # the relative size of one unit in the last place, at most
# Bounds on device-minus-oracle, DERIVED from what tests/test_gpu_fastmath.py pins for fastmath.hpp (flog within 4 ulp of
# libm's logarithm, exp(c log x) within 4e-15 of libm's pow, fast_rcp / fast_sqrt within 2 ulp), not from what the kernels give.
#
# (a) An electron-argon collision integral, Q(x) = C0 / x + sum_{k=1..8} Ck x^(k-1) with x = log T_e.  The device's x is
#     within 4 ulp of libm's and the oracle's within 1: 5 EPS relative.  The term of x^(k-1) moves by at most (k-1) 5 EPS
#     <= 35 EPS of its size (C0 / x by 5 EPS, plus 2 ulp of the reciprocal); the powers are formed by k-1 <= 7 products and
#     one more with Ck, each rounded on both sides: 8 EPS; the nine terms are added one after the other, each partial sum
#     rounded on both sides and no larger than the sum of magnitudes: 8 EPS.  Together
#         |Q_device - Q_oracle| <= 51 EPS sum_k |Ck x^k| = 1.13e-14 sum_k |Ck x^k|.
POLY_BOUND = (35 + 8 + 8) * EPS
# (b) A Coulomb collision integral, pi lambda_D^2 c0 log(1 + c1 Tp^c2)^c3 / Tp^2 at a nondimensional temperature Tp >= 1
#     (asserted below).  Tp^c2 is a pinned pow: 4e-15, and so is w = 1 + c1 Tp^c2.  L = log w moves by dw / w <= 4e-15 and
#     by 4 ulp of the logarithm; c1 >= 1.24 for the fits the closures use, so w >= 2.24 and L >= 0.8: 4e-15 / 0.8 + 9e-16 =
#     5.9e-15 relative.  L^c3 with c3 <= 1.25 is a pinned pow again: 4e-15 + 1.25 x 5.9e-15.  1 / Tp^2 from a 2-ulp
#     reciprocal squared: 9e-16; the products and pi lambda_D^2 (a square root, a reciprocal): 2e-15; libm on the oracle's
#     side, one ulp per pow and log: 1e-15.  Together 1.5e-14 relative.
FIT_BOUND = 1.5e-14
PRODUCT_BOUND = 16 * EPS  # a product of a handful of factors, among them a 2-ulp square root and a 2-ulp reciprocal


@functools.lru_cache(maxsize=None)
def _e_ar_coefficients():
    """C[5][9] of the electron-argon collision integrals Q^(1,1..5): tests/golden/e_ar_collision_coefficients.txt"""
    c = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e_ar_collision_coefficients.txt"))
    assert c.shape == (5, 9)
    return c


def _e_ar_polynomials(Te, want=None):
    """(values [5][N], sums of the magnitudes of the terms [5][N]) of the five polynomials at T_e; `want`: the oracle's
    values, which the fixture must reproduce"""
    x = np.log(Te)
    val, mag = [], []
    for r, C in enumerate(_e_ar_coefficients()):
        terms = [C[0] / x] + [C[k] * x ** (k - 1) for k in range(1, 9)]
        val.append(sum(terms))
        mag.append(sum(np.abs(t) for t in terms))
        if want is not None:
            assert np.abs(val[r] / want[r] - 1.0).max() < 1e-9, "the fixture's polynomial is not the oracle's"
    return val, mag


def electron_conductivity_bound(ph, ref):
    """Bound [N] on |device - oracle| of thermal_cond_elec, or None where the closure has no cancellation (constant
    transport, first-order k_e: the plain bound of the other rows holds).  The third-order electron conductivity of the
    collision-integral models (src/gas_transport.cpp:400-489, 1388-1407) is  k_e = c sqrt(T_e) X_e / D,
    D = L11 - L12^2 / L22,  where every L is a sum over the collision partners of X_sp times a combination of up to five
    collision integrals with coefficients of both signs (L22 of an (e, heavy) pair: 19.14 Q1 - 91.875 Q2 + 199.5 Q3 - 210 Q4
    + 90 Q5), the electron-argon ones polynomials in log T_e whose terms cancel to 1e-5 of their sum of magnitudes.  With
    dQ the bound (a) or (b) above on each collision integral, and n_t the number of terms of an L (each addition rounded on
    both sides),
        dL_k <= sum_terms |coefficient X_sp| dQ + n_t EPS sum_terms |term|,
        dD   <= dL11 + 2 |L12 / L22| dL12 + (L12 / L22)^2 dL22 + 4 EPS (|L11| + L12^2 / |L22|),
        |d k_e| <= |k_e| (dD / |D| + PRODUCT_BOUND)        (first order in the small quantities).
    The collision integrals are the oracle's own (tpsoracle_collision_integral) at its Debye length; that D restates the
    oracle's denominator is asserted (k_e D / (sqrt(T_e) X_e) is one constant)."""
    from oracle_lib import collision_integral

    gt = ph.gas_transport
    if ph.transport_model == capi.CONSTANT or not gt.third_order_k_electron:
        return None
    nsp, _, z = mixture(ph)
    ie = nsp - 2
    n, Th, Te = ref["n_sp"], ref["Th"], ref["Te"]
    X = n / n.sum(axis=0)
    k_b = R_U / 6.0221409e23
    dfac = k_b * 8.8541878128e-12 / 1.60218e-19 ** 2
    eps = 1.0e-30
    if ph.transport_model == capi.ARGON_MINIMAL:
        n_over_t = (n[ie] + eps) / Te + (n[gt.ion_index] + eps) / Th
    else:
        n_over_t = ((n + eps) * (z ** 2)[:, None]).sum(axis=0) / Te
    length = np.sqrt(dfac / 6.0221409e23 / n_over_t)
    circle, nd_te = np.pi * length ** 2, length * 4.0 * np.pi * dfac * Te
    assert nd_te.min() >= 1.0  # (b) above
    fit = lambda name, x: np.array([collision_integral(name, float(v)) for v in x])
    q2 = [fit(f"rep2{r}", nd_te) * circle for r in (2, 3, 4)]
    qi = [fit(f"att1{r}", nd_te) * circle for r in (1, 2, 3, 4, 5)]
    qn = [fit(f"eAr1{r}", Te) for r in (1, 2, 3, 4, 5)]
    _, qn_mag = _e_ar_polynomials(Te, want=qn)
    dq2 = [FIT_BOUND * np.abs(q) for q in q2]
    dqi = [FIT_BOUND * np.abs(q) for q in qi]
    dqn = [POLY_BOUND * m for m in qn_mag]
    ee = ((1.0,), (1.75, -2.0), (4.8125, -7.0, 5.0))
    ea = ((6.25, -15.0, 12.0), (10.9375, -39.375, 57.0, -30.0), (19.140625, -91.875, 199.5, -210.0, 90.0))
    L, dL = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for k in range(3):
        terms = [np.sqrt(2.0) * X[ie] * c * q for c, q in zip(ee[k], q2)]
        moved = [np.abs(np.sqrt(2.0) * X[ie] * c) * d for c, d in zip(ee[k], dq2)]
        for sp in range(nsp):
            if sp != ie:
                terms += [X[sp] * c * q for c, q in zip(ea[k], qi if z[sp] != 0 else qn)]
                moved += [np.abs(X[sp] * c) * d for c, d in zip(ea[k], dqi if z[sp] != 0 else dqn)]
        L[k] = sum(terms)
        dL[k] = sum(moved) + len(terms) * EPS * sum(np.abs(t) for t in terms)
    ratio = L[1] / L[2]
    D = L[0] - L[1] * ratio
    dD = dL[0] + 2.0 * np.abs(ratio) * dL[1] + ratio ** 2 * dL[2] + 4.0 * EPS * (np.abs(L[0]) + np.abs(L[1] * ratio))
    ke = ref["rows"][ref["layout"].FluxTrns + 3]
    shape = ke * D / (np.sqrt(Te) * X[ie])  # = the constant c if D restates the oracle's denominator
    assert np.abs(shape / shape[0] - 1.0).max() < 1e-9, "the restated denominator is not the oracle's"
    return np.abs(ke) * (dD / np.abs(D) + PRODUCT_BOUND)


def momentum_transfer_bound(ph, ref):
    """Bound [nsp, N] on |device - oracle| of the momentum-transfer frequencies of the NEUTRAL species (NaN in the other
    rows, which keep the plain bound), or None (constant transport).  The frequency of a neutral species is
    sqrt(T_e / m_e) n_sp Q^(1,1)_e-Ar(T_e) times constants: with (a) above for the polynomial and PRODUCT_BOUND for the
    factors around it,  |d nu| <= |nu| (POLY_BOUND sum_k |C_1k x^k| / |Q| + PRODUCT_BOUND)."""
    if ph.transport_model == capi.CONSTANT:
        return None
    nsp, _, z = mixture(ph)
    lay = ref["layout"]
    mt = np.abs(ref["rows"][lay.SpeciesTrns:lay.SpeciesTrns + nsp])
    val, mag = _e_ar_polynomials(ref["Te"])
    bound = np.full(mt.shape, np.nan)
    for sp in range(nsp):
        if sp != nsp - 2 and z[sp] == 0:
            bound[sp] = mt[sp] * (POLY_BOUND * mag[0] / np.abs(val[0]) + PRODUCT_BOUND)
    return bound
