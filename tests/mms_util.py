"""Manufactured solution of the compressible Navier-Stokes equations on a periodic box, differentiated
symbolically (sympy): the exact right-hand side  dU/dt = -div(F_c(U) - F_v(U, grad U))  of a smooth periodic
state, with the reference's closures (gamma-law gas, Sutherland viscosity, bulk viscosity multiplier, Prandtl
number: SURVEY.md appendix A.2, A.4, A.5).  Independent of the oracle and of the kernels: the order-of-accuracy
tests compare both with the PDE itself (the role of the reference's MASA-based mms.*.test, whose library is
not available here)."""
import functools

import numpy as np

GAMMA, RG, C1, S0, PR = 1.4, 287.058, 1.458e-6, 110.4, 0.71


@functools.lru_cache(maxsize=None)
def _build(dim, viscous, visc_mult, bulk_mult, lengths):
    import sympy as sp

    X = sp.symbols("x y z")[:dim]
    k = [2 * sp.pi / L for L in lengths]
    # smooth periodic primitives, bounded away from zero
    rho = 1.2 + 0.10 * sp.sin(k[0] * X[0]) * sp.cos(k[1] * X[1]) + (0.05 * sp.sin(k[2] * X[2]) if dim == 3 else 0)
    vel = [30.0 + 8.0 * sp.sin(k[0] * X[0] + 0.3) * sp.cos(k[1] * X[1]),
           -12.0 + 6.0 * sp.cos(k[0] * X[0]) * sp.sin(k[1] * X[1] + 0.5)]
    if dim == 3:
        vel[0] += 3.0 * sp.cos(k[2] * X[2])
        vel.append(7.0 + 5.0 * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[0] * X[0]))
    p = 101300.0 * (1 + 0.04 * sp.cos(k[0] * X[0] - 0.4) * sp.sin(k[1] * X[1]) + (0.02 * sp.cos(k[2] * X[2]) if dim == 3 else 0))
    T = p / (rho * RG)
    E = p / (GAMMA - 1) + rho * sum(v * v for v in vel) / 2
    U = [rho] + [rho * v for v in vel] + [E]
    F = [[U[0] * vel[d] for d in range(dim)]]
    for i in range(dim):
        F.append([U[1 + i] * vel[d] + (p if i == d else 0) for d in range(dim)])
    F.append([vel[d] * (E + p) for d in range(dim)])
    if viscous:
        mu = C1 * visc_mult * T ** sp.Rational(3, 2) / (T + S0)
        mub = bulk_mult * mu - sp.Rational(2, 3) * mu
        kap = mu * GAMMA * RG / ((GAMMA - 1) * PR)
        div = sum(sp.diff(vel[d], X[d]) for d in range(dim))
        tau = [[mu * (sp.diff(vel[i], X[j]) + sp.diff(vel[j], X[i])) + (mub * div if i == j else 0) for j in range(dim)]
               for i in range(dim)]
        for i in range(dim):
            for d in range(dim):
                F[1 + i][d] -= tau[i][d]
        for d in range(dim):
            F[dim + 1][d] -= sum(tau[i][d] * vel[i] for i in range(dim)) + kap * sp.diff(T, X[d])
    rhs = [-sum(sp.diff(F[eq][d], X[d]) for d in range(dim)) for eq in range(dim + 2)]
    return sp.lambdify(X, U, "numpy"), sp.lambdify(X, rhs, "numpy")


def manufactured(X, viscous=True, visc_mult=1.0, bulk_mult=0.0, lengths=(1.0, 1.0, 1.0)):
    """X: node coordinates (dim, N) -> (U, exact dU/dt), both (dim + 2, N)"""
    dim = X.shape[0]
    fu, fr = _build(dim, bool(viscous), float(visc_mult), float(bulk_mult), tuple(lengths[:dim]))
    bc = np.zeros(X.shape[1])
    U = np.array([np.asarray(v, dtype=np.float64) + bc for v in fu(*X)])
    R = np.array([np.asarray(v, dtype=np.float64) + bc for v in fr(*X)])
    return U, R


def observed_order(err_coarse, err_fine):
    return np.log2(np.asarray(err_coarse) / np.asarray(err_fine))


@functools.lru_cache(maxsize=None)
def _build_axisym(visc_mult, bulk_mult, lz):
    """Compressible Navier-Stokes in cylindrical coordinates (r, z) with swirl; state order of the reference's
    axisymmetric formulation: rho, rho u_r, rho u_z, rho u_theta, rho E."""
    import sympy as sp

    r, z = sp.symbols("r z", positive=True)
    k = 2 * sp.pi / lz
    rho = 1.2 + 0.10 * sp.sin(k * z) * sp.cos(9.0 * r) + 0.05 * sp.sin(14.0 * r)
    ur = 4.0 * sp.sin(11.0 * r) * sp.cos(k * z + 0.3)
    uz = 30.0 + 8.0 * sp.cos(8.0 * r) * sp.sin(k * z)
    ut = 6.0 * sp.sin(7.0 * r + 0.4) * (1 + 0.3 * sp.cos(k * z))
    p = 101300.0 * (1 + 0.04 * sp.cos(10.0 * r - 0.4) * sp.sin(k * z))
    T = p / (rho * RG)
    E = p / (GAMMA - 1) + rho * (ur * ur + uz * uz + ut * ut) / 2
    mu = C1 * visc_mult * T ** sp.Rational(3, 2) / (T + S0)
    mub = bulk_mult * mu - sp.Rational(2, 3) * mu
    kap = mu * GAMMA * RG / ((GAMMA - 1) * PR)
    div = sp.diff(r * ur, r) / r + sp.diff(uz, z)
    trr = 2 * mu * sp.diff(ur, r) + mub * div
    tzz = 2 * mu * sp.diff(uz, z) + mub * div
    ttt = 2 * mu * ur / r + mub * div
    trz = mu * (sp.diff(ur, z) + sp.diff(uz, r))
    trt = mu * (sp.diff(ut, r) - ut / r)
    tzt = mu * sp.diff(ut, z)

    def dv(fr, fz):  # divergence of an (r, z) flux in cylindrical coordinates
        return sp.diff(r * fr, r) / r + sp.diff(fz, z)

    rhs = [-dv(rho * ur, rho * uz),
           -dv(rho * ur * ur + p - trr, rho * ur * uz - trz) + (p - ttt + rho * ut * ut) / r,
           -dv(rho * ur * uz - trz, rho * uz * uz + p - tzz),
           -dv(rho * ur * ut - trt, rho * uz * ut - tzt) - (rho * ur * ut - trt) / r,
           -dv(ur * (E + p) - (trr * ur + trz * uz + trt * ut) - kap * sp.diff(T, r),
               uz * (E + p) - (trz * ur + tzz * uz + tzt * ut) - kap * sp.diff(T, z))]
    U = [rho, rho * ur, rho * uz, rho * ut, E]
    return sp.lambdify((r, z), U, "numpy"), sp.lambdify((r, z), rhs, "numpy")


def manufactured_axisym(X, visc_mult=1.0, bulk_mult=0.0, lz=1.0):
    """X: (r, z) node coordinates (2, N) -> (U, exact dU/dt), both (5, N)"""
    fu, fr = _build_axisym(float(visc_mult), float(bulk_mult), float(lz))
    bc = np.zeros(X.shape[1])
    U = np.array([np.asarray(v, dtype=np.float64) + bc for v in fu(X[0], X[1])])
    R = np.array([np.asarray(v, dtype=np.float64) + bc for v in fr(X[0], X[1])])
    return U, R


@functools.lru_cache(maxsize=None)
def _build_ternary(dim, lengths):
    """Inviscid, frozen, single-temperature ambipolar ternary plasma (Ar.+1, E, Ar): PerfectMixture closure of
    SURVEY.md appendix A.3 -- n_e = n_i, p = R (n_i + n_e + n_B) T, rho E = sum n c_v T + n_i E_f + rho |u|^2 / 2 --
    state rho, rho u, rho E, rho Y_ion."""
    import sympy as sp

    R_U = 8.3144598
    m_ar, m_e, e_form, cv = 39.948e-3, 5.4858e-7, 1520571.3883, 1.5 * R_U
    m_i = m_ar - m_e
    X = sp.symbols("x y z")[:dim]
    k = [2 * sp.pi / L for L in lengths]
    T = 8000.0 * (1 + 0.10 * sp.sin(k[0] * X[0]) * sp.cos(k[1] * X[1]))
    nB = 1.4 * (1 + 0.08 * sp.cos(k[0] * X[0] + 0.2) * sp.sin(k[1] * X[1]) + (0.04 * sp.sin(k[2] * X[2]) if dim == 3 else 0))
    ni = 2.0e-3 * (1 + 0.30 * sp.sin(k[0] * X[0] - 0.5) * sp.sin(k[1] * X[1] + 0.1))
    vel = [300.0 + 60.0 * sp.sin(k[0] * X[0] + 0.3) * sp.cos(k[1] * X[1]), -100.0 + 40.0 * sp.cos(k[0] * X[0]) * sp.sin(k[1] * X[1])]
    if dim == 3:
        vel.append(50.0 + 30.0 * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[0] * X[0]))
    ne = ni
    rho = m_i * ni + m_e * ne + m_ar * nB
    p = R_U * (ni + ne + nB) * T
    E = cv * (ni + ne + nB) * T + e_form * ni + rho * sum(v * v for v in vel) / 2
    U = [rho] + [rho * v for v in vel] + [E, m_i * ni]
    rhs = [-sum(sp.diff(U[0] * vel[d], X[d]) for d in range(dim))]
    for i in range(dim):
        rhs.append(-sum(sp.diff(U[1 + i] * vel[d] + (p if i == d else 0), X[d]) for d in range(dim)))
    rhs.append(-sum(sp.diff(vel[d] * (E + p), X[d]) for d in range(dim)))
    rhs.append(-sum(sp.diff(m_i * ni * vel[d], X[d]) for d in range(dim)))
    return sp.lambdify(X, U, "numpy"), sp.lambdify(X, rhs, "numpy")


def manufactured_ternary(X, lengths=(1.0, 1.0, 1.0)):
    dim = X.shape[0]
    fu, fr = _build_ternary(dim, tuple(lengths[:dim]))
    bc = np.zeros(X.shape[1])
    U = np.array([np.asarray(v, dtype=np.float64) + bc for v in fu(*X)])
    R = np.array([np.asarray(v, dtype=np.float64) + bc for v in fr(*X)])
    return U, R


# ---------------------------------------------------------------------------------------------------------------
# Manufactured states that satisfy a boundary condition EXACTLY on planar patches (tests/test_mms_boundaries.py): the
# weak boundary flux of such a state is consistent with the PDE, so the residual of the elements next to the patch
# converges to the same exact right-hand side at the same order as the interior's.
#   walls at y = 0 and y = L_y (x, z periodic):  s = sin(pi y / L_y) vanishes on both, c = cos(pi y / L_y) has
#   a vanishing y-derivative on both;
#   inlet at x = 0, outlet at x = L_x (y, z periodic):  a = sin(pi x / 2 L_x) vanishes at the inlet, b = cos(pi x / 2 L_x)
#   at the outlet.
# The data of the patches that go with the states:
BC_WALL_TEMPERATURE = 300.0  # VISC_ISOTH
BC_DRY_INLET = (1.2, 30.0, -12.0, 7.0)  # SUB_DENS_VEL: rho, u, v, w
BC_DRY_OUTLET_PRESSURE = 101300.0  # SUB_P
_TERNARY_M_AR, _TERNARY_M_E, _TERNARY_R_U = 39.948e-3, 5.4858e-7, 8.3144598
_TERNARY_N_ION_IN, _TERNARY_N_B_IN, _TERNARY_T_REF = 2.0e-3, 1.4, 8000.0
# SUB_DENS_VEL of the ternary: rho, u, v, w, rho Y_ion  (n_e = n_i: rho = m_Ar (n_i + n_B))
BC_TERNARY_INLET = (_TERNARY_M_AR * (_TERNARY_N_ION_IN + _TERNARY_N_B_IN), 300.0, -100.0, 50.0,
                    (_TERNARY_M_AR - _TERNARY_M_E) * _TERNARY_N_ION_IN)
BC_TERNARY_OUTLET_PRESSURE = _TERNARY_R_U * (2 * _TERNARY_N_ION_IN + _TERNARY_N_B_IN) * _TERNARY_T_REF
BC_KINDS = ("isoth", "adiab", "slip", "inout")


def _dry_air_rhs(sp, X, rho, vel, p, viscous, visc_mult, bulk_mult):
    """(U, -div(F_c - F_v)) of the primitives rho, vel, p: the closures of `_build`"""
    dim = len(X)
    T = p / (rho * RG)
    E = p / (GAMMA - 1) + rho * sum(v * v for v in vel) / 2
    U = [rho] + [rho * v for v in vel] + [E]
    F = [[U[0] * vel[d] for d in range(dim)]]
    for i in range(dim):
        F.append([U[1 + i] * vel[d] + (p if i == d else 0) for d in range(dim)])
    F.append([vel[d] * (E + p) for d in range(dim)])
    if viscous:
        mu = C1 * visc_mult * T ** sp.Rational(3, 2) / (T + S0)
        mub = bulk_mult * mu - sp.Rational(2, 3) * mu
        kap = mu * GAMMA * RG / ((GAMMA - 1) * PR)
        div = sum(sp.diff(vel[d], X[d]) for d in range(dim))
        tau = [[mu * (sp.diff(vel[i], X[j]) + sp.diff(vel[j], X[i])) + (mub * div if i == j else 0) for j in range(dim)]
               for i in range(dim)]
        for i in range(dim):
            for d in range(dim):
                F[1 + i][d] -= tau[i][d]
        for d in range(dim):
            F[dim + 1][d] -= sum(tau[i][d] * vel[i] for i in range(dim)) + kap * sp.diff(T, X[d])
    return U, [-sum(sp.diff(F[eq][d], X[d]) for d in range(dim)) for eq in range(dim + 2)]


@functools.lru_cache(maxsize=None)
def _build_bc(dim, kind, viscous, visc_mult, bulk_mult, lengths):
    """Dry air; kind:
    "isoth"  every velocity component ~ s, T = T_w + (...) s, p free, rho = p / (R T): the VISC_ISOTH wall state;
    "adiab"  velocities ~ s, T depends on y through c only (dT/dy = 0 on the walls): VISC_ADIAB;
    "slip"   v ~ s, everything else mixes c and s so that nothing else vanishes on the walls: SLIP / INV with Euler;
    "inout"  rho and the velocities leave their SUB_DENS_VEL data through a, p leaves its SUB_P datum through b."""
    import sympy as sp

    X = sp.symbols("x y z")[:dim]
    k = [2 * sp.pi / L for L in lengths]
    z3 = dim == 3
    if kind == "inout":
        a, b = sp.sin(sp.pi * X[0] / (2 * lengths[0])), sp.cos(sp.pi * X[0] / (2 * lengths[0]))
        r0, u0, v0, w0 = BC_DRY_INLET
        rho = r0 + 0.10 * a * sp.cos(k[1] * X[1]) + (0.05 * a * sp.sin(k[2] * X[2]) if z3 else 0)
        vel = [u0 + 8.0 * a * sp.cos(k[1] * X[1] + 0.3) + (3.0 * a * sp.cos(k[2] * X[2]) if z3 else 0),
               v0 + 6.0 * a * sp.sin(k[1] * X[1] + 0.5)]
        if z3:
            vel.append(w0 + 5.0 * a * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[1] * X[1]))
        p = BC_DRY_OUTLET_PRESSURE * (1 + 0.04 * b * sp.sin(k[1] * X[1] - 0.4) + (0.02 * b * sp.cos(k[2] * X[2]) if z3 else 0))
    else:
        s, c = sp.sin(sp.pi * X[1] / lengths[1]), sp.cos(sp.pi * X[1] / lengths[1])
        p = 101300.0 * (1 + 0.04 * sp.cos(k[0] * X[0] - 0.4) * (0.5 * c + 0.6 * s) + (0.02 * sp.cos(k[2] * X[2]) if z3 else 0))
        if kind == "slip":
            vel = [30.0 + 8.0 * sp.sin(k[0] * X[0] + 0.3) * (0.6 * c + 0.5 * s) + (3.0 * sp.cos(k[2] * X[2]) if z3 else 0),
                   (-12.0 + 6.0 * sp.cos(k[0] * X[0])) * s]
            if z3:
                vel.append(7.0 + 5.0 * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[0] * X[0]) * (0.7 * c - 0.4 * s))
            rho = 1.2 + 0.10 * sp.sin(k[0] * X[0]) * (0.7 * c + 0.4 * s) + (0.05 * sp.sin(k[2] * X[2]) if z3 else 0)
        else:
            vel = [(30.0 + 8.0 * sp.sin(k[0] * X[0] + 0.3) + (3.0 * sp.cos(k[2] * X[2]) if z3 else 0)) * s,
                   (-12.0 + 6.0 * sp.cos(k[0] * X[0])) * s]
            if z3:
                vel.append((7.0 + 5.0 * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[0] * X[0])) * s)
            if kind == "isoth":
                T = BC_WALL_TEMPERATURE + (40.0 + 15.0 * sp.sin(k[0] * X[0]) + (8.0 * sp.sin(k[2] * X[2]) if z3 else 0)) * s
            elif kind == "adiab":
                T = 300.0 * (1 + 0.08 * sp.sin(k[0] * X[0]) * c + (0.03 * sp.sin(k[2] * X[2]) if z3 else 0))
            else:
                raise ValueError(kind)
            rho = p / (RG * T)
    U, rhs = _dry_air_rhs(sp, X, rho, vel, p, viscous, visc_mult, bulk_mult)
    return sp.lambdify(X, U, "numpy"), sp.lambdify(X, rhs, "numpy")


def manufactured_bc(X, kind, viscous=True, visc_mult=1.0, bulk_mult=0.0, lengths=(1.0, 1.0, 1.0)):
    """X: node coordinates (dim, N) -> (U, exact dU/dt) of the dry-air state that satisfies the boundary condition `kind`"""
    dim = X.shape[0]
    fu, fr = _build_bc(dim, kind, bool(viscous), float(visc_mult), float(bulk_mult), tuple(lengths[:dim]))
    bc = np.zeros(X.shape[1])
    U = np.array([np.asarray(v, dtype=np.float64) + bc for v in fu(*X)])
    R = np.array([np.asarray(v, dtype=np.float64) + bc for v in fr(*X)])
    return U, R


@functools.lru_cache(maxsize=None)
def _build_ternary_bc(dim, kind, lengths):
    """The closure of `_build_ternary` with kind = "slip" (inviscid walls at y = 0, L_y) or "inout" (rho, the velocities and
    the ion partial density leave the SUB_DENS_VEL data through a, p its SUB_P datum through b, T from the equation of
    state)."""
    import sympy as sp

    R_U, m_ar, m_e = _TERNARY_R_U, _TERNARY_M_AR, _TERNARY_M_E
    e_form, cv = 1520571.3883, 1.5 * R_U
    m_i = m_ar - m_e
    X = sp.symbols("x y z")[:dim]
    k = [2 * sp.pi / L for L in lengths]
    z3 = dim == 3
    if kind == "inout":
        a, b = sp.sin(sp.pi * X[0] / (2 * lengths[0])), sp.cos(sp.pi * X[0] / (2 * lengths[0]))
        r0, u0, v0, w0, ri0 = BC_TERNARY_INLET
        rho = r0 * (1 + 0.08 * a * sp.cos(k[1] * X[1] + 0.2) + (0.04 * a * sp.sin(k[2] * X[2]) if z3 else 0))
        ni = ri0 / m_i * (1 + 0.30 * a * sp.sin(k[1] * X[1] + 0.1))
        vel = [u0 + 60.0 * a * sp.cos(k[1] * X[1] + 0.3), v0 + 40.0 * a * sp.sin(k[1] * X[1])]
        if z3:
            vel.append(w0 + 30.0 * a * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[1] * X[1]))
        p = BC_TERNARY_OUTLET_PRESSURE * (1 + 0.10 * b * sp.sin(k[1] * X[1] - 0.4) + (0.03 * b * sp.cos(k[2] * X[2]) if z3 else 0))
        nB = (rho - (m_i + m_e) * ni) / m_ar
        T = p / (R_U * (2 * ni + nB))
    elif kind == "slip":
        s, c = sp.sin(sp.pi * X[1] / lengths[1]), sp.cos(sp.pi * X[1] / lengths[1])
        T = _TERNARY_T_REF * (1 + 0.10 * sp.sin(k[0] * X[0]) * (0.6 * c + 0.5 * s))
        nB = 1.4 * (1 + 0.08 * sp.cos(k[0] * X[0] + 0.2) * (0.5 * c + 0.6 * s) + (0.04 * sp.sin(k[2] * X[2]) if z3 else 0))
        ni = 2.0e-3 * (1 + 0.30 * sp.sin(k[0] * X[0] - 0.5) * (0.7 * c + 0.4 * s))
        vel = [300.0 + 60.0 * sp.sin(k[0] * X[0] + 0.3) * (0.6 * c + 0.5 * s), (-100.0 + 40.0 * sp.cos(k[0] * X[0])) * s]
        if z3:
            vel.append(50.0 + 30.0 * sp.sin(k[2] * X[2] + 0.2) * sp.cos(k[0] * X[0]) * (0.7 * c - 0.4 * s))
        p = R_U * (2 * ni + nB) * T
        rho = (m_i + m_e) * ni + m_ar * nB
    else:
        raise ValueError(kind)
    E = cv * (2 * ni + nB) * T + e_form * ni + rho * sum(v * v for v in vel) / 2
    U = [rho] + [rho * v for v in vel] + [E, m_i * ni]
    rhs = [-sum(sp.diff(U[0] * vel[d], X[d]) for d in range(dim))]
    for i in range(dim):
        rhs.append(-sum(sp.diff(U[1 + i] * vel[d] + (p if i == d else 0), X[d]) for d in range(dim)))
    rhs.append(-sum(sp.diff(vel[d] * (E + p), X[d]) for d in range(dim)))
    rhs.append(-sum(sp.diff(m_i * ni * vel[d], X[d]) for d in range(dim)))
    return sp.lambdify(X, U, "numpy"), sp.lambdify(X, rhs, "numpy")


def manufactured_ternary_bc(X, kind, lengths=(1.0, 1.0, 1.0)):
    dim = X.shape[0]
    fu, fr = _build_ternary_bc(dim, kind, tuple(lengths[:dim]))
    bc = np.zeros(X.shape[1])
    U = np.array([np.asarray(v, dtype=np.float64) + bc for v in fu(*X)])
    R = np.array([np.asarray(v, dtype=np.float64) + bc for v in fr(*X)])
    return U, R


# ---------------------------------------------------------------------------------------------------------------
# The reference's own manufactured-solution checks of ONE assembled Mult: utils/compute_rhs (utils/compute_rhs.cpp:
# 102-160) behind test/mms.euler_2d.test and test/mms.cns_2d.test.  The exact state and its source come from MASA
# [third party: pecos/MASA 0.50, absent from this image]; they are restated here from MASA's published forms and
# differentiated with sympy.
#
# euler_2d (MASA src/euler.cpp, documented in MASA's "Euler 2D" manufactured solution):
#     rho = rho_0 + rho_x sin(a_rhox pi x / L) + rho_y cos(a_rhoy pi y / L)
#     u   = u_0   + u_x   sin(a_ux   pi x / L) + u_y   cos(a_uy   pi y / L)
#     v   = v_0   + v_x   cos(a_vx   pi x / L) + v_y   sin(a_vy   pi y / L)
#     p   = p_0   + p_x   cos(a_px   pi x / L) + p_y   sin(a_py   pi y / L)
# Parameters: the reference sets L, Gamma and the eight a_* (src/masa_handler.cpp:236-262); the twelve amplitudes
# keep MASA's defaults (euler_2d<Scalar>::init_var).  MASA's sources are not here, so the defaults below are written
# from memory of that file -- NOT tuned: they were typed once, and the first evaluation reproduced the three numbers
# test/mms.euler_2d.test holds (5.74794e-5 / 5.75172e-5 / 5.7516e-5) to all six printed digits, which is the check on
# the recollection.
MASA_EULER_2D_DEFAULTS = dict(u_0=200.23, u_x=1.1, u_y=1.08, v_0=1.2, v_x=1.6, v_y=0.47, rho_0=100.02, rho_x=2.22, rho_y=0.8,
                              p_0=150.2, p_x=0.91, p_y=0.623, a_px=0.165, a_py=0.612, a_rhox=1.0, a_rhoy=1.0, a_ux=0.1987,
                              a_uy=1.189, a_vx=1.91, a_vy=1.0, Gamma=1.01, mu=0.918, L=3.02)
# src/masa_handler.cpp:245-261 (initEuler2D)
TPS_EULER_2D_OVERRIDES = dict(L=3.02, Gamma=1.4, a_rhox=2.0, a_rhoy=2.0, a_ux=2.0, a_uy=2.0, a_vx=2.0, a_vy=2.0, a_px=2.0, a_py=2.0)
# src/masa_handler.cpp:273-300 (initCNS2DSutherlands) with the input's viscosity multipliers (defaults 1, 0:
# src/M2ulPhyS.cpp:2678-2679)
TPS_CNS_2D_OVERRIDES = dict(L=3.02, Gamma=1.4, R=287.058, Pr=0.71, Amu=1.458e-6, Bmu=1.5, Cmu=110.4, bulkViscMult=0.0,
                            rho_0=1.02, rho_x=0.11, rho_y=0.13, a_rhox=2.0, a_rhoy=2.0, a_ux=2.0, a_uy=2.0, a_vx=2.0, a_vy=2.0,
                            a_px=2.0, a_py=2.0)


@functools.lru_cache(maxsize=None)
def _build_masa_2d(items, viscous):
    import sympy as sp

    P = dict(items)
    x, y = sp.symbols("x y")
    L, pi = P["L"], sp.pi
    rho = P["rho_0"] + P["rho_x"] * sp.sin(P["a_rhox"] * pi * x / L) + P["rho_y"] * sp.cos(P["a_rhoy"] * pi * y / L)
    u = P["u_0"] + P["u_x"] * sp.sin(P["a_ux"] * pi * x / L) + P["u_y"] * sp.cos(P["a_uy"] * pi * y / L)
    v = P["v_0"] + P["v_x"] * sp.cos(P["a_vx"] * pi * x / L) + P["v_y"] * sp.sin(P["a_vy"] * pi * y / L)
    p = P["p_0"] + P["p_x"] * sp.cos(P["a_px"] * pi * x / L) + P["p_y"] * sp.sin(P["a_py"] * pi * y / L)
    g = P["Gamma"]
    E = p / (g - 1) + rho * (u * u + v * v) / 2
    vel, X = [u, v], [x, y]
    U = [rho, rho * u, rho * v, E]
    F = [[rho * vel[d] for d in range(2)]]
    for i in range(2):
        F.append([U[1 + i] * vel[d] + (p if i == d else 0) for d in range(2)])
    F.append([vel[d] * (E + p) for d in range(2)])
    if viscous:  # Sutherland law mu = Amu T^Bmu / (T + Cmu), kappa = mu cp / Pr, bulk viscosity multiplier
        T = p / (rho * P["R"])
        mu = P["Amu"] * T ** P["Bmu"] / (T + P["Cmu"])
        mub = P["bulkViscMult"] * mu - sp.Rational(2, 3) * mu
        kap = mu * g * P["R"] / ((g - 1) * P["Pr"])
        div = sum(sp.diff(vel[d], X[d]) for d in range(2))
        tau = [[mu * (sp.diff(vel[i], X[j]) + sp.diff(vel[j], X[i])) + (mub * div if i == j else 0) for j in range(2)]
               for i in range(2)]
        for i in range(2):
            for d in range(2):
                F[1 + i][d] -= tau[i][d]
        for d in range(2):
            F[3][d] -= sum(tau[i][d] * vel[i] for i in range(2)) + kap * sp.diff(T, X[d])
    S = [sum(sp.diff(F[k][d], X[d]) for d in range(2)) for k in range(4)]  # MASA's source: Q = div F(U_exact)
    return sp.lambdify((x, y), U, "numpy"), sp.lambdify((x, y), S, "numpy")


def masa_2d(X, overrides, viscous=False):
    """(U_exact, Q) at the nodes X (2, N): the state of masa_eval_exact_* as src/masa_handler.cpp:219-238 assembles it
    and the source of masa_eval_source_* the MASA forcing adds to the residual (src/forcing_terms.cpp:979-1011)."""
    P = dict(MASA_EULER_2D_DEFAULTS)
    P.update(overrides)
    fu, fs = _build_masa_2d(tuple(sorted(P.items())), bool(viscous))
    z = np.zeros(X.shape[1])
    U = np.array([np.asarray(a, dtype=np.float64) + z for a in fu(X[0], X[1])])
    S = np.array([np.asarray(a, dtype=np.float64) + z for a in fs(X[0], X[1])])
    return U, S


def compute_rhs_errors(l2_norm, y, S):
    """utils/compute_rhs.cpp:134-147 with compare_rhs = False: per variable (density, momentum vector, energy) the L2
    norm of Mult(U_exact) -- which already contains the MASA forcing -- over the L2 norm of the forcing."""
    e0 = l2_norm(y[0]) / l2_norm(S[0])
    e1 = np.hypot(l2_norm(y[1]), l2_norm(y[2])) / np.hypot(l2_norm(S[1]), l2_norm(S[2]))
    e2 = l2_norm(y[3]) / l2_norm(S[3])
    return e0, e1, e2


# ---------------------------------------------------------------------------------------------------------------
# test/mms.euler.test: the transient 3-D Euler solution `euler_transient_3d` (MASA [third party, absent]) run for 300 / 600
# RK4 steps on periodic-cube.mesh refined once / twice, p = 1, basisType = integrationRule = 0 (test/inputs/
# mms.euler.3d.r1.ini, r2.ini); the test holds the convergence RATES of the density / velocity / pressure errors.
# EVERY parameter of the solution is set by the reference (src/masa_handler.cpp:356-417, below); the form is MASA's:
#     rho = rho_0 + rho_x sin(a_rhox pi x/L) + rho_y cos(a_rhoy pi y/L) + rho_z sin(a_rhoz pi z/L) + rho_t sin(a_rhot pi t/L)
#     u   = u_0   + u_x   sin(a_ux   pi x/L) + u_y   cos(a_uy   pi y/L) + u_z   cos(a_uz   pi z/L) + u_t   cos(a_ut   pi t/L)
#     v   = v_0   + v_x   cos(a_vx   pi x/L) + v_y   sin(a_vy   pi y/L) + v_z   sin(a_vz   pi z/L) + v_t   sin(a_vt   pi t/L)
#     w   = w_0   + w_x   sin(a_wx   pi x/L) + w_y   sin(a_wy   pi y/L) + w_z   cos(a_wz   pi z/L) + w_t   cos(a_wt   pi t/L)
#     p   = p_0   + p_x   cos(a_px   pi x/L) + p_y   sin(a_py   pi y/L) + p_z   cos(a_pz   pi z/L) + p_t   cos(a_pt   pi t/L)
# (the spatial part is MASA's published euler_3d, the time terms follow its euler_transient_1d; `forms` = one letter
# s / c per variable for the TIME term, so that tools/mms_euler_transient.py can run the family -- the default is the
# form above).
TPS_EULER_TRANSIENT_3D = dict(
    Gamma=1.4, L=2.0,
    rho_0=1.0, rho_x=0.1, rho_y=0.1, rho_z=0.0, rho_t=0.15, u_0=130.0, u_x=10.0, u_y=5.0, u_z=0.0, u_t=10.0,
    v_0=5.0, v_x=1.0, v_y=-1.0, v_z=0.0, v_t=2.0, w_0=0.0, w_x=2.0, w_y=1.0, w_z=0.0, w_t=-1.0,
    p_0=101300.0, p_x=101.0, p_y=101.0, p_z=0.0, p_t=1013.0,
    a_rhox=2.0, a_rhoy=2.0, a_rhoz=0.0, a_rhot=400.0, a_ux=2.0, a_uy=2.0, a_uz=0.0, a_ut=400.0,
    a_vx=2.0, a_vy=2.0, a_vz=0.0, a_vt=400.0, a_wx=2.0, a_wy=2.0, a_wz=0.0, a_wt=0.0,
    a_px=2.0, a_py=2.0, a_pz=0.0, a_pt=400.0)


class _Transient3D:
    def __init__(self, fprim, fstate, fsource):
        self._fp, self._fu, self._fs = fprim, fstate, fsource

    @staticmethod
    def _eval(f, X, t):
        z = np.zeros(X.shape[1])
        return np.array([np.asarray(a, dtype=np.float64) + z for a in f(X[0], X[1], X[2], t)])

    def prim(self, X, t):  # rho, u, v, w, p
        return self._eval(self._fp, X, t)

    def state(self, X, t):  # conserved, as src/masa_handler.cpp:318-335 assembles it
        return self._eval(self._fu, X, t)

    def source(self, X, t):  # masa_eval_source_*: Q = dU/dt + div F(U)
        return self._eval(self._fs, X, t)


@functools.lru_cache(maxsize=None)
def euler_transient_3d(forms="scscc"):
    import sympy as sp

    P = TPS_EULER_TRANSIENT_3D
    x, y, z, t = sp.symbols("x y z t")
    L, pi = P["L"], sp.pi
    tf = [sp.sin if c == "s" else sp.cos for c in forms]

    def arg(name, s):
        return P[name] * pi * s / L

    rho = P["rho_0"] + P["rho_x"] * sp.sin(arg("a_rhox", x)) + P["rho_y"] * sp.cos(arg("a_rhoy", y)) + P["rho_z"] * sp.sin(arg("a_rhoz", z)) + P["rho_t"] * tf[0](arg("a_rhot", t))
    u = P["u_0"] + P["u_x"] * sp.sin(arg("a_ux", x)) + P["u_y"] * sp.cos(arg("a_uy", y)) + P["u_z"] * sp.cos(arg("a_uz", z)) + P["u_t"] * tf[1](arg("a_ut", t))
    v = P["v_0"] + P["v_x"] * sp.cos(arg("a_vx", x)) + P["v_y"] * sp.sin(arg("a_vy", y)) + P["v_z"] * sp.sin(arg("a_vz", z)) + P["v_t"] * tf[2](arg("a_vt", t))
    w = P["w_0"] + P["w_x"] * sp.sin(arg("a_wx", x)) + P["w_y"] * sp.sin(arg("a_wy", y)) + P["w_z"] * sp.cos(arg("a_wz", z)) + P["w_t"] * tf[3](arg("a_wt", t))
    p = P["p_0"] + P["p_x"] * sp.cos(arg("a_px", x)) + P["p_y"] * sp.sin(arg("a_py", y)) + P["p_z"] * sp.cos(arg("a_pz", z)) + P["p_t"] * tf[4](arg("a_pt", t))
    g = P["Gamma"]
    vel, X = [u, v, w], [x, y, z]
    E = p / (g - 1) + rho * sum(c * c for c in vel) / 2
    U = [rho, rho * u, rho * v, rho * w, E]
    F = [[rho * vel[d] for d in range(3)]]
    for i in range(3):
        F.append([U[1 + i] * vel[d] + (p if i == d else 0) for d in range(3)])
    F.append([vel[d] * (E + p) for d in range(3)])
    S = [sp.diff(U[k], t) + sum(sp.diff(F[k][d], X[d]) for d in range(3)) for k in range(5)]
    a = (x, y, z, t)
    return _Transient3D(sp.lambdify(a, [rho, u, v, w, p], "numpy"), sp.lambdify(a, U, "numpy"), sp.lambdify(a, S, "numpy"))


def lp_errors_box(X, U, ms, t, p, gamma=1.4):
    """M2ulPhyS::checkSolutionError for dry air (src/masa_handler.cpp:139-152): the L2 errors of the density, velocity and
    pressure grid functions against the exact fields, as mfem::GridFunction::ComputeLpError(2, coefficient) forms them
    with its default rule [third party: MFEM, fem/gridfunc.cpp: Gauss-Legendre of order 2 p + 3 per element].
    Axis-aligned box elements with a tensor Gauss-Legendre nodal basis (X: node coordinates (3, ne * (p+1)^3), U: the
    conserved state at the nodes); the nodal interpolants are evaluated at the rule's points in physical coordinates,
    which does not depend on how an element's local axes are oriented."""
    npe = (p + 1) ** 3
    ne = X.shape[1] // npe
    nq = (2 * p + 3) // 2 + 1
    gq, wq = np.polynomial.legendre.leggauss(nq)
    gq, wq = 0.5 * (gq + 1.0), 0.5 * wq
    gn = 0.5 * (np.polynomial.legendre.leggauss(p + 1)[0] + 1.0)
    rho = U[0]
    fields = np.stack([rho, U[1] / rho, U[2] / rho, U[3] / rho,
                       (gamma - 1.0) * (U[4] - 0.5 * (U[1] ** 2 + U[2] ** 2 + U[3] ** 2) / rho)]).reshape(5, ne, npe)
    Xe = X.reshape(3, ne, npe)
    lag, xq, vol = [], [], np.ones(ne)
    for d in range(3):
        lo, hi = Xe[d].min(axis=1), Xe[d].max(axis=1)
        h = (hi - lo) / (gn[-1] - gn[0])
        x0 = lo - gn[0] * h
        pts = x0[:, None] + gq[None, :] * h[:, None]  # (ne, nq)
        # 1-D nodal positions of the element in this direction, and the Lagrange factor of every node at every point
        knots = x0[:, None] + gn[None, :] * h[:, None]  # (ne, p+1)
        ld = np.ones((ne, npe, nq))
        for a in range(p + 1):
            mine = np.isclose(Xe[d][:, :, None], knots[:, None, a:a + 1], rtol=0, atol=1e-9 * np.abs(h)[:, None, None] + 1e-300)[..., 0]
            fac = np.ones((ne, nq))
            for b in range(p + 1):
                if b != a:
                    fac *= (pts - knots[:, b:b + 1]) / (knots[:, a:a + 1] - knots[:, b:b + 1])
            ld = np.where(mine[:, :, None], fac[:, None, :], ld)
        lag.append(ld)
        xq.append(pts)
        vol = vol * h
    # values at the points: (5, ne, nq, nq, nq)
    vals = np.einsum("fen,eni,enj,enk->feijk", fields, lag[0], lag[1], lag[2], optimize=True)
    Xq = np.stack([np.broadcast_to(xq[0][:, :, None, None], (ne, nq, nq, nq)), np.broadcast_to(xq[1][:, None, :, None], (ne, nq, nq, nq)),
                   np.broadcast_to(xq[2][:, None, None, :], (ne, nq, nq, nq))]).reshape(3, -1)
    exact = ms.prim(Xq, t).reshape(5, ne, nq, nq, nq)
    w3 = wq[:, None, None] * wq[None, :, None] * wq[None, None, :]
    d2 = (vals - exact) ** 2
    integ = lambda a: float(np.sqrt(np.sum(a * w3[None] * vol[:, None, None, None])))  # noqa: E731
    return integ(d2[0]), integ(d2[1] + d2[2] + d2[3]), integ(d2[4])


# ---------------------------------------------------------------------------------------------------------------
# test/mms.ternary_2d.test: `ternary_2d_2t_periodic_ambipolar`, a manufactured solution of the TPS team's MASA fork [third
# party, absent] for the two-temperature ambipolar ternary mixture with constant transport and one reaction with detailed
# balance.  Every parameter is in src/masa_handler.cpp:501-546, 652-672; the FORM is not in the reference.  Found by
# running the family the parameter names suggest (tools/mms_ternary_periodic.py; the record is profiles/
# r04_mms_ternary_periodic.txt):  f = f0 + dfx gx(2 pi kfx (x / Lx - offset_fx)) + dfy gy(2 pi kfy (y / Ly - offset_fy))  with
# (gx, gy) = (cos, cos) for rho, Y_ion, T, T_e and MASA's velocity convention (sin, cos) for u, (cos, sin) for v.
TERNARY_FORM = "cos-|u=sc-|v=cs-"
TERNARY_REF = (9.4069e-4, 0.1560, 0.0449, 1.3975e-3, 2.6037e-3, 3.0008e-3)  # test/mms.ternary_2d.test:42-67
TERNARY_LX = TERNARY_LY = 5.0

# src/masa_handler.cpp:501-546 (initTernary2DBase) and :652-658 (initTernary2D2TPeriodicAmbipolar)
TERNARY_P = dict(u=(1.5, 0.1, 0.2, 1.0, 2.0, -0.33, 0.47), v=(0.91, 0.13, 0.11, 2.0, 1.0, 0.11, 0.92),
         rho=(1.2, 0.17, 0.09, 1.0, 1.0, 0.74, 0.19), Y0=(0.34, 0.13, 0.07, 2.0, 1.0, 0.17, 0.58),
         T=(500.0, 37.0, 29.0, 1.0, 1.0, 0.71, 0.29), TE=(700.0, 49.3, 23.1, 2.0, 1.0, 0.31, 0.91))


def ternary_physics():
    """test/inputs/mms.ternary_plasma.2d.ini:120-185 in mixture order (Ar.+1, E, Ar)"""
    from tps_amd import capi

    ph = capi.argon_ternary_physics(capi.NS, two_temperature=True, transport=capi.CONSTANT, reactions="balance")
    mx, nsp = ph.mixture, 3
    m_ar, m_e = 39.948e-3, 10.0e-3
    for sp, (mw, ef) in enumerate(((m_ar - m_e, 1.521e4), (m_e, 0.0), (m_ar, 0.0))):
        mx.gas_params[sp + capi.SPECIES_MW * nsp] = mw
        mx.gas_params[sp + capi.FORMATION_ENERGY * nsp] = ef
        mx.molar_cv[sp] = 1.5
    ct = ph.constant_transport
    ct.viscosity, ct.bulk_viscosity, ct.thermal_conductivity, ct.electron_thermal_conductivity = 1.1, 0.3, 0.6, 0.3
    for sp, (d, f) in enumerate(((1.3, 2.3), (3.1, 0.9), (1.9, 4.1))):
        ct.diffusivity[sp], ct.mt_freq[sp] = d, f
    ch = ph.chemistry
    ch.num_reactions = 1
    ch.minimum_temperature = 0.0
    ch.reaction_energies[0] = 1.521e4
    ch.detailed_balance[0] = 1
    ch.reaction_models[0] = capi.ARRHENIUS
    for sp, (r, p) in enumerate(((0, 1), (1, 2), (1, 0))):  # Ar + E <=> Ar.+1 + 2 E
        ch.reactant_stoich[sp], ch.product_stoich[sp] = r, p
    for k, v in enumerate((4.7, 1.2, 6.49e4)):
        ch.rate_params[k] = v
    for k, v in enumerate((1.39, 0.7, 6.197e2)):
        ch.equilibrium_constant_params[k] = v
    return ph


def ternary_exact_state(ph, X, form=None):
    """form: "cos-" (every field g = cos, offsets subtracted) or, for the search over the velocity components,
    "cos-|u=sc+|v=cs-": per-field overrides, two letters = g of the x term and of the y term, then the offset sign"""
    parts = (form or TERNARY_FORM).split("|")
    base = parts[0]
    over = dict(p.split("=") for p in parts[1:])
    trig = {"s": np.sin, "c": np.cos}

    def fld(name):
        f0, dx, dy, kx, ky, ox, oy = TERNARY_P[name]
        spec = over.get(name, base[0] * 2 + base[-1])
        gx, gy, sgn = trig[spec[0]], trig[spec[1]], (-1.0 if spec[2] == "-" else 1.0)
        return f0 + dx * gx(2 * np.pi * kx * (X[0] / TERNARY_LX + sgn * ox)) + dy * gy(2 * np.pi * ky * (X[1] / TERNARY_LY + sgn * oy))

    from tps_amd import capi, cases

    rho, u, v, y0, th, te = (fld(n) for n in ("rho", "u", "v", "Y0", "T", "TE"))
    m_i = ph.mixture.gas_params[0 + capi.SPECIES_MW * 3]
    return cases.plasma_conserved(ph, 2, rho, [u, v], th, [rho * y0 / m_i], te)


def _lagrange(nodes, x):
    """values of the Lagrange basis on `nodes` at the points x: (len(x), len(nodes))"""
    out = np.ones((x.size, nodes.size))
    for a in range(nodes.size):
        for b in range(nodes.size):
            if b != a:
                out[:, a] *= (x - nodes[b]) / (nodes[a] - nodes[b])
    return out


def _oracle_mult_factory(mesh, disc, ph):
    from oracle_lib import Oracle

    return Oracle(mesh, disc, ph, threads=8).mult


def ternary_fine_source(ph, form, Xc, n_fine, p_fine=5, mult_factory=None):
    """Q = -RHS(U_exact) at the points Xc: the operator itself (`mult_factory(mesh, disc, physics)` -> U -> Mult(U); default the
    oracle) at order p_fine on the collocated pair on an n_fine^2 mesh -- its residual converges to the PDE at O(h^5) --,
    evaluated at Xc by Lagrange interpolation inside the fine elements"""
    from oracle_lib import Oracle
    from tps_amd import capi, meshgen

    m = meshgen.box_quad(n_fine, n_fine, lengths=(TERNARY_LX, TERNARY_LY))
    disc = capi.Disc(p_fine, 0, 0, 0, 0)
    Xf = Oracle(m, disc, ph).node_coords()
    y = (mult_factory or _oracle_mult_factory)(m, disc, ph)(ternary_exact_state(ph, Xf, form))
    npe = (p_fine + 1) ** 2
    neq = y.shape[0]
    h = TERNARY_LX / n_fine
    gn = 0.5 * (np.polynomial.legendre.leggauss(p_fine + 1)[0] + 1.0)
    # element of every target point (points on element borders go to the element on their right / above, periodic)
    ix = np.floor(Xc[0] / h + 1e-12).astype(int) % n_fine
    iy = np.floor(Xc[1] / h + 1e-12).astype(int) % n_fine
    xi = np.clip(Xc[0] / h - np.floor(Xc[0] / h + 1e-12), 0.0, 1.0)
    eta = np.clip(Xc[1] / h - np.floor(Xc[1] / h + 1e-12), 0.0, 1.0)
    # element numbering / node numbering of the generated box: read them off the node coordinates
    Xe = Xf.reshape(2, -1, npe)
    cx = np.floor(Xe[0].mean(axis=1) / h).astype(int)
    cy = np.floor(Xe[1].mean(axis=1) / h).astype(int)
    emap = -np.ones((n_fine, n_fine), dtype=int)
    emap[cx, cy] = np.arange(cx.size)
    e = emap[ix, iy]
    lx, ly = _lagrange(gn, xi), _lagrange(gn, eta)
    # local node -> (a, b) indices from the first element's coordinates
    a_of = np.argmin(np.abs((Xe[0][0] - Xe[0][0].min())[:, None] / h - (gn - gn[0])[None, :]), axis=1)
    b_of = np.argmin(np.abs((Xe[1][0] - Xe[1][0].min())[:, None] / h - (gn - gn[0])[None, :]), axis=1)
    w = lx[:, a_of] * ly[:, b_of]  # (npts, npe)
    ye = y.reshape(neq, -1, npe)
    return -np.einsum("kpn,pn->kp", ye[:, e, :], w)


def ternary_rel_errors(Xc, U, Uex, p=2):
    """M2ulPhyS::checkSolutionError (src/masa_handler.cpp:153-163): per component ||U_h - U_exact|| / ||U_exact||, both by
    mfem::GridFunction::ComputeLpError's default rule (Gauss-Legendre, order 2p + 3) on the Gauss-Lobatto nodal basis.
    `Uex`: callable points -> exact conserved state."""
    npe = (p + 1) ** 2
    ne = Xc.shape[1] // npe
    nq = (2 * p + 3) // 2 + 1
    gq, wq = np.polynomial.legendre.leggauss(nq)
    gq, wq = 0.5 * (gq + 1.0), 0.5 * wq
    Xe = Xc.reshape(2, ne, npe)
    lo = Xe.min(axis=2)
    h = Xe.max(axis=2) - lo  # Gauss-Lobatto nodes include the end points
    gl = np.array([0.0, 0.5, 1.0]) if p == 2 else None
    a_of = np.rint((Xe[0][0] - lo[0][0]) / h[0][0] * p).astype(int)
    b_of = np.rint((Xe[1][0] - lo[1][0]) / h[1][0] * p).astype(int)
    L = _lagrange(gl, gq)  # (nq, p+1)
    W = np.einsum("in,jn->ijn", L[:, a_of], L[:, b_of])  # (nq, nq, npe)
    neq = U.shape[0]
    vals = np.einsum("ken,ijn->keij", U.reshape(neq, ne, npe), W)
    xq = lo[0][:, None, None] + gq[None, :, None] * h[0][:, None, None] + 0 * gq[None, None, :]
    yq = lo[1][:, None, None] + gq[None, None, :] * h[1][:, None, None] + 0 * gq[None, :, None]
    ex = Uex(np.stack([xq.ravel(), yq.ravel()])).reshape(neq, ne, nq, nq)
    w2 = wq[:, None] * wq[None, :] * (h[0] * h[1])[:, None, None]
    num = np.sqrt(np.sum((vals - ex) ** 2 * w2[None], axis=(1, 2, 3)))
    den = np.sqrt(np.sum(ex ** 2 * w2[None], axis=(1, 2, 3)))
    return num / den



def ternary_run(form=None, n_fine=40, steps=500, dt=1e-5, mult_factory=None, source="point"):
    """test/mms.ternary_2d.test: 10 x 10 periodic quads on [0, 5]^2 (`beam_mesh -nx 1 -nt 5 -b 5 -rs 1`), order 2, Gauss-Lobatto
    pair, 500 RK4 steps of 1e-5 s from the exact state with the (steady) source at every stage; returns the six relative errors.
    source = "point": the classic manufactured source from the point closures (`ternary_point_source`); "fine": -RHS(U_exact) of
    the operator itself at order 5 on an n_fine^2 mesh (`ternary_fine_source`) -- they agree to 5e-7"""
    from oracle_lib import Oracle
    from tps_amd import capi, meshgen

    form = form or TERNARY_FORM
    ph = ternary_physics()
    m = meshgen.box_quad(10, 10, lengths=(TERNARY_LX, TERNARY_LY))
    disc = capi.Disc(2, 1, 1, 0, 0)
    o = Oracle(m, disc, ph, threads=8)
    Xc = o.node_coords()
    if source == "point":
        Q = ternary_point_source(ph, form, Xc, o)
    else:
        Q = ternary_fine_source(ph, form, Xc, n_fine, mult_factory=mult_factory)
    mult = (mult_factory or _oracle_mult_factory)(m, disc, ph)
    x = ternary_exact_state(ph, Xc, form)
    for _ in range(steps):
        k1 = mult(x) + Q
        k2 = mult(x + 0.5 * dt * k1) + Q
        k3 = mult(x + 0.5 * dt * k2) + Q
        k4 = mult(x + dt * k3) + Q
        x = x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return ternary_rel_errors(Xc, x, lambda X: ternary_exact_state(ph, X, form))


_FD8 = np.array([1.0 / 280, -4.0 / 105, 1.0 / 5, -4.0 / 5, 0.0, 4.0 / 5, -1.0 / 5, 4.0 / 105, -1.0 / 280])


def ternary_point_source(ph, form, X, oracle, h=0.01):
    """The manufactured source the classic way: Q = div [F_c(U) - F_v(U, grad Up)] - S(U, Up, grad Up) of the exact fields,
    with the fluxes and sources of the POINT closures (the oracle's restatements of Fluxes::ComputeConvectiveFluxes /
    ComputeViscousFluxes and SourceTerm, `oracle_lib.Oracle.convective_flux / viscous_flux / source / prim`) and eighth-order
    central differences of step h for the two levels of derivatives (the exact fields are entire functions: the truncation
    error is below 1e-14, the round-off of a difference quotient ~1e-13 relative).  Independent of the DG operators -- volume,
    face, inverse mass -- which `ternary_fine_source` goes through."""
    dim, npts = 2, X.shape[1]
    offs = np.arange(-4, 5) * h

    def up_and_grad(P):  # P: (2, m) points -> U (neq, m), Up (neq, m), gradUp (m, dim, neq)
        U = ternary_exact_state(ph, P, form)
        m = P.shape[1]
        Up = np.array([oracle.prim(U[:, i]) for i in range(m)]).T
        g = np.zeros((m, dim, U.shape[0]))
        for d in range(dim):
            for k, c in enumerate(_FD8):
                if c == 0.0:
                    continue
                Pk = P.copy()
                Pk[d] += offs[k]
                Uk = ternary_exact_state(ph, Pk, form)
                g[:, d, :] += (c / h) * np.array([oracle.prim(Uk[:, i]) for i in range(m)])
        return U, Up, g

    def flux(P):  # (m, dim, neq)
        U, _, g = up_and_grad(P)
        return np.array([oracle.convective_flux(U[:, i]) - oracle.viscous_flux(U[:, i], g[i]) for i in range(P.shape[1])])

    div = np.zeros((npts, ternary_exact_state(ph, X[:, :1], form).shape[0]))
    for d in range(dim):
        for k, c in enumerate(_FD8):
            if c == 0.0:
                continue
            Pk = X.copy()
            Pk[d] += offs[k]
            div += (c / h) * flux(Pk)[:, d, :]
    U, Up, g = up_and_grad(X)
    S = np.array([oracle.source(U[:, i], Up[:, i], g[i]) for i in range(npts)])
    return (div - S).T
