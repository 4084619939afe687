"""numpy restatements for the two-dimensional table gas (``flow/lte/table_dim = 2``), written from the formulas of
include/tpsrhs.h and the reference's closures, not from the library's code: the bilinear interpolant of
``GslTableInterpolator2D`` (GSL is not needed: ``gsl_interp2d_bilinear`` is the formula below) and the Newton iteration of
``LteMixture::ComputeTemperatureInternal`` (src/lte_mixture.cpp:161-223)."""
import numpy as np


def cell(x, xe):
    """cell i with x[i] <= xe < x[i+1]; the last abscissa belongs to the last cell; outside: the end cell (extrapolation)"""
    return np.clip(np.searchsorted(x, xe, side="right") - 1, 0, len(x) - 2)


def bilinear(x, y, f, xe, ye, what=0):
    """f (ny, nx) at the points (xe, ye): the value (what = 0), d/dx (1) or d/dy (2)"""
    xe, ye = np.asarray(xe, dtype=np.float64), np.asarray(ye, dtype=np.float64)
    i, j = cell(x, xe), cell(y, ye)
    dx, dy = x[i + 1] - x[i], y[j + 1] - y[j]
    t, u = (xe - x[i]) / dx, (ye - y[j]) / dy
    z00, z10, z01, z11 = f[j, i], f[j, i + 1], f[j + 1, i], f[j + 1, i + 1]
    if what == 1:
        return (-(1 - u) * z00 + (1 - u) * z10 - u * z01 + u * z11) / dx
    if what == 2:
        return (-(1 - t) * z00 - t * z10 + (1 - t) * z01 + t * z11) / dy
    return (1 - t) * (1 - u) * z00 + t * (1 - u) * z10 + (1 - t) * u * z01 + t * u * z11


def bilinear_exact(x, y, f, xe, ye, what=0):
    """the same formula in exact rational arithmetic (every float is a rational number), rounded once at the end.  In
    float64 the formula for d/dy subtracts values of the size of the table from each other: where the table hardly depends
    on y its own rounding, eps |z| / dy, is far above 1e-12 of the slope -- a reference has to be better than that."""
    from fractions import Fraction as F

    out = np.empty(len(xe))
    ii, jj = cell(x, np.asarray(xe)), cell(y, np.asarray(ye))
    for n, (i, j) in enumerate(zip(ii, jj)):
        dx, dy = F(x[i + 1]) - F(x[i]), F(y[j + 1]) - F(y[j])
        t, u = (F(xe[n]) - F(x[i])) / dx, (F(ye[n]) - F(y[j])) / dy
        z00, z10, z01, z11 = F(f[j, i]), F(f[j, i + 1]), F(f[j + 1, i]), F(f[j + 1, i + 1])
        if what == 1:
            v = (-(1 - u) * z00 + (1 - u) * z10 - u * z01 + u * z11) / dx
        elif what == 2:
            v = (-(1 - t) * z00 - t * z10 + (1 - t) * z01 + t * z11) / dy
        else:
            v = (1 - t) * (1 - u) * z00 + t * (1 - u) * z10 + (1 - t) * u * z01 + t * u * z11
        out[n] = float(v)
    return out


def largest_slope(x, y, f, xe, ye, what):
    """the largest |slope| along x (what = 1) or y (2) among the four edges of the cell of each point"""
    i, j = cell(x, xe), cell(y, ye)
    if what == 1:
        a, b = (f[j, i + 1] - f[j, i]), (f[j + 1, i + 1] - f[j + 1, i])
        return np.maximum(np.abs(a), np.abs(b)) / (x[i + 1] - x[i])
    a, b = (f[j + 1, i] - f[j, i]), (f[j + 1, i + 1] - f[j, i + 1])
    return np.maximum(np.abs(a), np.abs(b)) / (y[j + 1] - y[j])


def temperature(t, energy, rho):
    """ComputeTemperatureInternal per state: guess T(e, rho) of the e_rev table, Newton on e(T, rho) with the reference's four
    tolerances and 20 iterations.  Returns (T, iterations, converged); `t` = capi.lte2d_tables()."""
    energy, rho = np.asarray(energy, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    T = bilinear(t["erev_e"], t["erev_rho"], t["erev_T"], energy, rho)
    th = (t["thermo_T"], t["thermo_rho"], t["thermo_e"])
    res = energy - bilinear(*th, T, rho)
    res0 = np.abs(res)
    with np.errstate(invalid="ignore", divide="ignore"):
        conv = (np.abs(res) < 1e-18) | (np.abs(res) / res0 < 1e-12)
    it = np.zeros(T.shape, dtype=int)
    for _ in range(20):
        act = ~conv
        if not act.any():
            break
        dT = res[act] / bilinear(*th, T[act], rho[act], 1)
        T[act] += dT
        res[act] = energy[act] - bilinear(*th, T[act], rho[act])
        conv[act] = (np.abs(res[act]) < 1e-18) | (np.abs(res[act]) / res0[act] < 1e-12) | (np.abs(dT) < 1e-12) | (np.abs(dT) / T[act] < 1e-8)
        it[act] += 1
    return T, it, conv


def blended_1d_physics(rho, eq_system, radiation=False, transport="reference"):
    """The one-dimensional table gas that the two-dimensional one IS at a uniform density `rho`: every (T, rho) table
    blended between its two density lines, (1-u) f_j + u f_{j+1} -- for the frozen oracle, through the existing `lte`
    field.  Bilinear interpolation at a fixed density is linear interpolation in T of exactly these blends."""
    from tps_amd import capi

    t = capi.lte2d_tables()
    mu, kappa, sigma = t["trans_mu"], t["trans_kappa"], t["trans_sigma"]
    if transport == "synthetic":
        mu, kappa, sigma = capi.synthetic_transport_2d(t["trans_T"], t["trans_rho"], (mu, kappa))

    def blend(y, f):
        j = int(cell(y, rho))
        u = (rho - y[j]) / (y[j + 1] - y[j])
        return (1 - u) * f[j] + u * f[j + 1]

    ph = capi.lte_physics(eq_system, "rho0p255", radiation)
    keep = ph._keep
    ph.lte.energy_table = capi.make_table(t["thermo_T"], blend(t["thermo_rho"], t["thermo_e"]), keep=keep)
    ph.lte.gas_constant_table = capi.make_table(t["thermo_T"], blend(t["thermo_rho"], t["thermo_R"]), keep=keep)
    ph.lte.sound_speed_table = capi.make_table(t["thermo_T"], blend(t["thermo_rho"], t["thermo_c"]), keep=keep)
    ph.lte.viscosity_table = capi.make_table(t["trans_T"], blend(t["trans_rho"], mu), keep=keep)
    ph.lte.conductivity_table = capi.make_table(t["trans_T"], blend(t["trans_rho"], kappa), keep=keep)
    ph.lte.electric_conductivity_table = capi.make_table(t["trans_T"], blend(t["trans_rho"], sigma), keep=keep)
    return ph
