"""A numpy restatement of the conservative positivity limiter of include/tpsrhs.h (tpsrhs_limit) and of its weights.

Weights.  W_n = int_K l_n dV on the rule of tpsrhs_integrate: W_n = sum_q W_q l_n(xi_q), with the points and weights of
tests/integrals_util.py (tpsrhs_quadrature_points' rule, restated there) and the operator's Lagrange basis
(sampling_util.tensor_weights), in np.longdouble.  `weights` also returns A_n = sum_q |W_q| |l_n(xi_q)|, which the error
model of tpsrhs_integrate's contract needs for one basis function.

The operation, element by element, in float64 (the order of the sums is numpy's, not the device's: the tests' tolerances
say what that costs):
    row step        mean = sum W v / sum W;  m = min v with `<`
                    1 mean NaN: untouched, not counted    2 m >= f: untouched
                    3 mean > f: theta = (mean - f) / (mean - m); v <- max(mean + theta (v - mean), f)     -> limited[row]
                    4 else:     v <- max(v, f)                                                            -> clamped[row]
    pressure step   (dry air, after the row steps, f_p > 0)  p(U) = (gamma - 1)(U[nvel+1] - 1/2 sum U[d]^2 / U[0])
                    pbar = p(element means), pmin = min_n p(U_n);  pmin >= f_p: nothing
                    pbar > f_p: theta = (pbar - f_p) / (pbar - pmin), every row v <- vbar + theta (v - vbar) -> pressure_limited
                    else: untouched                                                                  -> pressure_unfixable
"""
import numpy as np

import integrals_util as iu
import sampling_util as su

EPS = iu.EPS
LD = np.longdouble
NAN, UNTOUCHED, SCALED, CLAMPED = 0, 1, 2, 3
P_UNTOUCHED, P_SCALED, P_UNFIXABLE = 0, 1, 2


def weights(mesh, order, basis_type, radial=False):
    """-> (W (NDofs,), A (NDofs,)) as np.longdouble: W_n = sum_q W_q l_n(xi_q), A_n = sum_q |W_q| |l_n(xi_q)|"""
    dim, ne = mesh.dim, mesh.num_elements
    xi, _ = iu.reference_points(dim, order)
    T = su.tensor_weights(xi, order, basis_type, dtype=LD)  # (nqd, npe)
    xyz, Wq = iu.geometry(mesh, order)
    if radial:
        Wq = Wq * xyz[0]
    Wq = Wq.reshape(ne, -1)
    return (Wq @ T).reshape(-1), (np.abs(Wq) @ np.abs(T)).reshape(-1)


def nanmin_lt(v):
    """min over the last axis kept with `<` from +inf: a NaN never wins"""
    return np.where(np.isnan(v), np.inf, v).min(axis=-1)


def pressure(U, nvel, gamma):
    """U (neq, ...) -> p"""
    k = sum(U[d] * U[d] for d in range(1, nvel + 1))
    return (gamma - 1.0) * (U[nvel + 1] - 0.5 * k / U[0])


def limit(x, w, npe, rows, floors, pressure_floor=0.0, nvel=None, gamma=1.4):
    """x (neq, NDofs), w (NDofs,) float64 -> dict(x, outcome (len(rows), ne), p_outcome (ne,), mean (len(rows), ne),
    limited (neq,), clamped (neq,), pressure_limited, pressure_unfixable)"""
    x = np.array(x, dtype=np.float64)
    neq = x.shape[0]
    ne = x.shape[1] // npe
    W = np.asarray(w, dtype=np.float64).reshape(ne, npe)
    sw = W.sum(axis=1)
    out = dict(limited=np.zeros(neq, dtype=np.int64), clamped=np.zeros(neq, dtype=np.int64), pressure_limited=0,
               pressure_unfixable=0, outcome=np.zeros((len(rows), ne), dtype=np.int64), mean=np.zeros((len(rows), ne)),
               p_outcome=np.zeros(ne, dtype=np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, (r, f) in enumerate(zip(rows, floors)):
            v = x[r].reshape(ne, npe)
            mean = (W * v).sum(axis=1) / sw
            m = nanmin_lt(v)
            oc = np.where(np.isnan(mean), NAN, np.where(m >= f, UNTOUCHED, np.where(mean > f, SCALED, CLAMPED)))
            theta = (mean - f) / (mean - m)
            scaled = np.maximum(mean[:, None] + theta[:, None] * (v - mean[:, None]), f)
            clamped = np.fmax(v, f)
            new = np.where((oc == SCALED)[:, None], scaled, np.where((oc == CLAMPED)[:, None], clamped, v))
            x[r] = new.reshape(-1)
            out["outcome"][i], out["mean"][i] = oc, mean
            out["limited"][r] += int((oc == SCALED).sum())
            out["clamped"][r] += int((oc == CLAMPED).sum())
        if pressure_floor > 0.0:
            U = x.reshape(neq, ne, npe)
            ubar = (W[None] * U).sum(axis=2) / sw[None]  # (neq, ne)
            pbar = pressure(ubar, nvel, gamma)
            pmin = nanmin_lt(pressure(U, nvel, gamma))
            oc = np.where(pmin >= pressure_floor, P_UNTOUCHED, np.where(pbar > pressure_floor, P_SCALED, P_UNFIXABLE))
            theta = (pbar - pressure_floor) / (pbar - pmin)
            new = ubar[:, :, None] + theta[None, :, None] * (U - ubar[:, :, None])
            x = np.where((oc == P_SCALED)[None, :, None], new, U).reshape(neq, -1)
            out["p_outcome"] = oc
            out["pressure_limited"] = int((oc == P_SCALED).sum())
            out["pressure_unfixable"] = int((oc == P_UNFIXABLE).sum())
    out["x"] = x
    return out


def element_integrals(w, v, npe):
    """sum_n W_n v_n per element, in np.longdouble -> (ne,)"""
    return (np.asarray(w, dtype=LD).reshape(-1, npe) * np.asarray(v, dtype=LD).reshape(-1, npe)).sum(axis=1)


def four_outcome_rows(rng, ne, npe, nrows, floors, with_clamped=True):
    """(nrows, ne * npe): per element and row one of
         0 untouched (all above the floor)           1 scaled (one node 0.5 below, the others 1 .. 2 above: mean > floor)
         2 clamped (all but one node below)          3 untouched with the minimum ON the floor (m >= f with equality)
    the kind is (element + row) % 4; without clamped elements kind 2 becomes kind 1.  -> (values, kinds (nrows, ne))"""
    v = np.zeros((nrows, ne, npe))
    kinds = np.zeros((nrows, ne), dtype=np.int64)
    for i in range(nrows):
        f = floors[i]
        for e in range(ne):
            k = (e + i) % 4
            if k == 2 and not with_clamped:
                k = 1
            kinds[i, e] = k
            n0 = rng.integers(npe)
            if k == 0:
                a = f + 1.0 + rng.random(npe)
            elif k == 1:
                a = f + 1.0 + rng.random(npe)
                a[n0] = f - 0.5
            elif k == 2:
                a = f - 1.0 + 0.5 * rng.random(npe)
                a[n0] = f + 0.3
            else:
                a = f + rng.random(npe)
                a[n0] = f
            v[i, e] = a
    return v.reshape(nrows, -1), kinds
