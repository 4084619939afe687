"""A numpy restatement, in np.longdouble, of the Legendre modal filter and smoothness sensor of include/tpsrhs.h
(tpsrhs_modal_transform, tpsrhs_modal_energy, tpsrhs_modal_filter_apply), with the error model the device tests use.

    V[a][k] = P_k(2 xi_a - 1),  u^ = (V^-1 x ... x V^-1) u,  F = V diag(sigma) V^-1,  u~ = (F x ... x F) u
    sigma_k = 1 (k <= k_c), exp(-alpha ((k - k_c) / (p - k_c))^s) (k > k_c)
    conservative: u~_n += sum W (u - u~) / sum W
    E_m = sum_{max(i, j[, k]) = m} u^^2 gamma_i gamma_j [gamma_k], gamma_k = 1 / (2k + 1);  S = E_p / sum E (0 for 0 / 0)
    sensor_row >= 0: an element is filtered on all listed rows only if S(incoming sensor row) > threshold

The nodes are the doubles of sampling_util.nodes_1d polished by Newton in long double, so V is the Vandermonde matrix of the
true Gauss points to ~1e-19; V^-1 by Gauss-Jordan with partial pivoting in long double.  The device takes these matrices
rounded to double (half an ulp per entry).

Error model.  For r = (M x ... x M) v computed in double, per node
    bound_n = 8 dim N1 eps ((|M| x ... x |M|) |v|)_n
the forward error of dim chained dot products of length N1, with a factor 8 for the different summation order and FMA
contraction (it also holds the half ulp of the rounded matrix entries).  The energies propagate it: dE_m = sum over the shell
of (2 |u^| du^ + du^^2) gamma...; the sensor S = E_p / T: dS = dE_p / T + E_p dT / T^2 + 4 eps S.  The mean correction
c = sum W (u - u~) / sum W propagates du~ and adds the rounding of its own sum: dc = (sum |W| du~ + npe eps sum |W| (|u| +
|u~|)) / |sum W|, and a corrected node carries du~_n + dc + eps |u~_n + c|."""
import numpy as np
from numpy.polynomial import legendre as L

import sampling_util as su

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def _unit(k):
    c = np.zeros(k + 1, dtype=LD)
    c[k] = 1
    return c


def legendre(k, z):
    """P_k(z) in long double"""
    return L.legval(np.asarray(z, dtype=LD), _unit(k))


def nodes(order, basis_type):
    """the p + 1 nodes z_a in [-1, 1], np.longdouble: Newton on P_n (Gauss-Legendre) or P'_{n-1} (interior Gauss-Lobatto)"""
    n1 = order + 1
    z = (2 * np.asarray(su.nodes_1d(order, basis_type), dtype=LD) - 1).copy()
    if basis_type == 0:
        f, df = _unit(n1), L.legder(_unit(n1))
        inner = slice(0, n1)
    else:
        f, df = L.legder(_unit(n1 - 1)), L.legder(_unit(n1 - 1), 2)
        inner = slice(1, n1 - 1)
        z[0], z[-1] = -1, 1
    if z[inner].size:
        for _ in range(4):
            z[inner] = z[inner] - L.legval(z[inner], f) / L.legval(z[inner], df)
    return z


def invert(A):
    """Gauss-Jordan with partial pivoting in long double"""
    n = A.shape[0]
    w = np.concatenate([np.array(A, dtype=LD), np.eye(n, dtype=LD)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(w[c:, c])))
        w[[c, piv]] = w[[piv, c]]
        w[c] = w[c] / w[c, c]
        for r in range(n):
            if r != c:
                w[r] = w[r] - w[r, c] * w[c]
    return w[:, n:]


def matrices(order, basis_type):
    """-> (V, Vinv) (p+1, p+1) np.longdouble, V[a][k] = P_k(z_a)"""
    z = nodes(order, basis_type)
    V = np.stack([legendre(k, z) for k in range(order + 1)], axis=1)
    return V, invert(V)


def sigma(order, cutoff, alpha, exponent):
    k = np.arange(order + 1)
    eta = np.where(k > cutoff, (k - cutoff).astype(LD) / LD(order - cutoff), LD(0))
    return np.where(k > cutoff, np.exp(-LD(alpha) * eta ** int(exponent)), LD(1))


def filter_matrix(order, basis_type, cutoff, alpha, exponent):
    V, Vi = matrices(order, basis_type)
    return (V * sigma(order, cutoff, alpha, exponent)[None, :]) @ Vi


def tensor_apply(M, v, dim):
    """(M x ... x M) v on every element: v (..., n1^dim) with the first direction fastest -> the same shape, np.longdouble"""
    M = np.asarray(M, dtype=LD)
    n1 = M.shape[0]
    v = np.asarray(v, dtype=LD)
    t = v.reshape(v.shape[:-1] + (n1,) * dim)
    for ax in range(dim):  # every tensor axis is contracted with M, whichever direction it is
        t = np.moveaxis(np.matmul(M, np.moveaxis(t, -1 - ax, -2)), -2, -1 - ax) if t.ndim > 1 else M @ t
    return t.reshape(v.shape)


def apply_bound(M, v, dim):
    """8 dim N1 eps ((|M| x ... x |M|) |v|)_n"""
    n1 = np.asarray(M).shape[0]
    return 8 * dim * n1 * LD(EPS) * tensor_apply(np.abs(np.asarray(M, dtype=LD)), np.abs(np.asarray(v, dtype=LD)), dim)


def shells(order, dim):
    """-> (shell (npe,) int, weight (npe,) LD): max(i, j[, k]) and gamma_i gamma_j [gamma_k] of every mode, first index fastest"""
    n1 = order + 1
    idx = np.indices((n1,) * dim).reshape(dim, -1)[::-1]  # row 0: i (fastest)
    g = 1 / (2 * np.arange(n1).astype(LD) + 1)
    w = np.ones(n1 ** dim, dtype=LD)
    for d in range(dim):
        w = w * g[idx[d]]
    return idx.max(axis=0), w


def energies(u, order, basis_type, dim):
    """u (NDofs,) -> dict(E (ne, p+1), S (ne,), dE, dS) in np.longdouble; S = 0 where the sum is 0"""
    n1 = order + 1
    npe = n1 ** dim
    _, Vi = matrices(order, basis_type)
    v = np.asarray(u, dtype=LD).reshape(-1, npe)
    uh, duh = tensor_apply(Vi, v, dim), apply_bound(Vi, v, dim)
    shell, w = shells(order, dim)
    c, dc = uh * uh * w, (2 * np.abs(uh) * duh + duh * duh) * w
    E = np.stack([c[:, shell == m].sum(axis=1) for m in range(n1)], axis=1)
    dE = np.stack([dc[:, shell == m].sum(axis=1) for m in range(n1)], axis=1)
    T, dT = E.sum(axis=1), dE.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(T == 0, LD(0), E[:, -1] / T)
        dS = np.where(T == 0, LD(0), dE[:, -1] / T + E[:, -1] * dT / (T * T) + 4 * LD(EPS) * S)
    return dict(E=E, S=S, dE=dE, dS=dS, uhat=uh, duhat=duh)


def modal_filter(x, w, dim, order, basis_type, rows=None, cutoff=0, alpha=36.0, exponent=16, conservative=True, sensor_row=-1,
                 sensor_threshold=0.0):
    """x (neq, NDofs) float64, w (NDofs,) float64 -> dict(x (neq, NDofs) LD, bound (neq, NDofs) LD, filtered (ne,) bool,
    S (ne,) LD or None, dS); rows not listed and elements not filtered come back as they were, with bound 0"""
    x = np.asarray(x, dtype=np.float64)
    neq = x.shape[0]
    npe = (order + 1) ** dim
    ne = x.shape[1] // npe
    rows = list(range(neq)) if rows is None else list(rows)
    F = filter_matrix(order, basis_type, cutoff, alpha, exponent)
    out, bound = x.astype(LD), np.zeros(x.shape, dtype=LD)
    S = dS = None
    filtered = np.ones(ne, dtype=bool)
    if sensor_row >= 0:
        en = energies(x[sensor_row], order, basis_type, dim)
        S, dS = en["S"], en["dS"]
        with np.errstate(invalid="ignore"):
            filtered = np.asarray(S > sensor_threshold)
    W = np.asarray(w, dtype=LD).reshape(ne, npe)
    sw = W.sum(axis=1)
    for r in rows:
        v = x[r].astype(LD).reshape(ne, npe)
        t, dt = tensor_apply(F, v, dim), apply_bound(F, v, dim)
        if conservative:
            with np.errstate(invalid="ignore", divide="ignore"):
                c = (W * (v - t)).sum(axis=1) / sw
                dc = ((np.abs(W) * dt).sum(axis=1) + npe * LD(EPS) * (np.abs(W) * (np.abs(v) + np.abs(t))).sum(axis=1)) / np.abs(sw)
            t = t + c[:, None]
            dt = dt + dc[:, None] + LD(EPS) * np.abs(t)
        out[r] = np.where(filtered[:, None], t, v).reshape(-1)
        bound[r] = np.where(filtered[:, None], dt, LD(0)).reshape(-1)
    return dict(x=out, bound=bound, filtered=filtered, S=S, dS=dS)


def element_integrals(w, v, npe):
    """sum_n W_n v_n per element, in np.longdouble -> (ne,)"""
    return (np.asarray(w, dtype=LD).reshape(-1, npe) * np.asarray(v, dtype=LD).reshape(-1, npe)).sum(axis=1)


def node_coordinates_ref(order, basis_type, dim):
    """z (dim, npe) in [-1, 1], np.longdouble: the reference coordinates of an element's nodes, first direction fastest"""
    z = nodes(order, basis_type)
    n1 = order + 1
    idx = np.indices((n1,) * dim).reshape(dim, -1)[::-1]
    return np.stack([z[idx[d]] for d in range(dim)])
