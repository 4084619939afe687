"""A numpy restatement of the quadrature rule of include/tpsrhs.h (tpsrhs_quadrature_points, tpsrhs_integrate) and the
rounding bound that follows from its summation structure.

The rule: tensor Gauss-Legendre with NQ = p + 2 points per direction on [0,1]; point q = e NQ^dim + (i + j NQ + k NQ^2);
order-1 geometry (the bi-/trilinear map through elem_coords, MFEM vertex order, as tests/sampling_util.py states it);
W_q = w_i w_j (w_k) |det J(xi_q)|, times the first coordinate of the mapped point with `radial`; a nodal field is
evaluated with the operator's Lagrange basis.  Everything from the vertex coordinates on is computed in np.longdouble, and
each element's terms are summed (in longdouble) before the elements are.

The bound is derived, not measured.  With the terms of one element summed first (NQ^dim terms), the element sums added in
any order (ne terms) and 8 dim (p + 1) roundings in the interpolation of one value and in det J,
    |device - exact| <= K eps S1      for sum   = sum_q W_q g_q,      S1 = sum_q |W_q| A_q
    |device - exact| <= 2 K eps S2    for sumsq = sum_q W_q g_q^2,    S2 = sum_q |W_q| (A_q + |exact_q|)^2
    K = NQ^dim + ne + 8 dim (p + 1),  A_q = sum_nodes |l_node(xi_q)| |f_node|   (without exact_q, g = f_h and |exact_q| = 0).
"""
import numpy as np

import sampling_util as su
from tps_amd import meshgen

EPS = np.finfo(np.float64).eps
LD = np.longdouble


def rule_1d(order):
    """the NQ = order + 2 Gauss-Legendre points and weights on [0,1]"""
    g, w = np.polynomial.legendre.leggauss(order + 2)
    return 0.5 * (g + 1.0), 0.5 * w


def reference_points(dim, order):
    """xi (dim, NQ^dim) with q = i + j NQ + k NQ^2, and the products of the 1-D weights (NQ^dim,)"""
    g, w = rule_1d(order)
    nq = g.size
    if dim == 2:
        j, i = np.meshgrid(np.arange(nq), np.arange(nq), indexing="ij")
        idx = [i.ravel(), j.ravel()]
    else:
        k, j, i = np.meshgrid(np.arange(nq), np.arange(nq), np.arange(nq), indexing="ij")
        idx = [i.ravel(), j.ravel(), k.ravel()]
    xi = np.stack([g[a] for a in idx])
    wprod = np.prod(np.stack([w[a] for a in idx]), axis=0)
    return xi, wprod


def geometry(mesh, order):
    """-> (xyz (dim, npts), W (npts,) without the radial factor), np.longdouble"""
    dim = mesh.dim
    xi, wprod = reference_points(dim, order)
    xi, wprod = xi.astype(LD), wprod.astype(LD)
    ex = np.asarray(mesh.elem_coords, dtype=LD)  # (ne, nv, dim)
    ne, nqd = ex.shape[0], xi.shape[1]
    x = np.zeros((dim, ne, nqd), dtype=LD)
    J = np.zeros((ne, dim, dim, nqd), dtype=LD)  # J[e, a, d, q] = dx_a / dxi_d
    for v, c in enumerate(su.CORNERS[dim]):
        f = [xi[d] if c[d] else 1 - xi[d] for d in range(dim)]
        shp = np.prod(np.stack(f), axis=0)
        x += ex[:, v, :].T[:, :, None] * shp[None, None, :]
        for d in range(dim):
            dshp = np.full(nqd, 1.0 if c[d] else -1.0, dtype=LD)
            for k in range(dim):
                if k != d:
                    dshp = dshp * f[k]
            J[:, :, d, :] += ex[:, v, :, None] * dshp[None, None, :]
    if dim == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    else:
        det = (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1])
               + J[:, 0, 1] * (J[:, 1, 2] * J[:, 2, 0] - J[:, 1, 0] * J[:, 2, 2])
               + J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))
    W = wprod[None, :] * np.abs(det)
    return x.reshape(dim, -1), W.reshape(-1)


def constant_K(mesh, order):
    return (order + 2) ** mesh.dim + mesh.num_elements + 8 * mesh.dim * (order + 1)


def integrate(mesh, order, basis_type, field, exact_q=None, radial=False):
    """field (nrows, NDofs), exact_q (nrows, npts) or None -> dict(sum, sumsq, S1, S2, K): float64 arrays (nrows,)"""
    field = np.atleast_2d(np.asarray(field, dtype=np.float64))
    dim, ne = mesh.dim, mesh.num_elements
    npe = (order + 1) ** dim
    xi, _ = reference_points(dim, order)
    nqd = xi.shape[1]
    T = su.tensor_weights(xi, order, basis_type, dtype=LD)  # (nqd, npe)
    xyz, W = geometry(mesh, order)
    if radial:
        W = W * xyz[0]
    W = W.reshape(ne, nqd)
    nrows = field.shape[0]
    out = {k: np.zeros(nrows) for k in ("sum", "sumsq", "S1", "S2")}
    for r in range(nrows):
        u = field[r].reshape(ne, npe).astype(LD)
        vals = u @ T.T  # (ne, nqd)
        A = np.abs(u) @ np.abs(T).T
        ex = np.zeros_like(vals) if exact_q is None else np.asarray(exact_q[r], dtype=LD).reshape(ne, nqd)
        g = vals - ex
        out["sum"][r] = float((W * g).sum(axis=1).sum())
        out["sumsq"][r] = float((W * g * g).sum(axis=1).sum())
        out["S1"][r] = float((np.abs(W) * A).sum(axis=1).sum())
        out["S2"][r] = float((np.abs(W) * (A + np.abs(ex)) ** 2).sum(axis=1).sum())
    out["K"] = constant_K(mesh, order)
    return out


def check(name, got_sum, got_sumsq, ref, exact_sum=None, exact_sumsq=None):
    """prints the achieved errors in units of eps * S and asserts the bounds; `exact_*`: closed forms that replace the
    restatement's values as the reference (the bound then also has to absorb nothing else: the rule is exact for them)"""
    K = ref["K"]
    want1 = ref["sum"] if exact_sum is None else np.asarray(exact_sum)
    want2 = ref["sumsq"] if exact_sumsq is None else np.asarray(exact_sumsq)
    e1 = np.abs(np.asarray(got_sum) - want1) / (EPS * ref["S1"])
    e2 = np.abs(np.asarray(got_sumsq) - want2) / (EPS * ref["S2"])
    print(f"{name}: K = {K}; |sum - ref| / (eps S1) = {e1.max():.3f}; |sumsq - ref| / (eps S2) = {e2.max():.3f} (bound {2 * K})")
    assert (e1 <= K).all(), (name, e1, K)
    assert (e2 <= 2 * K).all(), (name, e2, 2 * K)
    return e1.max(), e2.max()


# ---- meshes ------------------------------------------------------------------------------------------------------------------
def ring_quad(nr=4, ntheta=12, r_in=0.5, r_out=10.0, stretch=1.05):
    """the cross-section of meshgen.ogrid_cylinder: a 2-D O-grid ring, periodic in theta; attributes 1 inlet, 2 outlet, 3 wall"""
    dr0 = (r_out - r_in) * (stretch - 1.0) / (stretch ** nr - 1.0)
    r = r_in + dr0 * (stretch ** np.arange(nr + 1) - 1.0) / (stretch - 1.0)
    r[-1] = r_out

    def xyz(i, j):
        th = 2.0 * np.pi * j / ntheta
        return np.stack([r[i] * np.cos(th), r[i] * np.sin(th)], axis=-1)

    def outer(centre):
        return np.where(centre[:, 0] < 0.0, 1, 2)

    return meshgen._structured(2, (nr, ntheta), xyz, (False, True), {(0, 0): 3, (0, 1): outer})


def perturbed_box(dim, n, seed=3, amp=0.18):
    """the unit box with walls all round, n cells per direction, every INTERIOR vertex moved by up to amp cell sizes per
    direction: the elements are non-affine and the box is still the unit box"""
    n = tuple(n)
    m = (meshgen.box_hex if dim == 3 else meshgen.box_quad)(*n, periodic=(False,) * dim)
    rng = np.random.default_rng(seed)
    shift = rng.uniform(-amp, amp, size=(m.num_vertices, dim)) / np.array(n, dtype=np.float64)
    ex = np.array(m.elem_coords, dtype=np.float64)
    interior = np.all((ex > 1e-12) & (ex < 1.0 - 1e-12), axis=2)  # (ne, nv)
    ex = ex + np.where(interior[:, :, None], shift[np.asarray(m.elem_vertices)], 0.0)
    import dataclasses

    return dataclasses.replace(m, elem_coords=ex)


def shoelace_areas(quads):
    """quads (ne, 4, 2) in MFEM (counter-clockwise) order -> (ne,) areas"""
    x, y = quads[..., 0], quads[..., 1]
    return 0.5 * np.abs((x * np.roll(y, -1, axis=1) - np.roll(x, -1, axis=1) * y).sum(axis=1))


def monomial_integral_unit_box(exps):
    """int over [0,1]^dim of prod x_d^e_d"""
    return float(np.prod([1.0 / (e + 1) for e in exps]))


def polynomial(dim, p, seed):
    """a polynomial of total degree <= p with seeded coefficients: (f(X), int f over the unit box, int f^2 over the unit box)"""
    rng = np.random.default_rng(seed)
    terms = [e for e in np.ndindex(*([p + 1] * dim)) if sum(e) <= p]
    coef = rng.uniform(-1.0, 1.0, size=len(terms))

    def f(X):
        out = np.zeros(X.shape[1])
        for c, e in zip(coef, terms):
            t = np.full(X.shape[1], c)
            for d in range(dim):
                t = t * X[d] ** e[d]
            out += t
        return out

    i1 = sum(c * monomial_integral_unit_box(e) for c, e in zip(coef, terms))
    i2 = sum(c1 * c2 * monomial_integral_unit_box(tuple(a + b for a, b in zip(e1, e2)))
             for c1, e1 in zip(coef, terms) for c2, e2 in zip(coef, terms))
    return f, i1, i2
