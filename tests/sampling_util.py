"""A numpy restatement of point location and point evaluation on the conventions of include/tpsrhs.h: the bi-/trilinear
vertex map of an element (MFEM vertex order), its inversion by Newton from the element centre, the 1-D nodes of the nodal
basis (as tps_amd.rhs_operator.node_coordinates builds them), the Lagrange weights as products of quotients, the evaluation
u(xi) = sum_n w_n u_n with local = i + j (p+1) + k (p+1)^2, and the point formula of the reference's PlaneInterpolator.
tests/test_sampling_restatement.py pins it against polynomials and an extended-precision evaluation; the library is
compared with it (tests/test_locate_points.py, tests/test_gpu_sampling.py)."""
import numpy as np

from tps_amd import meshgen

CORNERS = {2: [(0, 0), (1, 0), (1, 1), (0, 1)],
           3: [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]}
EPS = np.finfo(np.float64).eps


def vertex_map(ex, xi):
    """ex: (nv, dim) the vertices of ONE element or (npts, nv, dim) one element per point; xi: (dim, npts) -> (dim, npts)"""
    xi = np.asarray(xi)
    dim = xi.shape[0]
    ex = np.asarray(ex)
    if ex.ndim == 2:
        ex = np.broadcast_to(ex, (xi.shape[1],) + ex.shape)
    out = np.zeros((dim, xi.shape[1]), dtype=xi.dtype)
    for v, c in enumerate(CORNERS[dim]):
        shp = np.ones(xi.shape[1], dtype=xi.dtype)
        for d in range(dim):
            shp = shp * (xi[d] if c[d] else 1.0 - xi[d])
        out += ex[:, v, :].T * shp
    return out


def jacobian(ex, xi):
    """ex (nv, dim), xi (dim,) -> J[a, d] = dx_a / dxi_d"""
    dim = len(xi)
    J = np.zeros((dim, dim))
    for v, c in enumerate(CORNERS[dim]):
        for d in range(dim):
            dw = 1.0 if c[d] else -1.0
            for k in range(dim):
                if k != d:
                    dw *= xi[k] if c[k] else 1.0 - xi[k]
            J[:, d] += ex[v] * dw
    return J


def newton_invert(ex, p, max_iter=50):
    """-> (xi, iterations, converged): Newton on vertex_map(ex, xi) = p from the element centre"""
    dim = len(p)
    xi = np.full(dim, 0.5)
    for it in range(1, max_iter + 1):
        r = np.asarray(p) - vertex_map(ex, xi[:, None])[:, 0]
        try:
            s = np.linalg.solve(jacobian(ex, xi), r)
        except np.linalg.LinAlgError:
            return xi, it, False
        xi = xi + s
        if not np.isfinite(s).all():
            return xi, it, False
        if np.abs(s).max() <= 1e-13:
            return xi, it, True
    return xi, max_iter, False


def nodes_1d(order, basis_type=0):
    """the p + 1 nodes on [0,1]: Gauss-Legendre (0) or Gauss-Lobatto (1), as rhs_operator.node_coordinates builds them"""
    n1 = order + 1
    if basis_type == 0:
        x, _ = np.polynomial.legendre.leggauss(n1)
    else:
        inner = np.polynomial.legendre.Legendre.basis(n1 - 1).deriv().roots() if n1 > 2 else np.array([])
        x = np.concatenate([[-1.0], np.sort(inner.real), [1.0]])
    return 0.5 * (x + 1.0)


def lagrange_weights(nodes, t, dtype=np.float64):
    """l_a(t) = prod_{j != a} (t - x_j) / (x_a - x_j): (n1, npts)"""
    x = np.asarray(nodes, dtype=dtype)
    t = np.asarray(t, dtype=dtype)
    out = np.ones((len(x), t.size), dtype=dtype)
    for a in range(len(x)):
        for j in range(len(x)):
            if j != a:
                out[a] = out[a] * ((t - x[j]) / (x[a] - x[j]))
    return out


def tensor_weights(ref, order, basis_type=0, dtype=np.float64):
    """ref (dim, npts) -> W (npts, (p+1)^dim), W[:, i + j n1 + k n1^2] = l_i(ref_0) l_j(ref_1) l_k(ref_2)"""
    ref = np.asarray(ref)
    dim, n1 = ref.shape[0], order + 1
    nodes = nodes_1d(order, basis_type)
    w = [lagrange_weights(nodes, ref[d], dtype) for d in range(dim)]  # (n1, npts) each
    if dim == 2:
        W = w[1][:, None, :] * w[0][None, :, :]  # [j, i, pt]
    else:
        W = w[2][:, None, None, :] * (w[1][None, :, None, :] * w[0][None, None, :, :])  # [k, j, i, pt]
    return W.reshape(n1 ** dim, -1).T


def evaluate(field, elem, ref, order, basis_type=0, dtype=np.float64):
    """field (nrows, NDofs), elem (npts,) >= 0, ref (dim, npts) -> (values (nrows, npts), sum |w u| (nrows, npts))"""
    field = np.asarray(field)
    if field.ndim == 1:
        field = field[None, :]
    dim = np.asarray(ref).shape[0]
    npe = (order + 1) ** dim
    W = tensor_weights(ref, order, basis_type, dtype)
    idx = np.asarray(elem)[:, None] * npe + np.arange(npe)[None, :]
    u = field[:, idx].astype(dtype)  # (nrows, npts, npe)
    prod = W[None, :, :] * u
    return prod.sum(axis=2), np.abs(prod).sum(axis=2)


def bound(w, u, p, dim):
    """Rounding bound of one evaluated value sum_n w_n u_n in float64, 4 k eps sum |w_n u_n| with k = 3 p dim +
    (p + 1)^dim: the first term counts the roundings of the dim products of p quotients that make up one weight
    (a difference, a quotient and a product each), the second the length of the sum.  w, u: (..., npe)."""
    k = 3 * p * dim + (p + 1) ** dim
    return 4.0 * k * EPS * np.abs(np.asarray(w) * np.asarray(u)).sum(axis=-1)


def bound_from_abs(sum_abs, p, dim):
    """the same bound from sum |w_n u_n| (what evaluate returns)"""
    return 4.0 * (3 * p * dim + (p + 1) ** dim) * EPS * np.asarray(sum_abs, dtype=np.float64)


def plane_points(point, normal, bb0, bb1, n):
    """PlaneInterpolator::setInterpolationPoints (src/gslib_interpolator.cpp:121-190) in its order of operations:
    (3, n*n), i fastest."""
    point, normal, bb0, bb1 = (np.asarray(v, dtype=np.float64) for v in (point, normal, bb0, bb1))
    ndotp = 0.0
    for d in range(3):
        ndotp += normal[d] * point[d]
    big = max(max(abs(normal[0]), abs(normal[1])), abs(normal[2]))
    m = 0 if big == abs(normal[0]) else (1 if big == abs(normal[1]) else 2)
    a, b = [d for d in range(3) if d != m]
    cells = float(n - 1)
    da, db = (bb1[a] - bb0[a]) / cells, (bb1[b] - bb0[b]) / cells
    j, i = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    pa = (da * i + bb0[a]).ravel()
    pb = (db * j + bb0[b]).ravel()
    out = np.zeros((3, n * n))
    out[a], out[b] = pa, pb
    out[m] = (ndotp - (normal[a] * pa) - (normal[b] * pb)) / normal[m]
    return out


def random_polynomial(dim, p, seed):
    """a polynomial of total degree <= p with seeded coefficients of order one: f(X), X (dim, n)"""
    rng = np.random.default_rng(seed)
    terms = [e for e in np.ndindex(*([p + 1] * dim)) if sum(e) <= p]
    coef = rng.uniform(-1.0, 1.0, size=len(terms))

    def f(X):
        X = np.asarray(X)
        out = np.zeros(X.shape[1], dtype=X.dtype)
        for c, e in zip(coef, terms):
            t = np.full(X.shape[1], c, dtype=X.dtype)
            for d in range(dim):
                t = t * X[d] ** e[d]
            out += t
        return out

    return f


def points_in_elements(mesh, npts, seed, lo=0.02, hi=0.98):
    """npts points made as map(elem, xi), xi uniform in (lo, hi)^dim, elements drawn uniformly:
    -> (xyz (dim, npts), elem (npts,), xi (dim, npts))"""
    rng = np.random.default_rng(seed)
    elem = rng.integers(0, mesh.num_elements, size=npts)
    xi = rng.uniform(lo, hi, size=(mesh.dim, npts))
    return vertex_map(np.asarray(mesh.elem_coords)[elem], xi), elem, xi


def box(dim, warp=0.0, lengths=None, scramble=None):
    """box_hex(3, 2, 2) / box_quad(3, 2) with walls on every side (a periodic direction needs three cells, and the
    second and third have two), optionally with every element's local frame rotated at random"""
    if dim == 3:
        m = meshgen.box_hex(3, 2, 2, lengths=lengths or (1.0, 1.0, 1.0), periodic=(False, False, False), warp=warp)
    else:
        m = meshgen.box_quad(3, 2, lengths=lengths or (1.0, 1.0), periodic=(False, False), warp=warp)
    return meshgen.scramble_orientations(m, scramble) if scramble is not None else m


def affine_box(dim):
    """the affine, orientation-scrambled box of the polynomial tests"""
    return box(dim, lengths=(1.5, 1.0, 0.7)[:dim], scramble=5)
