"""A numpy restatement of the surface rule of include/tpsrhs.h (tpsrhs_patch_faces, tpsrhs_surface_integrate) and the
rounding bound that follows from its summation structure.

The rule: a face is (element, local face 2 d + s); on it the tensor Gauss-Legendre points with NQ = p + 2 per tangential
direction (the other reference directions a < b in ascending order, xi_d = s, point i + j NQ); order-1 geometry (the
bi-/trilinear map through elem_coords, MFEM vertex order); the area-weighted outward normal
N_q = (2 s - 1) sgn(det J) cof(J) e_d; dS_q = w_i w_j |N_q|, n dS = w_i w_j N_q, both times the first coordinate of the mapped
point with `radial`; a nodal field is evaluated with the operator's Lagrange basis.  Everything from the vertex coordinates
on is computed in np.longdouble, and each face's terms are summed (in longdouble) before the faces are.

The bound is derived, not measured.  With the terms of one face summed first (NQ^(dim-1) terms), the face sums of a patch
added in any order (nf_p terms), 8 dim (p + 1) roundings in the interpolations of the dim components and their products,
and 16 in the geometry of a point (the map, the cofactors, the weight),
    |device - exact| <= K_s eps S,   K_s = NQ^(dim-1) + nf_p + 8 dim (p + 1) + 16,   S = sum_q w_q G_q R_q A_q,
    G_q = |dX/da| |dX/db| (3-D; |dX/da| in 2-D) >= |N_q|,  R_q = |r_q| with the radial weight and 1 without,
    A_q = sum_nodes |l_node(xi_q)| |f_node|, summed over the dim components for FLUX.
"""
import dataclasses
import math

import numpy as np

import integrals_util as iu
import sampling_util as su
from tps_amd import meshgen

EPS = iu.EPS
LD = np.longdouble
SCALAR, FLUX, NORMAL = "scalar", "flux", "normal"

# local MFEM vertex -> lexicographic corner (bit d = reference coordinate d)
_LEX = {dim: [sum(c[d] << d for d in range(dim)) for c in su.CORNERS[dim]] for dim in (2, 3)}


# ---- which faces make a patch ----------------------------------------------------------------------------------------------
def tangential(dim, d):
    return [k for k in range(dim) if k != d]


def face_vertices(dim, f):
    """the local MFEM vertices of local face f = 2 d + s, in (ta, tb) order"""
    d, s = f >> 1, f & 1
    t = tangential(dim, d)
    out = []
    for tb in ((0, 1) if dim == 3 else (0,)):
        for ta in (0, 1):
            c = [0] * dim
            c[d] = s
            c[t[0]] = ta
            if dim == 3:
                c[t[1]] = tb
            out.append(su.CORNERS[dim].index(tuple(c)))
    return out


def patch_faces_np(mesh, attributes):
    """-> (elem, face, patch) int32: the boundary records of `mesh` with attribute attributes[p], each matched to the first
    (element, local face) in ascending order that carries its vertices"""
    dim = mesh.dim
    ev = np.asarray(mesh.elem_vertices)
    attributes = [int(a) for a in attributes]
    recs = {}
    for b, ids in enumerate(np.asarray(mesh.bdr_vertices)):
        recs.setdefault(tuple(sorted(int(i) for i in ids)), []).append(b)
    out = []
    for e in range(mesh.num_elements):
        for f in range(2 * dim):
            key = tuple(sorted(int(ev[e, v]) for v in face_vertices(dim, f)))
            for b in recs.pop(key, []):
                a = int(mesh.bdr_attributes[b])
                if a in attributes:
                    out.append((e, f, attributes.index(a)))
    assert not recs, "a boundary record that is no element's face"
    a = np.array(out, dtype=np.int32).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def face_centres(mesh, elem, face):
    ex = np.asarray(mesh.elem_coords)
    return np.array([ex[e, face_vertices(mesh.dim, f)].mean(axis=0) for e, f in zip(elem, face)]).reshape(-1, mesh.dim)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def face_points(dim, order, f):
    """xi (dim, NQ^(dim-1)) of local face f with point i + j NQ (i along a), and the products of the 1-D weights"""
    g, w = iu.rule_1d(order)
    d, s = f >> 1, f & 1
    t = tangential(dim, d)
    nq = g.size
    if dim == 2:
        i = np.arange(nq)
        xi = np.zeros((2, nq))
        xi[t[0]] = g[i]
        wprod = w[i]
    else:
        j, i = np.meshgrid(np.arange(nq), np.arange(nq), indexing="ij")
        i, j = i.ravel(), j.ravel()
        xi = np.zeros((3, nq * nq))
        xi[t[0]] = g[i]
        xi[t[1]] = g[j]
        wprod = w[i] * w[j]
    xi[d] = float(s)
    return xi, wprod


def face_geometry(ex, xi, f):
    """ex (nv, dim) the element's vertices (MFEM order), xi (dim, nq) -> x (dim, nq), N (dim, nq) the area-weighted outward
    normal, G (nq,) = the product of the lengths of the tangential derivatives; np.longdouble"""
    dim = xi.shape[0]
    d, s = f >> 1, f & 1
    ex = np.asarray(ex, dtype=LD)
    xi = np.asarray(xi, dtype=LD)
    nq = xi.shape[1]
    x = np.zeros((dim, nq), dtype=LD)
    J = np.zeros((dim, dim, nq), dtype=LD)  # J[a, k] = dx_a / dxi_k
    for v, c in enumerate(su.CORNERS[dim]):
        fac = [xi[k] if c[k] else 1 - xi[k] for k in range(dim)]
        x += ex[v][:, None] * np.prod(np.stack(fac), axis=0)[None, :]
        for k in range(dim):
            dshp = np.full(nq, 1.0 if c[k] else -1.0, dtype=LD)
            for m in range(dim):
                if m != k:
                    dshp = dshp * fac[m]
            J[:, k, :] += ex[v][:, None] * dshp[None, :]
    if dim == 2:
        o = 1 - d
        cof = np.stack([J[1, o], -J[0, o]]) if d == 0 else np.stack([-J[1, o], J[0, o]])
        G = np.sqrt(J[0, o] ** 2 + J[1, o] ** 2)
    else:
        p, q = (d + 1) % 3, (d + 2) % 3
        cof = np.stack([J[1, p] * J[2, q] - J[2, p] * J[1, q], J[2, p] * J[0, q] - J[0, p] * J[2, q],
                        J[0, p] * J[1, q] - J[1, p] * J[0, q]])
        G = np.sqrt((J[:, p] ** 2).sum(axis=0)) * np.sqrt((J[:, q] ** 2).sum(axis=0))
    det = (cof * J[:, d]).sum(axis=0)
    N = (2 * s - 1) * np.sign(det) * cof
    return x, N, G


def constant_K(dim, order, nfaces):
    return (order + 2) ** (dim - 1) + nfaces + 8 * dim * (order + 1) + 16


def integrate(mesh, order, basis_type, elem, face, patch, num_patches, field, form=SCALAR, radial=False):
    """field: (nrows, NDofs) for SCALAR / NORMAL, (nrows, dim, NDofs) for FLUX.
    -> dict(val (npatch, nrows[, dim]), S (npatch, nrows), K (npatch,)): float64"""
    dim = mesh.dim
    npe = (order + 1) ** dim
    field = np.asarray(field, dtype=np.float64)
    field = field.reshape((-1, dim, field.shape[-1])) if form == FLUX else field.reshape((-1, 1, field.shape[-1]))
    nrows = field.shape[0]
    od = dim if form == NORMAL else 1
    ex = np.asarray(mesh.elem_coords)
    terms = [[[] for _ in range(nrows * od)] for _ in range(num_patches)]
    bound = [[[] for _ in range(nrows)] for _ in range(num_patches)]
    nf = np.zeros(num_patches, dtype=np.int64)
    tabs = {}
    for e, f, p in zip(elem, face, patch):
        e, f, p = int(e), int(f), int(p)
        nf[p] += 1
        if f not in tabs:
            xi, wprod = face_points(dim, order, f)
            tabs[f] = (xi, wprod.astype(LD), su.tensor_weights(xi, order, basis_type, dtype=LD))
        xi, wprod, T = tabs[f]
        x, N, G = face_geometry(ex[e], xi, f)
        w = wprod * x[0] if radial else wprod
        wabs = wprod * np.abs(x[0]) if radial else wprod
        u = field[:, :, e * npe:(e + 1) * npe].astype(LD)  # (nrows, ncomp, npe)
        vals = u @ T.T                                      # (nrows, ncomp, nq)
        A = (np.abs(u) @ np.abs(T).T).sum(axis=1)           # (nrows, nq)
        for r in range(nrows):
            if form == SCALAR:
                terms[p][r].append((w * np.sqrt((N * N).sum(axis=0)) * vals[r, 0]).sum())
            elif form == FLUX:
                terms[p][r].append((w[None, :] * N * vals[r]).sum())
            else:
                for k in range(dim):
                    terms[p][r * dim + k].append((w * N[k] * vals[r, 0]).sum())
            bound[p][r].append((wabs * G * A[r]).sum())
    val = np.array([[float(sum(t, LD(0))) for t in tp] for tp in terms]).reshape((num_patches, nrows) + ((dim,) if od > 1 else ()))
    S = np.array([[float(sum(t, LD(0))) for t in tp] for tp in bound]).reshape(num_patches, nrows)
    return dict(val=val, S=S, K=np.array([constant_K(dim, order, int(n)) for n in nf]))


def check(name, got, ref, exact=None, log=None):
    """prints the achieved error in units of eps * S and asserts the bound K_s eps S (+ 8 eps |exact| against a closed form,
    which replaces the restatement's value as the reference); -> the largest error / bound ratio"""
    got = np.asarray(got, dtype=np.float64)
    want = ref["val"] if exact is None else np.broadcast_to(np.asarray(exact, dtype=np.float64), got.shape)
    S = ref["S"] if got.ndim == 2 else ref["S"][:, :, None]
    K = ref["K"][:, None] if got.ndim == 2 else ref["K"][:, None, None]
    bound = K * EPS * S + (8 * EPS * np.abs(want) if exact is not None else 0.0)
    err = np.abs(got - want)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if got.size else 0.0
    line = f"{name}: K_s <= {int(ref['K'].max())}; max error / bound = {ratio:.4f}"
    print(line)
    if log is not None:
        log.append((name, ratio))
    assert ok.all(), (name, err, bound)
    return ratio


# ---- meshes and closed forms -------------------------------------------------------------------------------------------------
def planar_box(dim, n, seed=3, amp=0.18):
    """the unit box with walls all round (attributes 1 + 2 d + s), n cells per direction, every vertex moved by up to amp cell
    sizes in each direction in which it is not on the boundary: interior vertices move freely (integrals_util.perturbed_box),
    vertices of a box face move WITHIN it, edge vertices along their edge, corners not at all.  The faces stay planar and the
    domain the unit box, but the boundary quadrilaterals are no parallelograms."""
    n = tuple(n)
    m = (meshgen.box_hex if dim == 3 else meshgen.box_quad)(*n, periodic=(False,) * dim)
    rng = np.random.default_rng(seed)
    shift = rng.uniform(-amp, amp, size=(m.num_vertices, dim)) / np.array(n, dtype=np.float64)
    ex = np.array(m.elem_coords, dtype=np.float64)
    free = (ex > 1e-12) & (ex < 1.0 - 1e-12)  # (ne, nv, dim): per direction
    ex = ex + np.where(free, shift[np.asarray(m.elem_vertices)], 0.0)
    return dataclasses.replace(m, elem_coords=ex)


def polynomial_terms(dim, p, seed):
    """the coefficients and exponents integrals_util.polynomial(dim, p, seed) draws"""
    rng = np.random.default_rng(seed)
    terms = [e for e in np.ndindex(*([p + 1] * dim)) if sum(e) <= p]
    return rng.uniform(-1.0, 1.0, size=len(terms)), terms


def polynomial_eval(coef, terms, X):
    out = np.zeros(X.shape[1])
    for c, e in zip(coef, terms):
        t = np.full(X.shape[1], c)
        for d in range(X.shape[0]):
            t = t * X[d] ** e[d]
        out += t
    return out


def polynomial_derivative(coef, terms, k):
    """(coef, terms) of d/dx_k"""
    out = [(c * e[k], tuple(ed - (1 if d == k else 0) for d, ed in enumerate(e))) for c, e in zip(coef, terms) if e[k] > 0]
    return [c for c, _ in out], [e for _, e in out]


def box_face_integral(coef, terms, d, s):
    """int of sum_t c_t prod_k x_k^e_k over the face x_d = s of the unit box"""
    return math.fsum(c * (float(s) ** e[d] if e[d] else 1.0) * math.prod(1.0 / (ek + 1) for k, ek in enumerate(e) if k != d)
                     for c, e in zip(coef, terms))


def box_patches(mesh):
    """(elem, face, patch) of the 2 dim sides of a box mesh with the default attributes 1 + 2 d + s, patch = 2 d + s"""
    return patch_faces_np(mesh, [1 + k for k in range(2 * mesh.dim)])
