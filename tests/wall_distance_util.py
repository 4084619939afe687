"""The wall-distance function restated in numpy (the contract of include/tpsrhs.h, "the wall-distance function"; the
reference's evaluateDistanceSerial, src/utils.cpp:371-514), the selection of the wall faces restated from the mesh
arrays, the meshes of the tests and their closed forms.  Nothing here calls the library."""
import functools

import numpy as np

from tps_amd import meshgen
from tps_amd.rhs_operator import node_coordinates

EPS = np.finfo(np.float64).eps
_CORNERS = {2: meshgen._QUAD_CORNERS, 3: meshgen._HEX_CORNERS}


def local_face_corners(dim, f):
    """MFEM vertex numbers of local face f = 2 d + s (xi_d = s) of an element, in (ta, tb) corner order: the tangential
    axes are the remaining axes in increasing order (tps_amd/csrc/topology.hpp)."""
    d, s = f >> 1, f & 1
    tang = [a for a in range(dim) if a != d]
    out = []
    for t in range(1 << (dim - 1)):
        bits = [0] * dim
        bits[d] = s
        for i, a in enumerate(tang):
            bits[a] = (t >> i) & 1
        out.append(int(np.where((_CORNERS[dim] == bits).all(axis=1))[0][0]))
    return out


def wall_faces_np(mesh, attributes):
    """(nf, 2^(dim-1), dim): corners of the boundary faces whose attribute is in `attributes`, from the owning element's
    elem_coords, in ascending (element, local face) order; a record is taken by the first element face that carries it."""
    dim = mesh.dim
    recs = {}
    for b, v in enumerate(mesh.bdr_vertices):
        recs.setdefault(tuple(sorted(int(i) for i in v)), []).append(b)
    faces = []
    for e in range(mesh.num_elements):
        for f in range(2 * dim):
            c = local_face_corners(dim, f)
            key = tuple(sorted(int(i) for i in mesh.elem_vertices[e][c]))
            for b in recs.pop(key, []):
                if int(mesh.bdr_attributes[b]) in attributes:
                    faces.append(mesh.elem_coords[e][c])
    assert not recs, "a boundary record that is no element's face"
    return np.array(faces, dtype=np.float64).reshape(-1, 1 << (dim - 1), dim)


def wall_distance_np(xp, faces, chunk=2048, return_iterations=False):
    """xp (dim, N) node coordinates, faces (nf, 2^(dim-1), dim), corner = ta + 2 tb -> distance (N,).
    Per pair: Gauss-Newton from the face centre with the reference's stopping rule, clamp to the reference square, the
    Euclidean distance; the minimum over the faces with `<` from 1e30 (a NaN never wins)."""
    dim, N = xp.shape
    nf = faces.shape[0]
    out = np.full(N, 1e30)
    iters = np.zeros((N, nf), dtype=np.int64)
    if nf == 0:
        return (out, iters) if return_iterations else out
    F = np.asarray(faces, dtype=np.float64)
    a = F[:, 0]
    b = F[:, 1] - F[:, 0]
    if dim == 3:
        c = F[:, 2] - F[:, 0]
        d = (F[:, 3] - F[:, 1]) - (F[:, 2] - F[:, 0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for i0 in range(0, N, chunk):
            P = xp[:, i0:i0 + chunk].T[:, None, :]  # (n, 1, dim)
            n = P.shape[0]
            s = np.full((n, nf), 0.5)
            t = np.full((n, nf), 0.5)

            def evaluate(s, t):
                if dim == 3:
                    J1 = b[None] + d[None] * t[..., None]
                    J2 = c[None] + d[None] * s[..., None]
                    X = a[None] + s[..., None] * J1 + t[..., None] * c[None]
                    dx = P - X
                    return dx, J1, J2, (J1 * dx).sum(-1), (J2 * dx).sum(-1)
                J1 = np.broadcast_to(b[None], (n, nf, dim))
                dx = P - (a[None] + s[..., None] * J1)
                return dx, J1, None, (J1 * dx).sum(-1), np.zeros((n, nf))

            dx, J1, J2, g1, g2 = evaluate(s, t)
            r0 = np.sqrt(g1 * g1 + g2 * g2)
            rnorm = r0.copy()
            it = np.zeros((n, nf), dtype=np.int64)
            while True:
                active = (rnorm > 1e-16) & (rnorm / r0 > 1e-10) & (it < 20)
                if not active.any():
                    break
                A11 = (J1 * J1).sum(-1)
                if dim == 3:
                    A12, A22 = (J1 * J2).sum(-1), (J2 * J2).sum(-1)
                    det = A11 * A22 - A12 * A12
                    s = np.where(active, s + (A22 * g1 - A12 * g2) / det, s)
                    t = np.where(active, t + (A11 * g2 - A12 * g1) / det, t)
                else:
                    s = np.where(active, s + g1 / A11, s)
                dx, J1, J2, g1, g2 = evaluate(s, t)
                rnorm = np.where(active, np.sqrt(g1 * g1 + g2 * g2), rnorm)
                it += active

            def clamp(v):  # keeps a NaN
                return np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))

            dx = evaluate(clamp(s), clamp(t))[0]
            dist = np.sqrt((dx * dx).sum(-1))
            best = np.fmin.reduce(dist, axis=1)  # the NaNs lose, as with `<`
            out[i0:i0 + n] = np.fmin(1e30, best)
            iters[i0:i0 + n] = it
    return (out, iters) if return_iterations else out


def bbox_diagonal(xp):
    return float(np.sqrt(((xp.max(axis=1) - xp.min(axis=1)) ** 2).sum()))


# ---- the meshes of the tests, their wall attributes and closed forms ----------------------------------------------------------
def tube():
    return meshgen.annulus_quad(3, 5, r_in=0.0, r_out=0.05, length=0.25)


def tube_exact(X):
    return 0.05 - X[0]


def cylinder():
    return meshgen.ogrid_cylinder(3, 8, 3)


def chords_exact(X, r_in=0.5, ntheta=8):
    """minimum over the chords of the inner polygon of the 2-D point-to-segment distance"""
    th = 2.0 * np.pi * np.arange(ntheta + 1) / ntheta
    A = r_in * np.stack([np.cos(th[:-1]), np.sin(th[:-1])], axis=1)
    B = r_in * np.stack([np.cos(th[1:]), np.sin(th[1:])], axis=1)
    P = X[:2].T[:, None, :]
    AB = (B - A)[None]
    u = np.clip(((P - A[None]) * AB).sum(-1) / (AB * AB).sum(-1), 0.0, 1.0)
    D = P - (A[None] + u[..., None] * AB)
    return np.sqrt((D * D).sum(-1)).min(axis=1)


def partial_wall_box():
    """the bottom of a 4 x 3 x 3 box split into attribute 7 (x < 0.5) and 8; the other sides 1..4 and 6"""
    attrs = {(d, s): 1 + 2 * d + s for d in range(3) for s in (0, 1)}
    attrs[(2, 0)] = lambda centre: np.where(centre[:, 0] < 0.5, 7, 8)
    return meshgen.box_hex(4, 3, 3, periodic=(False,) * 3, bdr_attr=attrs)


def partial_wall_exact(X):
    return np.sqrt(np.maximum(X[0] - 0.5, 0.0) ** 2 + X[2] ** 2)


def bottom_box(nx, ny, nz, warp=0.0):
    """a box with walls all round; its bottom z = 0 is attribute 5"""
    return meshgen.box_hex(nx, ny, nz, periodic=(False,) * 3, warp=warp)


CASES = {  # name -> (mesh, wall attributes, closed form or None)
    "tube": (tube, (3,), tube_exact),
    "cylinder": (cylinder, (3,), chords_exact),
    "partial": (partial_wall_box, (7,), partial_wall_exact),
    "tiles143": (lambda: bottom_box(13, 11, 2), (5,), lambda X: X[2]),
    # 285 faces: two full LDS tiles of 128 faces (WD_TILE in tps_amd/csrc/wall_distance.hpp) and 29 more
    "tiles285": (lambda: bottom_box(19, 15, 2), (5,), lambda X: X[2]),
    "warped": (lambda: bottom_box(4, 4, 4, warp=0.05), (5,), None),
}


@functools.lru_cache(maxsize=None)
def restated(name, order, basis):
    """(mesh, faces, X, L, distance of the restatement): computed once per case, shared and left unchanged"""
    make, attrs, _ = CASES[name]
    mesh = make()
    faces = wall_faces_np(mesh, attrs)
    X = node_coordinates(mesh, order, basis)
    d = wall_distance_np(X, faces)
    for arr in (faces, X, d):
        arr.setflags(write=False)
    return mesh, faces, X, bbox_diagonal(X), d
