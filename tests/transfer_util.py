"""Shared inputs of the device-location and mesh-to-mesh transfer tests (tests/test_locate_one.py, tests/test_gpu_locate.py,
tests/test_gpu_transfer.py): the meshes, the seeded point sets -- interior points, images of reference points with
coordinates exactly 0 or 1 (faces, edges, vertices), points outside the mesh, one NaN -- and the pairs of non-matching
boxes.  Geometry helpers come from tests/sampling_util.py."""
import dataclasses

import numpy as np

import sampling_util as su
from tps_amd import capi, cases, meshgen


def walls(mesh):
    return [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]


def box(dim, n, lengths, warp=0.0, scramble=None, origin=None):
    """n cells per direction (a tuple) with walls on every side, optionally warped, scrambled and shifted"""
    if dim == 3:
        m = meshgen.box_hex(*n, lengths=lengths, periodic=(False, False, False), warp=warp)
    else:
        m = meshgen.box_quad(*n, lengths=lengths, periodic=(False, False), warp=warp)
    if scramble is not None:
        m = meshgen.scramble_orientations(m, scramble)
    if origin is not None:
        m = dataclasses.replace(m, elem_coords=np.asarray(m.elem_coords) + np.asarray(origin, dtype=np.float64))
    return m


def box_case(mesh, order, basis=0):
    """a dry-air operator's inputs on `mesh`: only geometry and basis matter to location and transfer"""
    return cases.Case(f"box{mesh.dim}d_p{order}_b{basis}", mesh, capi.Disc(order, basis, basis, 0, 0),
                      capi.dry_air_physics(capi.NS), walls(mesh))


LOCATE_MESHES = {
    "hex_warped_scrambled": lambda: box(3, (3, 3, 3), (1.5, 1.0, 0.7), warp=0.1, scramble=7),
    "quad_warped": lambda: box(2, (5, 5), (1.5, 1.0), warp=0.1),
    "ogrid": lambda: meshgen.ogrid_cylinder(4, 12, 3),
}


def point_set(mesh, n_interior, n_boundary, seed):
    """(dim, npts): n_interior points strictly inside elements, n_boundary images of reference points with one, two or dim
    coordinates exactly 0 or 1, points outside the bounding box on every side, the axis of the O-grid's hole when the mesh
    has one (inside the box, in no element) and a NaN -- shuffled, so that a wave of the device locator meets all kinds."""
    dim = mesh.dim
    rng = np.random.default_rng(seed)
    ex = np.asarray(mesh.elem_coords)
    inner, _, _ = su.points_in_elements(mesh, n_interior, seed)
    eb = rng.integers(0, mesh.num_elements, size=n_boundary)
    xi = rng.uniform(0.02, 0.98, size=(dim, n_boundary))
    for i in range(n_boundary):
        pinned = rng.choice(dim, size=1 + i % dim, replace=False)  # 1: a face, 2: an edge (3-D) or a vertex (2-D), 3: a vertex
        xi[pinned, i] = rng.integers(0, 2, size=len(pinned))
    bdr = su.vertex_map(ex[eb], xi)
    X = ex.reshape(-1, dim)
    lo, hi = X.min(axis=0), X.max(axis=0)
    mid, ext = 0.5 * (lo + hi), hi - lo
    outside = []
    for d in range(dim):
        for s in (-1.0, 1.0):
            for frac in (0.05, 0.3, 3.0):
                p = mid + 0.2 * ext * rng.uniform(-1.0, 1.0, size=dim)
                p[d] = mid[d] + s * (0.5 + frac) * ext[d]
                outside.append(p)
    if np.abs(np.linalg.norm(X[:, :2], axis=1).min() - 0.5) < 1e-12 and dim == 3:  # the O-grid: its cylinder is a hole
        outside += [np.array([0.0, 0.0, mid[2]]), np.array([0.2, -0.1, mid[2]])]
    nan = mid.copy()
    nan[0] = np.nan
    pts = np.concatenate([inner, bdr, np.array(outside).T, nan[:, None]], axis=1)
    return np.ascontiguousarray(pts[:, rng.permutation(pts.shape[1])])


# The pairs of the polynomial test: an affine, orientation-scrambled source with three (3-D) or four (2-D) cells per
# direction and an affine target with 2 and 4 cells per direction strictly inside it, shifted so that no face of the target
# lies on a face of the source.
def source_box(dim):
    return box(3, (3, 3, 3), (1.5, 1.0, 0.7), scramble=5) if dim == 3 else box(2, (4, 4), (1.5, 1.0), scramble=5)


def target_box(dim):
    if dim == 3:
        return box(3, (2, 4, 2), (1.2, 0.8, 0.5), origin=(0.13, 0.07, 0.09))
    return box(2, (2, 4), (1.2, 0.8), origin=(0.13, 0.07))
