"""tpsrhs_locate_points and tpsrhs_plane_points through the C ABI (host only: no device is touched), against the numpy
restatement of tests/sampling_util.py."""
import ctypes as C

import numpy as np
import pytest

import sampling_util as su
from tps_amd import capi, meshgen
from tps_amd.rhs_operator import TpsRhsError, locate_points, plane_points

MESHES = {
    "box_hex_warped": lambda: su.box(3, warp=0.1),
    "ogrid_cylinder": lambda: meshgen.ogrid_cylinder(4, 12, 3),
    "box_quad_warped": lambda: su.box(2, warp=0.1),
    "annulus_quad": lambda: meshgen.annulus_quad(3, 5),
}


def _extent(mesh):
    X = np.asarray(mesh.elem_coords).reshape(-1, mesh.dim)
    return float((X.max(axis=0) - X.min(axis=0)).max())


@pytest.mark.parametrize("name", list(MESHES))
def test_round_trip(name):
    mesh = MESHES[name]()
    xyz, elem, xi = su.points_in_elements(mesh, 400, seed=11)
    got_e, got_xi = locate_points(mesh, xyz)
    assert (got_e >= 0).all()
    assert np.array_equal(got_e, elem)
    dxi = np.abs(got_xi - xi).max()
    back = su.vertex_map(np.asarray(mesh.elem_coords)[got_e], got_xi)
    dx = np.abs(back - xyz).max()
    print(f"{name}: max |xi - xi_lib| = {dxi:.2e}, max |map(xi_lib) - x| = {dx:.2e} of L = {_extent(mesh):.2e}")
    assert dxi <= 1e-12
    assert dx <= 1e-12 * _extent(mesh)
    # the restatement's Newton agrees on a few points
    for i in range(0, 400, 67):
        r, its, ok = su.newton_invert(mesh.elem_coords[elem[i]], xyz[:, i])
        assert ok and np.abs(r - got_xi[:, i]).max() <= 1e-12


def test_points_outside():
    mesh = meshgen.ogrid_cylinder(4, 12, 3)  # r in [0.5, 10], the cylinder is a hole
    X = np.asarray(mesh.elem_coords).reshape(-1, 3)
    zmid = 0.5 * (X[:, 2].min() + X[:, 2].max())
    pts = np.array([[0.0, 0.0, zmid], [0.2, -0.1, zmid],  # inside the hole
                    [25.0, 0.0, zmid], [0.0, -30.0, zmid], [1.0, 1.0, X[:, 2].max() + 1.0],  # outside the bounding box
                    [9.0, 9.0, zmid],  # inside the box, outside the outer circle
                    [np.nan, 0.0, zmid]]).T
    e, xi = locate_points(mesh, pts)
    assert (e == -1).all() and not xi.any()
    mesh2 = su.box(2, warp=0.1)
    e, xi = locate_points(mesh2, np.array([[-0.5, 0.3], [0.5, 7.0]]).T)
    assert (e == -1).all() and not xi.any()
    # found and not-found points mixed: the found ones are unaffected
    xyz, elem, ref = su.points_in_elements(mesh, 5, seed=2)
    both = np.concatenate([pts[:, :3], xyz], axis=1)
    e, xi = locate_points(mesh, both)
    assert np.array_equal(e, np.concatenate([[-1, -1, -1], elem])) and np.abs(xi[:, 3:] - ref).max() <= 1e-12


def test_interior_faces_go_to_the_lower_element():
    mesh = su.box(3, lengths=(1.5, 1.0, 0.7))
    ex = np.asarray(mesh.elem_coords)
    rng = np.random.default_rng(5)
    for xface in (0.5, 1.0):
        n = 40
        pts = np.stack([np.full(n, xface), rng.uniform(0.05, 0.45, n), rng.uniform(0.02, 0.33, n)])
        e, xi = locate_points(mesh, pts)
        assert (e >= 0).all()
        for i in range(n):
            # every element whose closed box holds the point accepts it: the lowest index must have won
            lo, hi = ex.min(axis=1), ex.max(axis=1)
            holds = np.where(((pts[:, i] >= lo - 1e-12) & (pts[:, i] <= hi + 1e-12)).all(axis=1))[0]
            assert len(holds) == 2 and e[i] == holds.min()
        assert np.abs(su.vertex_map(ex[e], xi) - pts).max() <= 1e-12
    # the same after scrambling the orientations: geometry and element order are unchanged
    s = meshgen.scramble_orientations(mesh, 3)
    pts = np.stack([np.full(10, 0.5), np.linspace(0.1, 0.4, 10), np.full(10, 0.2)])
    assert np.array_equal(locate_points(s, pts)[0], locate_points(mesh, pts)[0])


@pytest.mark.parametrize("name", ["box_hex_warped", "annulus_quad"])
def test_partitioned_meshes_find_every_point_somewhere(name):
    mesh = MESHES[name]()
    parts = meshgen.partition(mesh, 2)
    xyz, elem, xi = su.points_in_elements(mesh, 400, seed=13)
    # plus points exactly on element faces (reference coordinate 0 or 1), which may lie on the cut
    on_face = xi.copy()
    on_face[0] = np.round(on_face[0])
    xyz = np.concatenate([xyz, su.vertex_map(np.asarray(mesh.elem_coords)[elem], on_face)], axis=1)
    found = np.zeros(xyz.shape[1], dtype=int)
    for part in parts:
        e, r = locate_points(part, xyz)
        ok = e >= 0
        found += ok
        back = su.vertex_map(np.asarray(part.elem_coords)[e[ok]], r[:, ok])
        assert np.abs(back - xyz[:, ok]).max() <= 1e-12 * _extent(mesh)
    assert (found >= 1).all()
    assert (found[:400] == 1).all()  # interior points belong to exactly one part


PLANES = [((0.3, 0.1, -0.2), (1.0, 0.0, 0.0)), ((0.3, 0.1, -0.2), (0.0, -2.0, 0.0)), ((0.3, 0.1, -0.2), (0.0, 0.0, 0.5)),
          ((0.3, 0.1, -0.2), (0.9, 0.3, -0.2)), ((0.3, 0.1, -0.2), (0.2, -0.8, 0.5)), ((0.3, 0.1, -0.2), (0.1, 0.6, 0.7)),
          ((0.3, 0.1, -0.2), (0.5, 0.5, 0.1))]  # a tie between x and y: the first wins


@pytest.mark.parametrize("point,normal", PLANES)
@pytest.mark.parametrize("n", [2, 7])
def test_plane_points_equal_the_restatement_bit_for_bit(point, normal, n):
    bb0, bb1 = (-1.0, -0.5, -2.0), (1.5, 0.75, 3.1)
    got = plane_points(point, normal, bb0, bb1, n)
    ref = su.plane_points(point, normal, bb0, bb1, n)
    assert got.shape == (3, n * n) and np.array_equal(got, ref)
    # the points lie on the plane
    r = np.tensordot(np.asarray(normal), got - np.asarray(point)[:, None], axes=(0, 0))
    assert np.abs(r).max() <= 1e-13


def test_status_codes():
    lib = capi.load()
    mesh = su.box(2)
    ma = capi.MeshArgs(mesh)
    xyz = np.array([[0.1], [0.2]])
    e, r = np.zeros(1, dtype=np.int32), np.zeros((2, 1))
    args = (C.byref(ma.c), 1, xyz.ctypes.data, 0.0, e.ctypes.data, r.ctypes.data)
    assert lib.tpsrhs_locate_points(*args) == 0 and e[0] >= 0
    for k, bad in ((0, None), (1, -1), (2, None), (4, None), (5, None), (3, float("nan"))):
        a = list(args)
        a[k] = bad
        assert lib.tpsrhs_locate_points(*a) == capi.ERR_INVALID_ARGUMENT, k
        assert "tpsrhs_locate_points" in lib.tpsrhs_last_error().decode()
    assert lib.tpsrhs_locate_points(C.byref(ma.c), 0, None, 0.0, None, None) == 0  # no points: nothing to do
    ma.c.dim = 4
    assert lib.tpsrhs_locate_points(*args) == capi.ERR_INVALID_ARGUMENT
    ma.c.dim = 2
    # a tolerance <= 0 is the default 1e-10: a point 1e-11 beyond the boundary is found, one 1e-9 beyond is not
    near = np.array([[-1e-11, -1e-9], [0.2, 0.2]])
    e2, _ = locate_points(mesh, near, tol=-1.0)
    assert e2[0] >= 0 and e2[1] == -1
    assert locate_points(mesh, near, tol=1e-8)[0][1] >= 0
    v = (C.c_double * 3)(0.0, 0.0, 1.0)
    out = np.zeros((3, 4))
    assert lib.tpsrhs_plane_points(v, v, v, v, 2, out.ctypes.data) == 0
    assert lib.tpsrhs_plane_points(v, v, v, v, 1, out.ctypes.data) == capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_plane_points(None, v, v, v, 2, out.ctypes.data) == capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_plane_points(v, v, v, v, 2, None) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(TpsRhsError):
        plane_points((0, 0, 0), (0, 0, 1), (0, 0, 0), (1, 1, 1), 1)
