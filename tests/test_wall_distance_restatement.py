"""The numpy restatement of the wall-distance function (tests/wall_distance_util.py), which the device tests compare
with, pinned by closed forms: a straight tube, the polygonal cylinder of the O-grid, a wall that covers part of a side (the
clamp at its edge), no wall at all.  L is the diagonal of the nodes' bounding box; the bound is 16 eps L."""
import numpy as np
import pytest

import wall_distance_util as wd
from tps_amd.rhs_operator import node_coordinates


def _check(name, order, basis):
    mesh, faces, X, L, d = wd.restated(name, order, basis)
    exact = wd.CASES[name][2](X)
    err = np.abs(d - exact).max()
    print(f"{name} p={order} basis={basis}: {faces.shape[0]} faces, {X.shape[1]} nodes, max error {err / (wd.EPS * L):.2f} eps L")
    assert err <= 16 * wd.EPS * L
    return faces


@pytest.mark.parametrize("order,basis", [(2, 0), (3, 1)])
def test_tube(order, basis):
    assert _check("tube", order, basis).shape == (5, 2, 2)


def test_cylinder():
    assert _check("cylinder", 2, 0).shape == (24, 4, 3)


def test_partial_wall_clamps_at_its_edge():
    faces = _check("partial", 2, 0)
    assert faces.shape == (6, 4, 3) and faces[..., 0].max() == 0.5
    _, _, X, _, d = wd.restated("partial", 2, 0)
    assert (X[0] > 0.5).any() and np.all(d[X[0] > 0.5] > X[2][X[0] > 0.5])  # beyond the edge the foot is ON the edge


def test_no_wall_face_gives_1e30():
    X = node_coordinates(wd.tube(), 2, 0)
    d = wd.wall_distance_np(X, wd.wall_faces_np(wd.tube(), ()))
    assert d.shape == (X.shape[1],) and np.all(d == 1e30)


def test_collapsed_face_never_wins():
    X = node_coordinates(wd.tube(), 1, 0)
    faces = wd.wall_faces_np(wd.tube(), (3,))
    dead = np.broadcast_to(faces[0, 0], (1, 2, 2))  # both corners in one point: J = 0, the update is 0 / 0
    d = wd.wall_distance_np(X, np.concatenate([dead, faces, dead]))
    assert np.array_equal(d, wd.wall_distance_np(X, faces))


def test_warped_faces_converge_within_15_iterations():
    mesh, faces, X, L, d = wd.restated("warped", 2, 0)
    d2, it = wd.wall_distance_np(X, faces, return_iterations=True)
    assert np.array_equal(d, d2) and it.size == 27648
    print("iterations: max", it.max(), "mean", it.mean())
    assert it.max() <= 15
    assert np.all(d <= X[2] + 0.05 * 0.25 + 1e-12) and np.all(d > 0)  # the bottom is displaced by at most warp * h
