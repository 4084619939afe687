"""Pins the numpy restatement of tests/sampling_util.py, which the library's point location and sampling are compared with:
it reproduces polynomials of total degree <= p on affine, orientation-scrambled meshes (an affine map keeps the total
degree, so the polynomial lies in the element's tensor space Q_p and nodal interpolation is exact), and its float64
evaluation stays within its own rounding bound of an extended-precision evaluation."""
import numpy as np
import pytest

import sampling_util as su
from tps_amd.rhs_operator import node_coordinates


affine_mesh = su.affine_box


@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("basis", [0, 1], ids=["legendre", "lobatto"])
@pytest.mark.parametrize("dim", [2, 3])
def test_reproduces_polynomials(dim, basis, order):
    mesh = affine_mesh(dim)
    f = su.random_polynomial(dim, order, seed=10 * order + dim)
    u = f(node_coordinates(mesh, order, basis))
    xyz, elem, xi = su.points_in_elements(mesh, 200, seed=3)
    got, _ = su.evaluate(u, elem, xi, order, basis)
    err = np.abs(got[0] - f(xyz)).max()
    print(f"dim {dim} basis {basis} p {order}: max error {err:.2e} of max |u| {np.abs(u).max():.2e}")
    assert err <= 1e-12 * np.abs(u).max()


@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("basis", [0, 1], ids=["legendre", "lobatto"])
@pytest.mark.parametrize("dim", [2, 3])
def test_float64_evaluation_is_within_its_bound_of_extended_precision(dim, basis, order):
    mesh = affine_mesh(dim)
    rng = np.random.default_rng(7)
    u = rng.standard_normal((2, mesh.num_elements * (order + 1) ** dim))
    _, elem, xi = su.points_in_elements(mesh, 200, seed=4, lo=0.0, hi=1.0)
    got, _ = su.evaluate(u, elem, xi, order, basis)
    ref, sum_abs = su.evaluate(u, elem, xi, order, basis, dtype=np.longdouble)
    b = su.bound_from_abs(sum_abs, order, dim)
    ratio = (np.abs(got - ref).astype(np.float64) / b).max()
    print(f"dim {dim} basis {basis} p {order}: max |float64 - long double| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    # bound() itself, from the weights and the values of one point
    W = su.tensor_weights(xi[:, :1], order, basis)
    npe = (order + 1) ** dim
    assert np.isclose(su.bound(W[0], u[0, elem[0] * npe:(elem[0] + 1) * npe], order, dim), b[0, 0], rtol=1e-12)


def test_newton_recovers_reference_coordinates():
    for mesh in (su.box(3, warp=0.1), su.box(2, warp=0.1)):
        xyz, elem, xi = su.points_in_elements(mesh, 20, seed=1)
        for i in range(20):
            got, its, ok = su.newton_invert(mesh.elem_coords[elem[i]], xyz[:, i])
            assert ok and its <= 6 and np.abs(got - xi[:, i]).max() <= 1e-12


def test_plane_points_lattice():
    pts = su.plane_points((0.2, 0.3, 0.4), (0.0, 0.0, 2.0), (0, 0, 0), (1, 2, 3), 3)
    assert np.array_equal(pts[0], [0, 0.5, 1] * 3) and np.array_equal(pts[1], [0, 0, 0, 1, 1, 1, 2, 2, 2])
    assert np.array_equal(pts[2], np.full(9, 0.4))
