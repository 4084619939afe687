"""tpsrhs_quadrature_points (host only, tps_amd/csrc/quadrature_points.hpp) against the numpy restatement of the rule
(tests/integrals_util.py): the points to 16 eps times the bounding-box diagonal, the weights to the rounding of det J, the
sum of the weights against the area / volume of the mesh, and the refusals.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import integrals_util as iu
from tps_amd import capi, meshgen
from tps_amd.rhs_operator import quadrature_points

EPS = iu.EPS

MESHES = {
    "ring2d": lambda: iu.ring_quad(4, 12),
    "annulus_rz": lambda: meshgen.annulus_quad(3, 5, r_in=0.0, r_out=0.05, length=0.25),
    "hexbox": lambda: iu.perturbed_box(3, (3, 2, 2)),
    "quadbox_scrambled": lambda: meshgen.scramble_orientations(iu.perturbed_box(2, (3, 2)), 5),
    "hexbox_scrambled": lambda: meshgen.scramble_orientations(iu.perturbed_box(3, (3, 2, 2)), 7),
    "ring3d": lambda: meshgen.ogrid_cylinder(3, 8, 3),
}


@pytest.mark.parametrize("order", [1, 2, 3, 5])
@pytest.mark.parametrize("name", list(MESHES))
def test_points_and_weights_match_the_restatement(name, order):
    mesh = MESHES[name]()
    dim, nqd = mesh.dim, (order + 2) ** mesh.dim
    xyz, w = quadrature_points(mesh, order)
    ref_xyz, ref_w = iu.geometry(mesh, order)
    assert xyz.shape == (dim, mesh.num_elements * nqd) and w.shape == (mesh.num_elements * nqd,)
    ex = np.asarray(mesh.elem_coords)
    diag = float(np.sqrt(((ex.reshape(-1, dim).max(axis=0) - ex.reshape(-1, dim).min(axis=0)) ** 2).sum()))
    err = np.abs(xyz - ref_xyz.astype(np.float64)).max() / (EPS * diag)
    # det J is a sum of (dim = 3: six) products of dim entries of J, each a combination of vertex differences no larger than
    # the element's own bounding-box diagonal h_e and carrying at most 6 roundings: 6 (3 * 6 + 2) + 5 = 125 < 128 eps h_e^dim
    h = np.sqrt(((ex.max(axis=1) - ex.min(axis=1)) ** 2).sum(axis=1))  # (ne,)
    _, wprod = iu.reference_points(dim, order)
    scale = (h[:, None] ** dim * wprod[None, :]).ravel()
    werr = (np.abs(w - ref_w.astype(np.float64)) / (EPS * scale)).max()
    # ... and each of the dim 1-D weights 1 / ((1 - z^2) P_n'(z)^2) comes from an NQ-step recurrence for P_n' (about 4 roundings
    # a step, doubled by the square): 8 NQ eps relative per direction
    wbound = 128 + 8 * dim * (order + 2)
    print(f"{name} p={order}: points {err:.3f} eps diag (bound 16); weights {werr:.3f} eps h^dim w (bound {wbound})")
    assert err <= 16.0
    assert werr <= wbound
    assert (w > 0).all()


@pytest.mark.parametrize("order", [1, 3, 5])
def test_sum_of_weights_is_the_area(order):
    ring = iu.ring_quad(4, 12)
    area = iu.shoelace_areas(np.asarray(ring.elem_coords)).astype(np.longdouble).sum()
    _, w = quadrature_points(ring, order)
    K = iu.constant_K(ring, order)
    err = abs(float(w.astype(np.longdouble).sum() - area)) / (EPS * float(area))
    print(f"ring p={order}: |sum w - area| = {err:.3f} eps area (bound K = {K})")
    assert err <= K
    # the extruded ring: every hexahedron is its quadrilateral times span / nz
    nz, span = 3, 2.0
    cyl = meshgen.ogrid_cylinder(3, 8, nz, span=span)
    quads = np.asarray(cyl.elem_coords)[:, :4, :2]
    vol = (iu.shoelace_areas(quads).astype(np.longdouble) * np.longdouble(span / nz)).sum()
    _, w = quadrature_points(cyl, order)
    K = iu.constant_K(cyl, order)
    err = abs(float(w.astype(np.longdouble).sum() - vol)) / (EPS * float(vol))
    print(f"extruded ring p={order}: |sum w - volume| = {err:.3f} eps volume (bound K = {K})")
    assert err <= K


def test_outputs_may_be_null_and_the_count_is_always_written():
    lib = capi.load()
    mesh = iu.perturbed_box(3, (3, 2, 2))
    ma = capi.MeshArgs(mesh)
    n = C.c_int64(-1)
    assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 2, None, None, C.byref(n)) == 0
    assert n.value == 12 * 4 ** 3
    xyz, w = quadrature_points(mesh, 2)
    only_w, only_x = np.full(n.value, -7.0), np.full((3, n.value), -7.0)
    assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 2, None, only_w.ctypes.data, C.byref(n)) == 0
    assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 2, only_x.ctypes.data, None, C.byref(n)) == 0
    assert np.array_equal(only_w, w) and np.array_equal(only_x, xyz)


def test_refusals():
    lib = capi.load()
    mesh = iu.perturbed_box(2, (3, 2))
    ma = capi.MeshArgs(mesh)
    n = C.c_int64(0)
    bad = capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_quadrature_points(None, 2, None, None, C.byref(n)) == bad
    assert "tpsrhs_quadrature_points" in lib.tpsrhs_last_error().decode()
    assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 2, None, None, None) == bad
    for order in (0, -1, 6):
        assert lib.tpsrhs_quadrature_points(C.byref(ma.c), order, None, None, C.byref(n)) == bad
    for dim in (1, 4):
        ma.c.dim = dim
        assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 2, None, None, C.byref(n)) == bad
    ma.c.dim = 2
    assert lib.tpsrhs_quadrature_points(C.byref(ma.c), 5, None, None, C.byref(n)) == 0 and n.value == 6 * 49
