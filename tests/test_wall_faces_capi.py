"""tpsrhs_wall_faces through the C ABI on the CPU (host only: no device is touched): the counts, coordinates and order of
the wall faces against the selection restated from the mesh arrays (tests/wall_distance_util.py), the reference's default
rule over the boundary conditions, a capacity smaller than the count, scrambled element orientations, the refusals."""
import ctypes as C

import numpy as np
import pytest

import wall_distance_util as wd
from tps_amd import capi, meshgen


@pytest.mark.parametrize("name,count", [("tube", 5), ("cylinder", 24), ("partial", 6)])
def test_counts_coordinates_and_order(name, count):
    make, attrs, _ = wd.CASES[name]
    mesh = make()
    got = capi.wall_faces(mesh, attributes=attrs)
    assert got.shape == (count, 1 << (mesh.dim - 1), mesh.dim)
    assert np.array_equal(got, wd.wall_faces_np(mesh, attrs))  # the same corners, the same (element, local face) order


def test_coordinates_against_the_generator():
    tube = capi.wall_faces(wd.tube(), attributes=[3])  # r = r_out, one face per axial cell, z ascending
    assert np.all(tube[:, :, 0] == 0.0 + (0.05 - 0.0) * 3 / 3)  # the generator's own arithmetic
    assert np.array_equal(tube[:, :, 1], np.array([[0.25 * j / 5, 0.25 * (j + 1) / 5] for j in range(5)]))
    cyl = capi.wall_faces(wd.cylinder(), attributes=[3])
    assert np.abs(np.hypot(cyl[..., 0], cyl[..., 1]) - 0.5).max() <= 2 * wd.EPS
    # local face xi_0 = 0 of the element: ta runs along theta, tb along z
    assert np.all(cyl[:, 0, 2] == cyl[:, 1, 2]) and np.all(cyl[:, 2, 2] > cyl[:, 0, 2])
    part = capi.wall_faces(wd.partial_wall_box(), attributes=[7])
    assert np.all(part[..., 2] == 0.0) and part[..., 0].max() == 0.5


def test_attribute_lists():
    mesh = wd.cylinder()
    assert capi.wall_faces(mesh, attributes=[1, 2, 3]).shape[0] == 48
    assert capi.wall_faces(mesh, attributes=[]).shape == (0, 4, 3)
    assert capi.wall_faces(mesh, attributes=[99]).shape == (0, 4, 3)


def test_default_rule_drops_inviscid_walls_only():
    mesh = wd.cylinder()
    for wall_type in (capi.VISC_ISOTH, capi.VISC_ADIAB, capi.SLIP, capi.VISC_GNRL):
        bcs = [capi.make_bc(1, capi.INLET, capi.SUB_DENS_VEL), capi.make_bc(2, capi.OUTLET, capi.SUB_P),
               capi.make_bc(3, capi.WALL, wall_type)]
        assert np.array_equal(capi.wall_faces(mesh, bcs), capi.wall_faces(mesh, attributes=[3]))
    bcs[2] = capi.make_bc(3, capi.WALL, capi.INV)
    assert capi.wall_faces(mesh, bcs).shape == (0, 4, 3)
    # a wall type value on another category is no wall: inlet type 3 is not VISC_ISOTH
    bcs = [capi.make_bc(1, capi.INLET, 3), capi.make_bc(2, capi.WALL, capi.SLIP), capi.make_bc(3, capi.WALL, capi.INV)]
    assert np.array_equal(capi.wall_faces(mesh, bcs), capi.wall_faces(mesh, attributes=[2]))
    assert capi.wall_faces(mesh, ()).shape == (0, 4, 3)


def _raw(mesh, natt, att, capacity, out, count):
    lib = capi.load()
    ma = capi.MeshArgs(mesh)
    return lib.tpsrhs_wall_faces(C.byref(ma.c) if mesh is not None else None, 0, None, natt,
                                 att.ctypes.data if att is not None else None, capacity,
                                 out.ctypes.data if out is not None else None, C.byref(count) if count is not None else None)


def test_capacity_smaller_than_the_count():
    mesh = wd.cylinder()
    full = capi.wall_faces(mesh, attributes=[3])
    att = np.array([3], dtype=np.int32)
    out = np.full((10, 4, 3), -7.0)
    n = C.c_int64(-1)
    assert _raw(mesh, 1, att, 7, out, n) == 0
    assert n.value == 24
    assert np.array_equal(out[:7], full[:7]) and np.all(out[7:] == -7.0)
    n = C.c_int64(-1)
    assert _raw(mesh, 1, att, 0, None, n) == 0 and n.value == 24


@pytest.mark.parametrize("seed", [1, 2])
def test_scrambled_orientations_give_the_same_faces(seed):
    for name in ("cylinder", "tube", "partial"):
        make, attrs, _ = wd.CASES[name]
        mesh = make()

        def as_sets(faces):
            return {frozenset(tuple(c) for c in f) for f in faces}

        a, b = capi.wall_faces(mesh, attributes=attrs), capi.wall_faces(meshgen.scramble_orientations(mesh, seed), attributes=attrs)
        assert a.shape == b.shape and as_sets(a) == as_sets(b)


def test_refusals():
    lib = capi.load()
    mesh = wd.tube()
    att = np.array([3], dtype=np.int32)
    n = C.c_int64(0)

    def refused(st):
        assert st == capi.ERR_INVALID_ARGUMENT
        assert b"tpsrhs_wall_faces" in lib.tpsrhs_last_error()

    ma = capi.MeshArgs(mesh)
    refused(lib.tpsrhs_wall_faces(None, 0, None, 1, att.ctypes.data, 0, None, C.byref(n)))
    refused(_raw(mesh, 1, att, 0, None, None))
    refused(_raw(mesh, 1, att, 4, None, n))    # capacity without an array
    refused(_raw(mesh, 1, att, -1, None, n))
    refused(_raw(mesh, 1, None, 0, None, n))   # a count of attributes without the list
    refused(lib.tpsrhs_wall_faces(C.byref(ma.c), 2, None, -1, None, 0, None, C.byref(n)))  # the default rule without bcs
    for dim in (1, 4):
        ma = capi.MeshArgs(mesh)
        ma.c.dim = dim
        refused(lib.tpsrhs_wall_faces(C.byref(ma.c), 0, None, 1, att.ctypes.data, 0, None, C.byref(n)))
    bad = meshgen.annulus_quad(3, 5)
    bad.bdr_vertices = bad.bdr_vertices.copy()
    bad.bdr_vertices[2] = [0, 5]  # two vertices that span no element face
    refused(_raw(bad, 1, att, 0, None, n))
