"""tpsrhs_wall_distance on the device against the numpy restatement (tests/wall_distance_util.py) and the closed forms.

The bound: |d_device - d_numpy| <= 256 eps L on every node, L the diagonal of the nodes' bounding box.  Rounding-level
perturbations of nodes and corners move the restatement by at most 8 eps L; the factor 256 is the margin for FMA
contraction and another summation order.  The closed forms hold to 16 eps L in the restatement
(tests/test_wall_distance_restatement.py), so the device is held to (256 + 16) eps L against them."""
import ctypes as C

import numpy as np
import pytest

import wall_distance_util as wd
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
BOUND = 256 * wd.EPS


def _operator(mesh, order, basis=0, wall_type=capi.VISC_ISOTH):
    """dry air, Navier-Stokes, a wall on every boundary attribute of the mesh"""
    from tps_amd.rhs_operator import RHSoperator

    bcs = [capi.make_bc(int(a), capi.WALL, wall_type, [300.0]) for a in np.unique(mesh.bdr_attributes)]
    return RHSoperator(mesh, capi.Disc(order, basis, basis, 0, 0), capi.dry_air_physics(capi.NS), bcs)


def _device(mesh, order, basis, **kw):
    op = _operator(mesh, order, basis)
    try:
        d = op.wallDistance(**kw)
        assert d.dtype.is_floating_point and d.is_cuda and d.numel() == op.NDofs
        return d.cpu().numpy()
    finally:
        op.close()


def _compare(name, order, basis):
    mesh, faces, X, L, ref = wd.restated(name, order, basis)
    got = _device(mesh, order, basis, attributes=list(wd.CASES[name][1]))
    err = np.abs(got - ref).max() / (wd.EPS * L)
    print(f"{name} p={order} basis={basis}: {X.shape[1]} nodes x {faces.shape[0]} faces, device - restatement = {err:.2f} eps L")
    assert np.abs(got - ref).max() <= BOUND * L
    exact = wd.CASES[name][2]
    if exact is not None:
        assert np.abs(got - exact(X)).max() <= (256 + 16) * wd.EPS * L
    return got


CLOSED = [("tube", p, b) for p in (1, 2, 3) for b in (0, 1)] + \
         [(n, p, b) for n in ("cylinder", "partial") for p in (1, 2, 3) for b in (0, 1)] + \
         [("cylinder", 5, 0), ("partial", 5, 0)]  # 216 nodes per element: NDofs is no multiple of the block of 256


@pytest.mark.parametrize("name,order,basis", CLOSED)
def test_closed_forms(name, order, basis):
    _compare(name, order, basis)


@pytest.mark.parametrize("name,nfaces", [("tiles143", 143), ("tiles285", 285)])
def test_more_faces_than_one_tile(name, nfaces):
    """the faces pass through LDS 128 at a time: one full tile and 15, two full tiles and 29"""
    assert wd.restated(name, 1, 0)[1].shape[0] == nfaces
    _compare(name, 1, 0)


@pytest.mark.parametrize("seed", [3])
def test_scrambled_orientations(seed):
    mesh = meshgen.scramble_orientations(wd.cylinder(), seed)
    X = node_coordinates(mesh, 2, 0)
    L = wd.bbox_diagonal(X)
    got = _device(mesh, 2, 0, attributes=[3])
    ref = wd.wall_distance_np(X, wd.wall_faces_np(mesh, (3,)))
    print("scrambled: device - restatement =", np.abs(got - ref).max() / (wd.EPS * L), "eps L")
    assert np.abs(got - ref).max() <= BOUND * L
    assert np.abs(got - wd.chords_exact(X)).max() <= (256 + 16) * wd.EPS * L
    # the same set of nodes as the plain mesh, element by element: the same set of distances
    plain = wd.restated("cylinder", 2, 0)[4].reshape(mesh.num_elements, -1)
    assert np.abs(np.sort(got.reshape(mesh.num_elements, -1), axis=1) - np.sort(plain, axis=1)).max() <= BOUND * L


def test_non_affine_faces():
    """warped bottom: a pair whose stop decision falls within rounding of 1e-10 may take one more iteration on one side,
    so at most 0.1 % of the nodes may exceed 256 eps L, and those lie within 1e-9 L"""
    mesh, faces, X, L, ref = wd.restated("warped", 2, 0)
    got = _device(mesh, 2, 0, attributes=[5])
    diff = np.abs(got - ref)
    over = diff > BOUND * L
    print(f"warped: max {diff.max() / (wd.EPS * L):.2f} eps L, {over.sum()} of {diff.size} nodes beyond 256 eps L")
    assert over.sum() <= 0.001 * diff.size
    assert diff.max() <= 1e-9 * L


def test_attribute_selection_and_the_default_rule():
    mesh, faces, X, L, ref3 = wd.restated("cylinder", 2, 0)
    ref123 = wd.wall_distance_np(X, wd.wall_faces_np(mesh, (1, 2, 3)))
    op = _operator(mesh, 2, 0)
    d3 = op.wallDistance(attributes=[3]).cpu().numpy()
    d123 = op.wallDistance(attributes=[1, 2, 3]).cpu().numpy()
    default = op.wallDistance().cpu().numpy()  # every patch is a viscous wall in this operator
    op.close()
    assert np.abs(d3 - ref3).max() <= BOUND * L and np.abs(d123 - ref123).max() <= BOUND * L
    assert np.all(d123 <= d3) and (d123 < d3).any()  # the outer ring is nearer to the outer nodes
    assert np.array_equal(default, d123)
    op = _operator(mesh, 2, 0, wall_type=capi.INV)
    none = op.wallDistance().cpu().numpy()
    op.close()
    assert np.all(none == 1e30)


@pytest.mark.parametrize("poison", ["0", "1"])
def test_zero_faces(monkeypatch, poison):
    """every entry is written, also without a face: under TPSRHS_POISON=1 the library's own allocations start as NaNs"""
    import torch

    monkeypatch.setenv("TPSRHS_POISON", poison)
    op = _operator(wd.tube(), 2, 0)
    d = op.wallDistance(faces=np.zeros((0, 2, 2)))
    assert torch.all(d == 1e30)
    out = torch.full((op.NDofs,), float("nan"), dtype=torch.float64, device=op.device)
    assert op._lib.tpsrhs_wall_distance(op._h, 0, None, C.c_void_p(out.data_ptr())) == 0
    assert torch.all(out == 1e30)
    assert torch.all(op.wallDistance(attributes=[]) == 1e30)
    op.close()


def test_partition_union_of_the_ranks_faces():
    """one process, no second rank: each slab's nodes against the wall faces of BOTH slabs"""
    slabs = [meshgen.ogrid_cylinder_slab(3, 8, 3, rank, 2) for rank in (0, 1)]
    own = [capi.wall_faces(m, attributes=[3]) for m in slabs]
    assert [f.shape[0] for f in own] == [24, 24]
    union = np.concatenate(own)
    for rank, mesh in enumerate(slabs):
        from tps_amd.rhs_operator import RHSoperator

        c = cases.cyl3d(3, 8, 3, 2)
        halo = type("NoExchange", (), {"callback": staticmethod(lambda *a: 0)})()  # wallDistance never exchanges
        op = RHSoperator(mesh, c.disc, c.physics, c.bcs, halo=halo)
        got = op.wallDistance(faces=union).cpu().numpy()
        alone = op.wallDistance(faces=own[rank]).cpu().numpy()
        op.close()
        X = node_coordinates(mesh, 2, 0)
        L = wd.bbox_diagonal(X)
        assert np.abs(got - wd.wall_distance_np(X, union)).max() <= BOUND * L
        assert np.abs(got - wd.chords_exact(X)).max() <= (256 + 16) * wd.EPS * L
        assert np.all(got <= alone)


def test_end_to_end_mixing_length():
    """the setting of test/inputs/pipe.axisym.mix.ini (tests/test_mixing_length.py): Mult with the computed distance
    against Mult with the analytic r_out - r"""
    import torch
    from parity_util import RHS_RTOL, rel_maxnorm
    from tps_amd.rhs_operator import RHSoperator

    c = cases.dry_air_axisym(5, 7, 3, capi.NS, capi.VISC_ISOTH, r_in=0.0)
    c.physics.dry_air.visc_mult = 50.0
    U = c.state(seed=5, amp=0.05)
    X = node_coordinates(c.mesh, 3)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    ys = []
    computed = op.wallDistance()  # the default rule: patch 3 is the isothermal wall, patch 4 (the axis) is inviscid
    analytic = torch.tensor(np.ascontiguousarray(0.05 - X[0]), dtype=torch.float64, device=op.device)
    assert (computed - analytic).abs().max().item() <= BOUND * wd.bbox_diagonal(X)
    for dist in (computed, analytic, None):
        y = torch.empty_like(x)
        op.setMixingLength(dist, max_mixing_length=0.004, pr_ratio=0.9, bulk_multiplier=0.5)
        op.Mult(x, y)
        ys.append(y.cpu().numpy().reshape(U.shape))
    op.close()
    assert rel_maxnorm(ys[0], ys[1]).max() < RHS_RTOL
    assert rel_maxnorm(ys[1], ys[2]).max() > 1e-4  # the model does change the residual


def test_error_paths():
    import torch

    op = _operator(wd.tube(), 1, 0)
    lib = op._lib
    out = torch.zeros(op.NDofs, dtype=torch.float64, device=op.device)
    faces = np.ascontiguousarray(capi.wall_faces(wd.tube(), attributes=[3]))
    o, f = C.c_void_p(out.data_ptr()), faces.ctypes.data

    def refused(st):
        assert st == capi.ERR_INVALID_ARGUMENT
        assert b"tpsrhs_wall_distance" in lib.tpsrhs_last_error()

    refused(lib.tpsrhs_wall_distance(None, 5, f, o))
    refused(lib.tpsrhs_wall_distance(op._h, -1, f, o))
    refused(lib.tpsrhs_wall_distance(op._h, 5, None, o))
    refused(lib.tpsrhs_wall_distance(op._h, 5, f, None))
    for bad in (np.nan, np.inf, -np.inf):
        g = faces.copy()
        g[4, 1, 0] = bad
        refused(lib.tpsrhs_wall_distance(op._h, 5, g.ctypes.data, o))
    assert torch.all(out == 0.0)  # refused before any device work
    assert lib.tpsrhs_wall_distance(op._h, 5, f, o) == 0
    with pytest.raises(ValueError):
        op.wallDistance(faces=np.zeros((3, 4, 3)))
    op.close()


@pytest.mark.parametrize("name,order,basis", [("tube", 3, 1), ("cylinder", 2, 0), ("partial", 5, 0), ("tiles143", 1, 0),
                                               ("tiles285", 1, 0), ("warped", 2, 0)])
def test_cull_is_bit_equal(monkeypatch, name, order, basis):
    """TPSRHS_WALLDIST_CULL: a face that is skipped cannot win the minimum, so the switch changes no bit"""
    mesh = wd.restated(name, order, basis)[0]
    op = _operator(mesh, order, basis)
    got = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("TPSRHS_WALLDIST_CULL", cull)
        got[cull] = op.wallDistance(attributes=list(wd.CASES[name][1])).cpu().numpy()
    op.close()
    assert np.array_equal(got["0"], got["1"])
