"""tpsrhs_lattice_coordinates / tpsrhs_lattice_fields (k_lattice) on the device against the numpy restatements
(tps_amd.paraview.lattice_points for the coordinates, tests/sampling_util.py for the values), against the arbitrary-point
sampler, and end to end through ParaviewCollection with the reader of tests/paraview_util.py.

Meshes: the 12-hex and the 6-quad box, warped and orientation-scrambled -- neither element count is a multiple of the
elements a block holds (2-D: 16, 7, 4, 2, 1 for p = 1..5; 3-D: 8, 2, 1, 1, 1), so every small-element kernel runs a tail
block.  The bound on a value is sampling_util.bound_from_abs: it covers the full-length sum, and the factorised sum is
shorter."""
import ctypes as C
import functools

import numpy as np
import pytest

import paraview_util as pu
import sampling_util as su
from tps_amd import capi, cases, meshgen
from tps_amd import paraview as pv
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
# (order, basis): both pairs where built -- the Gauss-Lobatto pair exists for orders 1..3
PAIRS = [(1, 0), (3, 0), (5, 0), (1, 1), (3, 1)]
PAIR_IDS = [f"p{p}_{'lobatto' if b else 'legendre'}" for p, b in PAIRS]


def levels_of(p):
    """1, p, 8 and one L != p in between"""
    return sorted({1, p, 8, 5 if p != 5 else 3})


def _walls(mesh):
    return [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]


_OPERATORS = {}


def _setup(dim, order, basis, affine=False):
    """(mesh, operator): one operator per configuration, shared by the tests and closed when the module is done"""
    from tps_amd.rhs_operator import RHSoperator

    key = (dim, order, basis, affine)
    if key not in _OPERATORS:
        mesh = su.affine_box(dim) if affine else su.box(dim, warp=0.2, scramble=5)
        _OPERATORS[key] = (mesh, RHSoperator(mesh, capi.Disc(order, basis, basis, 0, 0), capi.dry_air_physics(capi.NS), _walls(mesh)))
    return _OPERATORS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_operators():
    yield
    for _, op in _OPERATORS.values():
        op.close()
    _OPERATORS.clear()


def _dev(op, a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=op.device)


def _lattice_ref(mesh, levels):
    """(elem (npts,), ref (dim, npts)) of every lattice point"""
    npe = (levels + 1) ** mesh.dim
    return np.repeat(np.arange(mesh.num_elements), npe), np.tile(pv.lattice_reference(mesh.dim, levels), (1, mesh.num_elements))


@functools.lru_cache(maxsize=None)
def _field(dim, order, nrows=7):
    ne = {2: 6, 3: 12}[dim]
    f = np.random.default_rng(1000 * dim + order).standard_normal((nrows, ne * (order + 1) ** dim))  # of order one
    f.setflags(write=False)
    return f


def _corner_locals(dim, n_per_dir):
    return [sum((n_per_dir - 1) * c[d] * n_per_dir ** d for d in range(dim)) for c in su.CORNERS[dim]]


# ---- coordinates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 5, 8])
@pytest.mark.parametrize("dim", [2, 3])
def test_coordinates(dim, levels):
    mesh, op = _setup(dim, 1, 0)
    assert op.latticeSize(levels) == ((levels + 1) ** dim, mesh.num_elements * (levels + 1) ** dim)
    got = op.latticeCoordinates(levels).cpu().numpy()
    want = pv.lattice_points(mesh, levels)
    assert got.shape == want.shape
    # |x| is the length of the point: the warp carries single coordinates through zero (|x_d| down to 1e-18 next to vertex
    # coordinates of order one), where a bound relative to that one coordinate is one no evaluation of the map can meet
    norm = np.linalg.norm(want, axis=0)[None, :]
    ratio = np.abs(got - want) / np.maximum(EPS * norm, np.finfo(float).tiny)
    print(f"dim {dim} L {levels}: max |device - numpy| / (eps |x|) = {ratio.max():.2f}")
    assert (np.abs(got - want) <= 4 * EPS * norm).all()
    per = got.reshape(dim, mesh.num_elements, -1)
    for v, loc in enumerate(_corner_locals(dim, levels + 1)):
        assert np.array_equal(per[:, :, loc].T, np.asarray(mesh.elem_coords)[:, v, :])  # bit for bit


# ---- values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_values_match_the_restatement(dim, pair):
    import torch

    order, basis = pair
    mesh, op = _setup(dim, order, basis)
    field = _field(dim, order)
    dfield = _dev(op, field)
    keep = dfield.clone()
    for levels in levels_of(order):
        elem, ref = _lattice_ref(mesh, levels)
        val, sum_abs = su.evaluate(field, elem, ref, order, basis)
        b = su.bound_from_abs(sum_abs, order, dim)
        for nrows in (1, 7):
            got64 = op.latticeFields(dfield[:nrows], levels)
            got32 = op.latticeFields(dfield[:nrows], levels, dtype=torch.float32)
            g = got64.cpu().numpy()
            assert g.shape == (nrows, elem.size) and np.isfinite(g).all()
            ratio = np.abs(g - val[:nrows]) / np.maximum(b[:nrows], np.finfo(float).tiny)
            print(f"dim {dim} p {order} basis {basis} L {levels} nrows {nrows}: max |device - restatement| / bound = {ratio.max():.3f}")
            assert (np.abs(g - val[:nrows]) <= b[:nrows]).all()
            assert got32.dtype == torch.float32 and torch.equal(got32, got64.to(torch.float32))  # bit for bit
        one = op.latticeFields(dfield[3].clone(), levels)  # [NDofs] is one row
        assert one.shape == (1, elem.size) and torch.equal(one[0], op.latticeFields(dfield[:4], levels)[3])
    assert torch.equal(dfield, keep)  # the field is unchanged


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_polynomials_are_reproduced(dim, pair):
    order, basis = pair
    mesh, op = _setup(dim, order, basis, affine=True)
    f = su.random_polynomial(dim, order, seed=10 * order + dim)
    u = f(node_coordinates(mesh, order, basis))
    for levels in levels_of(order):
        elem, ref = _lattice_ref(mesh, levels)
        _, sum_abs = su.evaluate(u, elem, ref, order, basis)
        b = su.bound_from_abs(sum_abs, order, dim)[0]
        got = op.latticeFields(_dev(op, u), levels).cpu().numpy()[0]
        err = np.abs(got - f(pv.lattice_points(mesh, levels)))
        print(f"dim {dim} p {order} basis {basis} L {levels}: max error / bound = {(err / np.maximum(b, np.finfo(float).tiny)).max():.3f}")
        assert (err <= b).all()


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("dim", [2, 3])
def test_lobatto_nodes_on_the_lattice_are_copied_bit_for_bit(dim, order):
    mesh, op = _setup(dim, order, 1)
    field = _field(dim, order)
    n1 = order + 1
    # L = 1: the lattice is the corners, and the corner nodes of the Gauss-Lobatto basis sit there
    got = op.latticeFields(_dev(op, field), 1).cpu().numpy().reshape(7, mesh.num_elements, 2 ** dim)
    nodal = field.reshape(7, mesh.num_elements, n1 ** dim)
    lex_corner_nodes = [sum((order if (c >> d) & 1 else 0) * n1 ** d for d in range(dim)) for c in range(2 ** dim)]
    assert np.array_equal(got, nodal[:, :, lex_corner_nodes])
    if order <= 2:  # L = p: the nodes 0, (1/2,) 1 are the lattice and the rows of B are exact unit vectors
        assert np.array_equal(op.latticeFields(_dev(op, field), order).cpu().numpy(), field)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_shared_face_carries_each_elements_own_value(dim):
    order, levels = 3, 4
    mesh, op = _setup(dim, order, 0)
    npe = (order + 1) ** dim
    field = np.repeat(10.0 * (1 + np.arange(mesh.num_elements)), npe)[None, :]  # jumps by 10 or more between elements
    got = op.latticeFields(_dev(op, field), levels).cpu().numpy()[0]
    elem, ref = _lattice_ref(mesh, levels)
    _, sum_abs = su.evaluate(field, elem, ref, order, 0)
    assert (np.abs(got - 10.0 * (1 + elem)) <= su.bound_from_abs(sum_abs, order, dim)[0]).all()
    # ... in particular at the points two elements share: both copies exist, each with its own element's value
    X = pv.lattice_points(mesh, levels)
    close = np.abs(X[:, :, None] - X[:, None, :]).max(axis=0) < 1e-12
    np.fill_diagonal(close, False)
    # a point with exactly one coincident partner lies in the interior of a face between two elements
    on_faces = [(i, int(np.flatnonzero(close[i])[0])) for i in np.flatnonzero(close.sum(axis=1) == 1)]
    assert len(on_faces) >= 2 * (levels - 1) ** (dim - 1)
    for i, j in on_faces:
        assert elem[i] != elem[j] and abs(got[i] - got[j]) >= 10.0 - 1e-9
        assert round(got[i] / 10.0) - 1 == elem[i] and round(got[j] / 10.0) - 1 == elem[j]


# ---- guards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["double", "float"])
@pytest.mark.parametrize("case", [(2, 1, 8), (2, 4, 3), (3, 1, 8), (3, 2, 1), (3, 3, 3), (3, 5, 5)], ids=str)
def test_nothing_is_written_outside_the_output(case, f32):
    import torch

    dim, order, levels = case
    mesh, op = _setup(dim, order, 0)
    nrows, margin, sentinel = 3, 4096, -777.25
    _, npts = op.latticeSize(levels)
    field = _dev(op, np.random.default_rng(5).standard_normal((nrows, op.NDofs)))
    dt = torch.float32 if f32 else torch.float64
    buf = torch.full((margin + nrows * npts + margin,), sentinel, dtype=dt, device=op.device)
    out_ptr = buf.data_ptr() + margin * buf.element_size()
    st = capi.load().tpsrhs_lattice_fields(op._h, levels, nrows, C.c_void_p(field.data_ptr()), C.c_void_p(out_ptr), int(f32))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.all(buf[:margin] == sentinel) and torch.all(buf[margin + nrows * npts:] == sentinel)
    inner = buf[margin:margin + nrows * npts].view(nrows, npts)
    assert torch.equal(inner, op.latticeFields(field, levels, dtype=dt))
    assert not torch.any(inner == sentinel)


# ---- against the arbitrary-point sampler ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(1, 0), (3, 0), (5, 0), (3, 1)], ids=str)
@pytest.mark.parametrize("dim", [2, 3])
def test_interior_points_agree_with_the_sampler(dim, pair):
    """|lattice - sampler| <= the sum of the two evaluation bounds at the points strictly inside their element.

    The sampler inverts the vertex map at the coordinates it is given, so what it evaluates is the field at the coordinates it
    LOCATED; an error of the physical coordinates reaches them magnified by 1 / (element size), and neither evaluation bound
    counts it.  tpsrhs_lattice_coordinates therefore rounds once (double-double inside): measured on an MI355X the located
    coordinates are within 8.3e-16 of a / L and the worst case, p = 1 at L = 5, is at 0.734 (2-D) and 0.454 (3-D) of the sum,
    every other case below 0.07.  (With coordinates from a plain FMA evaluation, 1 - 2 ulp of |x| off, the same two cases were
    at 0.978 and 1.157.)  The parts are printed and the two evaluations asserted, each against its own restatement."""
    order, basis = pair
    mesh, op = _setup(dim, order, basis)
    field = _field(dim, order)
    dfield = _dev(op, field)
    for levels in (2, 5):
        elem, ref = _lattice_ref(mesh, levels)
        interior = np.all((ref > 0.0) & (ref < 1.0), axis=0)  # 0 < a, b, c < L
        assert interior.sum() == mesh.num_elements * (levels - 1) ** dim
        s = op.createSampler(op.latticeCoordinates(levels))
        sampled = s.sample(dfield).cpu().numpy()
        e_lib, ref_s, nfound = s.info()
        s.close()
        assert nfound >= interior.sum() and np.array_equal(e_lib[interior], elem[interior])
        got = op.latticeFields(dfield, levels).cpu().numpy()
        _, sum_abs = su.evaluate(field, elem, ref, order, basis)
        b = 2.0 * su.bound_from_abs(sum_abs, order, dim)  # the sum of the two bounds
        diff = np.abs(got - sampled)[:, interior]
        print(f"dim {dim} p {order} basis {basis} L {levels}: max |lattice - sampler| / bound = {(diff / b[:, interior]).max():.3f}")
        # the parts: each route against the restatement at ITS reference coordinates, and what the located coordinates add
        val_l, _ = su.evaluate(field, elem, ref, order, basis)
        val_s, abs_s = su.evaluate(field, elem[interior], ref_s[:, interior], order, basis)
        half = 0.5 * b[:, interior]
        assert (np.abs(got - val_l)[:, interior] <= half).all()
        assert (np.abs(sampled[:, interior] - val_s) <= su.bound_from_abs(abs_s, order, dim)).all()
        print(f"    lattice / its bound {(np.abs(got - val_l)[:, interior] / half).max():.3f}, sampler / its bound "
              f"{(np.abs(sampled[:, interior] - val_s) / half).max():.3f}, restatement at the located coordinates against a / L "
              f"/ one bound {(np.abs(val_s - val_l[:, interior]) / half).max():.3f}, max |located - a / L| = "
              f"{np.abs(ref_s - ref)[:, interior].max():.2e}")
        assert (diff <= b[:, interior]).all()


# ---- end to end: the reference's fields through the collection ------------------------------------------------------------
def _planar_ternary():
    mesh = meshgen.box_quad(3, 3, lengths=(1.0, 0.8), warp=0.05)
    return cases.Case("planar_ternary_p2", mesh, capi.Disc(2, 0, 0, 0, 0), capi.argon_ternary_physics(), [])


@pytest.mark.parametrize("kind", ["planar", "axisymmetric"])
def test_collection_end_to_end(tmp_path, kind):
    import torch

    from tps_amd.rhs_operator import RHSoperator

    c = _planar_ternary() if kind == "planar" else cases.argon_axisym(2, 3, 2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = _dev(op, c.state(seed=7)).reshape(-1)
    fields = pv.reference_fields(op, x)
    coll = pv.ParaviewCollection(str(tmp_path), "vis", op)
    assert coll.levels == 2 and coll.dtype == np.float32
    piece = coll.save(0, 0.0, fields)
    got = pu.read_vtu(piece)
    _, npts = op.latticeSize(2)
    assert got["npoints"] == npts and got["ncells"] == c.mesh.num_elements * 4 and np.all(got["types"] == 9)
    assert np.array_equal(got["points"][:, :2], op.latticeCoordinates(2).cpu().numpy().T.astype(np.float32))
    assert np.all(got["points"][:, 2] == 0.0)
    up = op.getPrimitives()
    assert np.array_equal(got["point_data"]["dens"], op.latticeFields(up[0].contiguous(), 2, dtype=torch.float32).cpu().numpy()[0])
    vel = got["point_data"]["vel"]
    assert vel.shape == (npts, 3) and np.all(vel[:, 2] == 0.0)  # two flow components, padded
    assert np.array_equal(vel[:, :2], op.latticeFields(up[1:3].contiguous(), 2, dtype=torch.float32).cpu().numpy().T)
    assert ("vtheta" in got["point_data"]) == (kind == "axisymmetric")
    if kind == "axisymmetric":
        assert np.array_equal(got["point_data"]["vtheta"], op.latticeFields(up[3].contiguous(), 2, dtype=torch.float32).cpu().numpy()[0])
        assert "Te" in got["point_data"]  # argon_axisym is a two-temperature plasma
    for name in ("temp", "press"):
        assert got["point_data"][name].shape == (npts,) and np.all(got["point_data"][name] > 0.0)
    lay = op.visualizationLayout()
    for name, _, rows in capi.visualization_names(lay):
        a = got["point_data"][name]
        assert a.shape[0] == npts and np.isfinite(a).all(), name
        assert a.ndim == (1 if rows == 1 else 2)
    pieces, arrays, _ = pu.read_pvtu(str(tmp_path / "vis" / "Cycle000000" / "data.pvtu"))
    assert pieces == ["proc000000.vtu"] and [a[0] for a in arrays] == got["order"]
    assert pu.read_pvd(str(tmp_path / "vis" / "vis.pvd")) == [(0.0, "Cycle000000/data.pvtu")]
    op.close()


# ---- the tool: a restart file as a collection ------------------------------------------------------------------------------
def test_restart_to_paraview_tool(tmp_path):
    import os
    import subprocess
    import sys

    import torch

    from tps_amd import mesh_io, restart

    mesh = su.box(2, warp=0.1)
    order = 2
    c = cases.Case("tool_box", mesh, capi.Disc(order, 0, 0, 0, 0), capi.dry_air_physics(capi.NS), _walls(mesh))
    U = c.state(seed=3)
    mesh_path, rst = str(tmp_path / "box.mesh"), str(tmp_path / "restart.h5")
    mesh_io.write_mfem_mesh(mesh_path, mesh)
    names = restart.variable_names(2, [], False)
    restart.write(rst, names, U, iteration=120, time=0.75, dt=1e-3, order=order, dimension=2, dofs_global=U.shape[1])
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "restart_to_paraview.py")
    r = subprocess.run([sys.executable, tool, mesh_path, rst, "--order", str(order), "-o", str(tmp_path / "out"), "--name", "box"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert pu.read_pvd(str(tmp_path / "out" / "box" / "box.pvd")) == [(0.75, "Cycle000120/data.pvtu")]
    got = pu.read_vtu(str(tmp_path / "out" / "box" / "Cycle000120" / "proc000000.vtu"))
    assert got["order"] == ["dens", "vel", "temp", "press"]  # dry air: no Te, no plasma fields, no sigma
    # dens is the first conserved row itself: the tool's file against this process's own evaluation
    mesh2, op = _setup(2, order, 0)
    assert mesh2.num_elements == mesh.num_elements
    want = op.latticeFields(_dev(op, U[0]), order, dtype=torch.float32).cpu().numpy()[0]
    assert got["npoints"] == want.size and np.array_equal(got["point_data"]["dens"], want)
    assert got["point_data"]["vel"].shape == (want.size, 3) and np.all(got["point_data"]["press"] > 0.0)
