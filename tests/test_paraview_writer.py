"""The host half of the ParaView output (tps_amd/paraview.py) without a device: the lattice points restated in numpy, the
sub-cell connectivity, the .vtu writer in both encodings read back bit for bit by a reader of the test's own
(tests/paraview_util.py), and the collection's directory layout with a numpy stand-in for the operator."""
import os
import types

import numpy as np
import pytest

import paraview_util as pu
import sampling_util as su
from tps_amd import paraview as pv

EPS = np.finfo(np.float64).eps


def corner_locals(dim, levels):
    """local lattice index of MFEM vertex v"""
    n = levels + 1
    return [sum(levels * c[d] * n ** d for d in range(dim)) for c in su.CORNERS[dim]]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("levels", [1, 3, 8])
def test_lattice_points_corners_are_the_vertices_bit_for_bit(dim, levels):
    mesh = su.box(dim, warp=0.2, scramble=5)
    X = pv.lattice_points(mesh, levels).reshape(dim, mesh.num_elements, -1)
    assert X.shape[2] == (levels + 1) ** dim
    for v, loc in enumerate(corner_locals(dim, levels)):
        assert np.array_equal(X[:, :, loc].T, np.asarray(mesh.elem_coords)[:, v, :])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("levels", [2, 5])
def test_lattice_points_agree_with_the_vertex_map(dim, levels):
    mesh = su.box(dim, warp=0.2, scramble=5)
    n, npe = levels + 1, (levels + 1) ** dim
    X = pv.lattice_points(mesh, levels)
    loc = np.arange(npe)
    xi = np.stack([((loc // n ** d) % n) / levels for d in range(dim)])  # local = a + b n + c n^2
    elem = np.repeat(np.arange(mesh.num_elements), npe)
    ref = su.vertex_map(np.asarray(mesh.elem_coords)[elem], np.tile(xi, (1, mesh.num_elements)))
    # two orders of summing 2^dim products of dim + 1 factors each: a few roundings of the largest term
    scale = np.abs(np.asarray(mesh.elem_coords)).max()
    assert np.abs(X - ref).max() <= 4 * (2 ** dim + dim) * EPS * scale
    interior = np.all((xi > 0) & (xi < 1), axis=0)
    assert interior.any() and np.abs(X - ref)[:, np.tile(interior, mesh.num_elements)].max() <= 4 * (2 ** dim + dim) * EPS * scale


def cell_measures(dim, X, conn):
    """signed area (shoelace) / volume (2 x 2 x 2 Gauss rule on det J of the trilinear map, which is exact) of the sub-cells"""
    nv = 2 ** dim
    P = X.T[conn.reshape(-1, nv)]  # (ncells, nv, dim), VTK order = MFEM order
    if dim == 2:
        x, y = P[:, :, 0], P[:, :, 1]
        return 0.5 * sum(x[:, i] * y[:, (i + 1) % 4] - x[:, (i + 1) % 4] * y[:, i] for i in range(4))
    g = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)
    vol = np.zeros(P.shape[0])
    for a in g:
        for b in g:
            for c in g:
                xi = (a, b, c)
                J = np.zeros((P.shape[0], 3, 3))
                for v, cr in enumerate(su.CORNERS[3]):
                    for d in range(3):
                        dw = 1.0 if cr[d] else -1.0
                        for k in range(3):
                            if k != d:
                                dw *= xi[k] if cr[k] else 1.0 - xi[k]
                        J[:, :, d] += P[:, v, :] * dw
                vol += np.linalg.det(J) / 8.0
    return vol


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("levels", [1, 2, 5])
def test_lattice_cells(dim, levels):
    mesh = su.box(dim, warp=0.2, scramble=5)
    ne, npe, nv = mesh.num_elements, (levels + 1) ** dim, 2 ** dim
    conn, offsets, types = pv.lattice_cells(dim, ne, levels)
    ncells = ne * levels ** dim
    assert conn.shape == (ncells * nv,) and offsets.shape == (ncells,) and types.shape == (ncells,)
    assert np.array_equal(offsets, nv * (1 + np.arange(ncells))) and np.all(types == (12 if dim == 3 else 9))
    assert conn.min() >= 0 and conn.max() < ne * npe
    owner = np.repeat(np.arange(ne), levels ** dim)
    assert np.array_equal(conn.reshape(ncells, nv) // npe, np.repeat(owner[:, None], nv, axis=1))  # inside the element's block
    for cell in conn.reshape(ncells, nv):
        assert len(set(cell.tolist())) == nv
    assert cell_measures(dim, pv.lattice_points(mesh, levels), conn).min() > 0.0
    # affine elements: the sub-cells are exact parallelepipeds and tile the mesh
    amesh = su.affine_box(dim)
    total = cell_measures(dim, pv.lattice_points(amesh, levels), pv.lattice_cells(dim, amesh.num_elements, levels)[0]).sum()
    exact = float(np.prod((1.5, 1.0, 0.7)[:dim]))
    assert abs(total - exact) <= 1e-13 * exact


def point_data(dim, npts, dtype, seed=3):
    rng = np.random.default_rng(seed)
    d = {"scalar": rng.standard_normal(npts).astype(dtype), "vec2": rng.standard_normal((2, npts)).astype(dtype),
         "vec3": (rng.standard_normal((3, npts)) * 1e-7).astype(dtype)}
    d["scalar"][:3] = [np.pi * 1e30, -1.0 / 3.0, np.finfo(dtype).tiny]  # values that need every digit
    return d


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("encoding", ["ascii", "appended"])
def test_write_vtu_round_trip(tmp_path, dim, dtype, encoding):
    mesh = su.box(dim, warp=0.2, scramble=5)
    levels = 2
    X = pv.lattice_points(mesh, levels).astype(dtype)
    cells = pv.lattice_cells(dim, mesh.num_elements, levels)
    data = point_data(dim, X.shape[1], dtype)
    path = str(tmp_path / "piece.vtu")
    pv.write_vtu(path, X, cells, data, encoding)
    got = pu.read_vtu(path)
    vtype = "Float64" if dtype == np.float64 else "Float32"
    assert got["npoints"] == X.shape[1] and got["ncells"] == cells[2].size
    assert got["points"].dtype == np.dtype(dtype) and got["points"].shape == (X.shape[1], 3)
    assert np.array_equal(got["points"][:, :dim], X.T)
    if dim == 2:
        assert np.all(got["points"][:, 2] == 0.0)
    assert np.array_equal(got["connectivity"], cells[0]) and got["vtk_types"]["connectivity"] == "Int64"
    assert np.array_equal(got["offsets"], cells[1]) and got["vtk_types"]["offsets"] == "Int64"
    assert np.array_equal(got["types"], cells[2]) and got["vtk_types"]["types"] == "UInt8"
    assert got["order"] == ["scalar", "vec2", "vec3"]
    for name in got["order"]:
        assert got["vtk_types"][name] == vtype and got["point_data"][name].dtype == np.dtype(dtype)
    assert np.array_equal(got["point_data"]["scalar"], data["scalar"])  # 17 / 9 digits round-trip; raw bytes are the bytes
    assert got["point_data"]["vec2"].shape == (X.shape[1], 3)
    assert np.array_equal(got["point_data"]["vec2"][:, :2], data["vec2"].T) and np.all(got["point_data"]["vec2"][:, 2] == 0.0)
    assert np.array_equal(got["point_data"]["vec3"], data["vec3"].T)
    if encoding == "appended":
        item = np.dtype(dtype).itemsize
        npts, ncells, nv = X.shape[1], cells[2].size, 2 ** dim
        sizes = [3 * npts * item, 8 * ncells * nv, 8 * ncells, ncells, npts * item, 3 * npts * item, 3 * npts * item]
        assert [n for _, n in got["appended"]] == sizes
        assert [o for o, _ in got["appended"]] == [int(v) for v in np.cumsum([0] + [8 + s for s in sizes[:-1]])]
    else:
        assert got["appended"] == [] and pu.MARK not in open(path, "rb").read()


def test_write_vtu_refuses_what_it_cannot_write(tmp_path):
    mesh = su.box(2)
    X = pv.lattice_points(mesh, 1)
    cells = pv.lattice_cells(2, mesh.num_elements, 1)
    with pytest.raises(ValueError):
        pv.write_vtu(str(tmp_path / "a.vtu"), X, cells, {"f": np.zeros(X.shape[1] + 1)}, "ascii")
    with pytest.raises(ValueError):
        pv.write_vtu(str(tmp_path / "a.vtu"), X, cells, {}, "base64")


class StandInOperator:
    """what ParaviewCollection asks of an operator, answered in numpy (tests/sampling_util.py) with torch CPU tensors"""

    def __init__(self, mesh, order, basis_type=0):
        self.mesh, self.order, self.basis = mesh, order, basis_type
        self._disc = types.SimpleNamespace(order=order)
        self.NDofs = mesh.num_elements * (order + 1) ** mesh.dim
        self.launches = 0

    def latticeCoordinates(self, levels):
        import torch

        return torch.from_numpy(pv.lattice_points(self.mesh, levels))

    def latticeFields(self, field, levels, dtype=None):
        import torch

        self.launches += 1
        npe = (levels + 1) ** self.mesh.dim
        elem = np.repeat(np.arange(self.mesh.num_elements), npe)
        ref = np.tile(pv.lattice_reference(self.mesh.dim, levels), (1, self.mesh.num_elements))
        vals, _ = su.evaluate(field.numpy().reshape(-1, self.NDofs), elem, ref, self.order, self.basis)
        return torch.from_numpy(vals).to(dtype or torch.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_collection_layout(tmp_path, dtype):
    import torch

    mesh = su.box(2, warp=0.2, scramble=5)
    op = StandInOperator(mesh, order=2)
    coll = pv.ParaviewCollection(str(tmp_path), "run", op, dtype=dtype, rank=0, nranks=3)
    assert coll.levels == 2  # SetLevelsOfDetail(order)
    rng = np.random.default_rng(1)
    for cycle, time in ((0, 0.0), (40, 1.25e-3)):
        fields = {"dens": torch.from_numpy(rng.standard_normal(op.NDofs)), "vel": torch.from_numpy(rng.standard_normal((2, op.NDofs))),
                  "temp": torch.from_numpy(rng.standard_normal(op.NDofs))}
        before = op.launches
        piece = coll.save(cycle, time, fields)
        assert op.launches == before + 1  # one evaluation over the stacked rows
        assert piece == str(tmp_path / "run" / ("Cycle%06d" % cycle) / "proc000000.vtu") and os.path.exists(piece)
    assert sorted(d for d in os.listdir(tmp_path / "run") if d.startswith("Cycle")) == ["Cycle000000", "Cycle000040"]
    assert pu.read_pvd(str(tmp_path / "run" / "run.pvd")) == [(0.0, "Cycle000000/data.pvtu"), (1.25e-3, "Cycle000040/data.pvtu")]
    got = pu.read_vtu(piece)
    vtype = "Float32" if dtype == np.float32 else "Float64"
    pieces, arrays, ptype = pu.read_pvtu(str(tmp_path / "run" / "Cycle000040" / "data.pvtu"))
    assert pieces == ["proc%06d.vtu" % r for r in range(3)] and ptype == vtype == got["vtk_types"]["Points"]
    assert arrays == [("dens", vtype, 1), ("vel", vtype, 3), ("temp", vtype, 1)]
    assert [(n, got["vtk_types"][n], 1 if got["point_data"][n].ndim == 1 else got["point_data"][n].shape[1]) for n in got["order"]] == arrays
    # the piece holds the collection's lattice and the last save's values in the collection's precision
    assert np.array_equal(got["points"][:, :2], pv.lattice_points(mesh, 2).T.astype(dtype))
    want = op.latticeFields(torch.cat([fields["dens"][None], fields["vel"], fields["temp"][None]]), 2).numpy().astype(dtype)
    assert np.array_equal(got["point_data"]["dens"], want[0]) and np.array_equal(got["point_data"]["temp"], want[3])
    assert np.array_equal(got["point_data"]["vel"][:, :2], want[1:3].T) and np.all(got["point_data"]["vel"][:, 2] == 0.0)
    assert np.array_equal(got["connectivity"], pv.lattice_cells(2, mesh.num_elements, 2)[0])


def test_other_ranks_write_their_piece_only(tmp_path):
    import torch

    mesh = su.box(2)
    op = StandInOperator(mesh, order=1)
    coll = pv.ParaviewCollection(str(tmp_path), "run", op, levels=3, rank=2, nranks=3)
    coll.save(7, 0.5, {"dens": torch.zeros(op.NDofs, dtype=torch.float64)})
    assert os.listdir(tmp_path / "run") == ["Cycle000007"] and os.listdir(tmp_path / "run" / "Cycle000007") == ["proc000002.vtu"]


def test_tools_print_their_help():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "restart_to_paraview.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--levels" in r.stdout and "--physics" in r.stdout and "--ascii" in r.stdout
