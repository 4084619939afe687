"""ParaView output of DG fields: the reference's ``ParaViewDataCollection`` with ``SetLevelsOfDetail(order)``
(``src/M2ulPhyS.cpp:443-446, 1877-1906``; ``paraviewColl->Save()`` at ``:2043-2045, 4131-4133``).

MFEM evaluates every registered grid function at a closed uniform lattice of each element and writes one ``.vtu`` per
rank with ``levels^dim`` linear sub-cells per element.  Here the values come from ``RHSoperator.latticeFields`` (one kernel
over all rows, ``tpsrhs_lattice_fields``) and this module is the host half: the lattice points restated in numpy, the
sub-cell connectivity, the ``.vtu`` / ``.pvtu`` / ``.pvd`` files.  numpy only; nothing here runs on the device, and
nothing here communicates: rank and rank count are arguments.

The file layout (VTK XML, ``UnstructuredGrid``, version 1.0, little endian, UInt64 headers) is the contract; the files
have not been opened in ParaView.  VTK Lagrange cells (``SetHighOrderOutput(true)``) are not written: the sub-cells at
``levels = order`` show the same point values.
"""
from __future__ import annotations

import os
import struct

import numpy as np

VTK_QUAD, VTK_HEXAHEDRON = 9, 12
_LEX_TO_MFEM = {2: (0, 1, 3, 2), 3: (0, 1, 3, 2, 4, 5, 7, 6)}  # lexicographic corner (bit d = coordinate d) -> MFEM vertex
_VTK_TYPE = {np.dtype(np.float64): "Float64", np.dtype(np.float32): "Float32", np.dtype(np.int64): "Int64",
             np.dtype(np.uint8): "UInt8"}
_HEADER = '<VTKFile type="{}" version="1.0" byte_order="LittleEndian" header_type="UInt64">'


def lattice_reference(dim, levels):
    """reference coordinates of one element's lattice, ``(dim, (levels + 1)^dim)``: ``t_a = a / levels``,
    ``local = a + b (levels + 1) + c (levels + 1)^2``"""
    n = levels + 1
    t = np.arange(n, dtype=np.float64) / np.float64(levels)
    loc = np.arange(n ** dim)
    return np.stack([t[(loc // n ** d) % n] for d in range(dim)])


def lattice_points(host_mesh, levels):
    """The lattice points of ``tpsrhs_lattice_coordinates`` in numpy, ``(dim, num_elements (levels + 1)^dim)``: the
    bi-/trilinear vertex map through ``elem_coords`` with the shape weights formed as products of ``t`` and ``1 - t`` and
    summed over the corners in lexicographic order, as the device does.  A lattice corner is the element's vertex bit
    for bit."""
    if not 1 <= levels:
        raise ValueError("levels >= 1")
    dim = host_mesh.dim
    ex = np.asarray(host_mesh.elem_coords, dtype=np.float64)  # (ne, 2^dim, dim)
    xi = lattice_reference(dim, levels)
    out = np.zeros((dim, ex.shape[0], xi.shape[1]))
    for c, v in enumerate(_LEX_TO_MFEM[dim]):
        w = np.ones(xi.shape[1])
        for d in range(dim):
            w = w * (xi[d] if (c >> d) & 1 else 1.0 - xi[d])
        out += ex[:, v, :].T[:, :, None] * w[None, None, :]
    return out.reshape(dim, -1)


def lattice_cells(dim, num_elements, levels):
    """``levels^dim`` linear sub-cells per element over the point numbering of :func:`lattice_points`:
    ``(connectivity, offsets, types)``.  ``VTK_QUAD``: corners (i,j), (i+1,j), (i+1,j+1), (i,j+1); ``VTK_HEXAHEDRON``: that
    quad at k, then at k+1.  ``offsets`` are the cumulative ends VTK stores; sub-cell i fastest, elements in order."""
    n, L = levels + 1, levels
    idx = np.arange(L ** dim)
    i, j = idx % L, (idx // L) % L
    base = i + j * n
    quad = np.stack([base, base + 1, base + 1 + n, base + n], axis=1)
    if dim == 3:
        k = idx // (L * L)
        quad = quad + (k * n * n)[:, None]
        quad = np.concatenate([quad, quad + n * n], axis=1)
    nv = quad.shape[1]
    conn = (quad[None, :, :] + (np.arange(num_elements, dtype=np.int64) * n ** dim)[:, None, None]).reshape(-1)
    ncells = num_elements * L ** dim
    offsets = (np.arange(ncells, dtype=np.int64) + 1) * nv
    types = np.full(ncells, VTK_HEXAHEDRON if dim == 3 else VTK_QUAD, dtype=np.uint8)
    return conn.astype(np.int64), offsets, types


def _as_point_array(name, a, npts):
    """``[npts]`` or ``[ncomp, npts]`` -> (interleaved array ``(npts, ncomp')``, ncomp'): two components are padded to three"""
    a = np.asarray(a)
    if a.dtype not in (np.float64, np.float32):
        a = a.astype(np.float64)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != npts:
        raise ValueError(f"point data {name!r}: expected [npts] or [ncomp, npts] with npts = {npts}, got {a.shape}")
    if a.shape[0] == 2:
        a = np.concatenate([a, np.zeros((1, npts), dtype=a.dtype)])
    return np.ascontiguousarray(a.T), a.shape[0]


def _ascii(a):
    if a.dtype == np.float64:
        fmt = "%.17g"
    elif a.dtype == np.float32:
        fmt = "%.9g"
    else:
        fmt = "%d"
    return "\n".join(" ".join(fmt % v for v in row) for row in a.reshape(a.shape[0], -1).tolist())


def write_vtu(path, points, cells, point_data, encoding="appended"):
    """One ``UnstructuredGrid`` piece.  ``points``: ``(dim, npts)`` float64 or float32 (2-D points get z = 0);
    ``cells``: what :func:`lattice_cells` returns; ``point_data``: name -> ``[npts]`` or ``[ncomp, npts]`` (a two-component
    vector is padded to three).  ``encoding``: ``"ascii"`` (17 significant digits for Float64, 9 for Float32) or
    ``"appended"`` (``<AppendedData encoding="raw">``, an underscore, then per array a UInt64 byte count and the raw
    little-endian bytes; ``offset`` attributes count from the byte after the underscore)."""
    if encoding not in ("ascii", "appended"):
        raise ValueError('encoding is "ascii" or "appended"')
    points = np.asarray(points)
    if points.dtype not in (np.float64, np.float32):
        points = points.astype(np.float64)
    if points.ndim != 2 or points.shape[0] not in (2, 3):
        raise ValueError("points: expected (dim, npts) with dim 2 or 3")
    npts = points.shape[1]
    xyz = np.zeros((npts, 3), dtype=points.dtype)
    xyz[:, :points.shape[0]] = points.T
    conn, offsets, types = (np.ascontiguousarray(c) for c in cells)
    conn, offsets, types = conn.astype(np.int64, copy=False), offsets.astype(np.int64, copy=False), types.astype(np.uint8, copy=False)
    arrays = []  # (section, name, ncomp, array)
    arrays.append(("Points", "Points", 3, xyz))
    arrays += [("Cells", "connectivity", 1, conn), ("Cells", "offsets", 1, offsets), ("Cells", "types", 1, types)]
    for name, a in point_data.items():
        arr, ncomp = _as_point_array(name, a, npts)
        arrays.append(("PointData", name, ncomp, arr))

    blobs, offset = [], 0
    lines = ['<?xml version="1.0"?>', _HEADER.format("UnstructuredGrid"), "<UnstructuredGrid>",
             f'<Piece NumberOfPoints="{npts}" NumberOfCells="{types.size}">']
    section = None
    for sec, name, ncomp, a in arrays:
        if sec != section:
            if section is not None:
                lines.append(f"</{section}>")
            lines.append(f"<{sec}>")
            section = sec
        head = f'<DataArray type="{_VTK_TYPE[a.dtype]}" Name="{name}" NumberOfComponents="{ncomp}"'
        if encoding == "ascii":
            lines.append(head + ' format="ascii">')
            lines.append(_ascii(a))
            lines.append("</DataArray>")
        else:
            raw = a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()
            lines.append(head + f' format="appended" offset="{offset}"/>')
            blobs.append(struct.pack("<Q", len(raw)) + raw)
            offset += 8 + len(raw)
    lines.append(f"</{section}>")
    lines += ["</Piece>", "</UnstructuredGrid>"]
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())
        if encoding == "appended":
            f.write(b'<AppendedData encoding="raw">\n_')
            for b in blobs:
                f.write(b)
            f.write(b"\n</AppendedData>\n")
        f.write(b"</VTKFile>\n")


def write_pvtu(path, pieces, point_arrays, points_type="Float32"):
    """The parallel index of one cycle: ``pieces`` are the file names of the ranks' ``.vtu``, ``point_arrays`` is
    ``[(name, VTK type, number of components)]`` as the pieces hold them."""
    lines = ['<?xml version="1.0"?>', _HEADER.format("PUnstructuredGrid"), '<PUnstructuredGrid GhostLevel="0">',
             "<PPoints>", f'<PDataArray type="{points_type}" Name="Points" NumberOfComponents="3"/>', "</PPoints>",
             "<PPointData>"]
    lines += [f'<PDataArray type="{t}" Name="{n}" NumberOfComponents="{c}"/>' for n, t, c in point_arrays]
    lines.append("</PPointData>")
    lines += [f'<Piece Source="{p}"/>' for p in pieces]
    lines += ["</PUnstructuredGrid>", "</VTKFile>"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_pvd(path, entries):
    """``entries``: ``[(time, file relative to the .pvd)]``, one ``DataSet`` each"""
    lines = ['<?xml version="1.0"?>', '<VTKFile type="Collection" version="0.1" byte_order="LittleEndian">', "<Collection>"]
    lines += [f'<DataSet timestep="{float(t)!r}" group="" part="0" file="{f}"/>' for t, f in entries]
    lines += ["</Collection>", "</VTKFile>"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _numpy_dtype(dtype):
    name = str(dtype).replace("torch.", "")
    if name not in ("float32", "float64"):
        name = np.dtype(dtype).name
    if name not in ("float32", "float64"):
        raise ValueError("dtype is float32 or float64")
    return np.dtype(name)


class ParaviewCollection:
    """How the reference uses ``ParaViewDataCollection``: ``<prefix>/<name>/Cycle%06d/proc%06d.vtu`` per save and rank, a
    ``data.pvtu`` next to the pieces naming those of all ranks, and ``<prefix>/<name>/<name>.pvd`` with one ``DataSet`` per
    saved cycle, rewritten at every save (the index files by rank 0).  ``levels`` defaults to the operator's order
    (``SetLevelsOfDetail(order)``).  The points and cells are built once; a save is one ``latticeFields`` launch over the
    stacked rows, one copy to the host and one file."""

    def __init__(self, prefix, name, op, levels=None, dtype=np.float32, rank=0, nranks=1, encoding="appended"):
        self.prefix, self.name, self.op = str(prefix), str(name), op
        self.levels = int(op._disc.order if levels is None else levels)
        self.dtype = _numpy_dtype(dtype)
        self.rank, self.nranks, self.encoding = int(rank), int(nranks), encoding
        self.dir = os.path.join(self.prefix, self.name)
        xyz = op.latticeCoordinates(self.levels)
        self.points = xyz.cpu().numpy().astype(self.dtype)
        dim = self.points.shape[0]
        npe = (self.levels + 1) ** dim
        self.npts = self.points.shape[1]
        self.cells = lattice_cells(dim, self.npts // npe, self.levels)
        self.cycles = []  # (cycle, time) in the order of the saves

    def save(self, cycle, time, fields):
        """``fields``: name -> byNODES tensor ``[NDofs]`` or ``[ncomp, NDofs]`` of the operator (float64).  Returns the
        path of this rank's piece."""
        import torch

        names = list(fields)
        if not names:
            raise ValueError("no fields to save")
        rows = [fields[n].reshape(1, -1) if fields[n].dim() == 1 else fields[n] for n in names]
        counts = [int(r.shape[0]) for r in rows]
        stacked = torch.cat(rows).contiguous()
        tdtype = torch.float32 if self.dtype == np.float32 else torch.float64
        host = self.op.latticeFields(stacked, self.levels, dtype=tdtype).cpu().numpy()
        data, first = {}, 0
        for n, c in zip(names, counts):
            data[n] = host[first] if c == 1 else host[first:first + c]
            first += c
        cdir = os.path.join(self.dir, "Cycle%06d" % cycle)
        os.makedirs(cdir, exist_ok=True)
        piece = os.path.join(cdir, "proc%06d.vtu" % self.rank)
        write_vtu(piece, self.points, self.cells, data, self.encoding)
        self.cycles = [(c, t) for c, t in self.cycles if c != cycle] + [(int(cycle), float(time))]
        if self.rank == 0:
            vtype = _VTK_TYPE[self.dtype]
            arrays = [(n, vtype, 1 if c == 1 else 3 if c == 2 else c) for n, c in zip(names, counts)]
            write_pvtu(os.path.join(cdir, "data.pvtu"), ["proc%06d.vtu" % r for r in range(self.nranks)], arrays, vtype)
            write_pvd(os.path.join(self.dir, self.name + ".pvd"),
                      [(t, "Cycle%06d/data.pvtu" % c) for c, t in self.cycles])
        return piece


def reference_fields(op, x, species_names=None):
    """The fields the reference registers with its collection (``src/M2ulPhyS.cpp:1658-1679, 1880-1903``) at the state
    ``x`` of the operator ``op``, name -> byNODES device tensor: ``dens`` (Up row 0), ``vel`` (rows 1..dim), ``vtheta``
    (row 3, axisymmetric), ``temp`` (row 1 + nvel), ``press``, ``Te`` (the last row of a two-temperature plasma), for
    mixtures every field of :meth:`RHSoperator.visualizationFields`, and ``sigma`` where the operator's physics stores a
    plasma conductivity."""
    import ctypes as C

    import torch

    from . import capi
    from .rhs_operator import TpsRhsError

    ph, dim = op._physics, op.dim
    axisym = bool(op._disc.axisymmetric)
    nvel = 3 if axisym else dim
    mixture = ph.working_fluid == capi.USER_DEFINED
    vis = op.visualizationFields(x, species_names) if mixture else None  # refreshes Up from x
    if vis is None:
        op.updateGradients(x)
    up = op.getPrimitives()
    fields = {"dens": up[0], "vel": up[1:1 + dim]}
    if axisym:
        fields["vtheta"] = up[3]
    fields["temp"] = up[1 + nvel]
    press = torch.empty(op.NDofs, dtype=torch.float64, device=op.device)
    st = op._lib.tpsrhs_eval_pointwise(op._h, 1, op.NDofs, C.c_void_p(x.data_ptr()), C.c_void_p(press.data_ptr()))
    if st != 0:
        raise TpsRhsError(st, "tpsrhs_eval_pointwise")
    fields["press"] = press
    if mixture and ph.mixture.two_temperature:
        fields["Te"] = up[op.num_equation - 1]
    if vis is not None:
        fields.update(vis)
    try:
        fields["sigma"] = op.getPlasmaConductivity(x)
    except TpsRhsError as e:
        if e.status != capi.ERR_UNSUPPORTED:
            raise
    return fields
