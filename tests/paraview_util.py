"""A small reader of the .vtu / .pvtu / .pvd files of tps_amd.paraview, written against the layout its issue fixes and
sharing no code with the writer: xml.etree for the markup, struct / numpy.frombuffer for the raw appended block
(`<AppendedData encoding="raw">`, an underscore, then per array a UInt64 byte count and the little-endian bytes; `offset`
attributes count from the byte after the underscore).  Used by tests/test_paraview_writer.py and tests/test_gpu_lattice.py."""
import struct
import xml.etree.ElementTree as ET

import numpy as np

HEADER = b'<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64">'
NP_TYPE = {"Float64": "<f8", "Float32": "<f4", "Int64": "<i8", "UInt8": "u1"}
MARK = b'<AppendedData encoding="raw">'


def read_vtu(path):
    """-> dict: npoints, ncells, points (npts, 3), connectivity, offsets, types, point_data {name: (npts, ncomp)},
    order (the PointData names as written), vtk_types {array name: VTK type}, appended [(offset attribute, byte count)]"""
    blob = open(path, "rb").read()
    assert HEADER in blob.split(b"\n", 2)[1], "the VTKFile header line"
    raw = None
    if MARK in blob:
        head, tail = blob.split(MARK, 1)
        k = tail.index(b"_")
        assert tail[:k].strip() == b""
        raw = tail[k + 1:]
        assert raw.rstrip().endswith(b"</VTKFile>")
        blob = head + b"</VTKFile>"
    root = ET.fromstring(blob)
    assert root.tag == "VTKFile" and root.attrib == {"type": "UnstructuredGrid", "version": "1.0", "byte_order": "LittleEndian",
                                                     "header_type": "UInt64"}
    piece = root.find("UnstructuredGrid/Piece")
    out = {"npoints": int(piece.attrib["NumberOfPoints"]), "ncells": int(piece.attrib["NumberOfCells"]), "point_data": {},
           "order": [], "vtk_types": {}, "appended": []}

    def array(el):
        dt, ncomp = NP_TYPE[el.attrib["type"]], int(el.attrib["NumberOfComponents"])
        if el.attrib["format"] == "ascii":
            toks = el.text.split()
            a = np.array([int(t) for t in toks] if dt[1] in "iu" or dt == "u1" else [float(t) for t in toks]).astype(dt)
        else:
            assert el.attrib["format"] == "appended" and raw is not None
            off = int(el.attrib["offset"])
            (nbytes,) = struct.unpack("<Q", raw[off:off + 8])
            a = np.frombuffer(raw[off + 8:off + 8 + nbytes], dtype=dt)
            out["appended"].append((off, nbytes))
        out["vtk_types"][el.attrib["Name"]] = el.attrib["type"]
        return a.reshape(-1, ncomp) if ncomp > 1 else a

    (pts,) = piece.findall("Points/DataArray")
    out["points"] = array(pts)
    for el in piece.findall("Cells/DataArray"):
        out[el.attrib["Name"]] = array(el)
    for el in piece.findall("PointData/DataArray"):
        out["point_data"][el.attrib["Name"]] = array(el)
        out["order"].append(el.attrib["Name"])
    if raw is not None:  # the offsets are consistent with the byte counts: the arrays tile the block in file order
        pos = 0
        for off, nbytes in out["appended"]:
            assert off == pos
            pos += 8 + nbytes
        assert raw[pos:].split() == [b"</AppendedData>", b"</VTKFile>"]
    return out


def read_pvtu(path):
    """-> (piece sources, [(name, type, ncomp)] of PPointData, type of the points)"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.attrib["type"] == "PUnstructuredGrid"
    g = root.find("PUnstructuredGrid")
    arrays = [(e.attrib["Name"], e.attrib["type"], int(e.attrib["NumberOfComponents"])) for e in g.findall("PPointData/PDataArray")]
    (pts,) = g.findall("PPoints/PDataArray")
    return [e.attrib["Source"] for e in g.findall("Piece")], arrays, pts.attrib["type"]


def read_pvd(path):
    """-> [(timestep, file)]"""
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.attrib["type"] == "Collection"
    return [(float(e.attrib["timestep"]), e.attrib["file"]) for e in root.findall("Collection/DataSet")]
