"""The lattice entries of the C ABI without a device (tpsrhs_lattice_size, tpsrhs_lattice_coordinates,
tpsrhs_lattice_fields): the symbols are declared, exported and prototyped; the host-only size entry counts the points of
every element's closed lattice; every invalid call answers TPSRHS_ERR_INVALID_ARGUMENT and names its entry before any device
work.  The calls that need a handle run in a stand-alone program (tests/lattice_capi_main.cpp, its own main, built with
hipcc for the host only): no operator can be created without a device, and the size entry reads only dim and the element
count of the one the program fills in.  The values are in tests/test_gpu_lattice.py."""
import ctypes as C
import os
import subprocess

import pytest

from tps_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tps_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ["tpsrhs_lattice_size", "tpsrhs_lattice_coordinates", "tpsrhs_lattice_fields"]


def test_symbols_are_exported_and_prototyped():
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTED_SYMBOLS
    vp, ip64 = C.c_void_p, C.POINTER(C.c_int64)
    assert lib.tpsrhs_lattice_size.argtypes == [vp, C.c_int, ip64, ip64]
    assert lib.tpsrhs_lattice_coordinates.argtypes == [vp, C.c_int, vp]
    assert lib.tpsrhs_lattice_fields.argtypes == [vp, C.c_int, C.c_int, vp, vp, C.c_int]


def test_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "tpsrhs.h")).read()
    assert "#define TPSRHS_MAXLATTICE 8" in hdr
    assert "int tpsrhs_lattice_size(tpsrhs_handle h, int levels, int64_t *points_per_element, int64_t *npts);" in hdr
    assert "int tpsrhs_lattice_coordinates(tpsrhs_handle h, int levels, double *xyz_out);" in hdr
    assert "int tpsrhs_lattice_fields(tpsrhs_handle h, int levels, int nrows, const double *field, void *out, int out_float32);" in hdr


def test_invalid_calls_through_ctypes_look_behind_no_pointer():
    lib = capi.load()
    fake = (C.c_double * 64)()  # stands for a handle and for device arrays
    p = C.cast(fake, C.c_void_p)
    a, b = C.c_int64(-7), C.c_int64(-7)
    for args in ((None, 3, C.byref(a), C.byref(b)), (p, 3, None, C.byref(b)), (p, 3, C.byref(a), None),
                 (p, 0, C.byref(a), C.byref(b)), (p, 9, C.byref(a), C.byref(b))):
        assert lib.tpsrhs_lattice_size(*args) == capi.ERR_INVALID_ARGUMENT
        assert "tpsrhs_lattice_size" in lib.tpsrhs_last_error().decode()
    assert (a.value, b.value) == (-7, -7)
    for args in ((None, 3, p), (p, 3, None), (p, 0, p), (p, 9, p), (p, -2, p)):
        assert lib.tpsrhs_lattice_coordinates(*args) == capi.ERR_INVALID_ARGUMENT
        assert "tpsrhs_lattice_coordinates" in lib.tpsrhs_last_error().decode()
    for args in ((None, 3, 1, p, p, 0), (p, 3, 1, None, p, 0), (p, 3, 1, p, None, 1), (p, 0, 1, p, p, 0), (p, 9, 1, p, p, 1),
                 (p, 3, 0, p, p, 0), (p, 3, -1, p, p, 1)):
        assert lib.tpsrhs_lattice_fields(*args) == capi.ERR_INVALID_ARGUMENT
        assert "tpsrhs_lattice_fields" in lib.tpsrhs_last_error().decode()
    assert not any(fake)


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lattice_capi") / "lattice_capi_main")
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", os.path.join(HERE, "lattice_capi_main.cpp"), "-o", exe,
           "-L" + CSRC, "-ltpsrhs", "-Wl,-rpath," + CSRC]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return [line.split() for line in r.stdout.splitlines()]


def test_lattice_size_counts_the_points(program_output):
    sizes = [t for t in program_output if t[0] == "size"]
    assert len(sizes) == 6
    seen = set()
    for _, dim, ne, levels, st, ppe, npts in sizes:
        dim, ne, levels = int(dim), int(ne), int(levels)
        assert int(st) == 0
        assert int(ppe) == (levels + 1) ** dim and int(npts) == ne * (levels + 1) ** dim
        seen.add((dim, levels))
    assert seen == {(d, L) for d in (2, 3) for L in (1, 3, 8)}


def test_every_invalid_call_is_refused_with_the_entry_named(program_output):
    refusals = [t for t in program_output if t[0] == "refused"]
    cases = {(t[1], t[2]) for t in refusals}
    for entry in NEW:
        assert (entry, "null_handle") in cases and (entry, "levels") in cases
    assert {("tpsrhs_lattice_size", "null_ppe"), ("tpsrhs_lattice_size", "null_npts"), ("tpsrhs_lattice_coordinates", "null_out"),
            ("tpsrhs_lattice_fields", "null_field"), ("tpsrhs_lattice_fields", "null_out"), ("tpsrhs_lattice_fields", "nrows")} <= cases
    assert sum(1 for t in refusals if t[2] == "levels") == 9  # levels 0, 9, -1 for each of the three entries
    for _, entry, what, status, named in refusals:
        assert int(status) == capi.ERR_INVALID_ARGUMENT, (entry, what)
        assert named == "1", (entry, what)
    assert ["untouched", "1", "1"] in program_output
