"""locate_one of tps_amd/csrc/point_locate.hpp -- the per-point function the device kernel k_locate runs -- against
locate_points, entry by entry and bit for bit, in a stand-alone program (tests/locate_one_main.cpp, its own main) that
includes the header alone and is built with plain g++: the search structure is built once (build_locate_grid) and the points
go through locate_one one at a time.  The second case builds the same program with AddressSanitizer and
UndefinedBehaviorSanitizer and runs it as a child process; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import transfer_util as tu
from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = {
    "hex_warped_3x3x3": lambda: tu.box(3, (3, 3, 3), (1.5, 1.0, 0.7), warp=0.1),
    "quad_warped_4x4": lambda: tu.box(2, (4, 4), (1.5, 1.0), warp=0.1),
    "ogrid_4x12x3": tu.LOCATE_MESHES["ogrid"],
}


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "locate_one_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _write_inputs(tmp_path):
    files = []
    for k, (name, make) in enumerate(MESHES.items()):
        mesh = make()
        xyz = tu.point_set(mesh, 300, 300, seed=20 + k)
        path = str(tmp_path / f"{name}.bin")
        with open(path, "wb") as f:
            np.array([mesh.dim, mesh.num_elements, xyz.shape[1]], dtype=np.int32).tofile(f)
            np.ascontiguousarray(mesh.elem_coords, dtype=np.float64).tofile(f)
            np.ascontiguousarray(xyz, dtype=np.float64).tofile(f)
        files.append((name, path, xyz.shape[1]))
    return files


def _run(exe, files):
    for name, path, npts in files:
        for tol in ("0", "1e-6"):
            r = subprocess.run([exe, path, tol], capture_output=True, text=True, timeout=120)
            print(name, tol, r.stdout.strip().replace("\n", "; "))
            assert r.returncode == 0 and "LOCATE_ONE EQUAL" in r.stdout, name + r.stdout[-3000:] + r.stderr[-3000:]
            assert f"points {npts} found" in r.stdout
            found = int(r.stdout.split("found")[1].split()[0])
            assert 600 <= found < npts  # the interior and boundary points are found, the points outside and the NaN are not
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_locate_one_equals_locate_points_bit_for_bit(tmp_path):
    exe = _build(tmp_path, ["-std=c++17", "-O2"], "locate_one")
    _run(exe, _write_inputs(tmp_path))


def test_locate_one_is_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    exe = _build(tmp_path, SANITIZE_FLAGS, "locate_one_sanitize")
    _run(exe, _write_inputs(tmp_path))
