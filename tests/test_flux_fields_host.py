"""The per-node body of tpsrhs_get_flux (tps_amd/csrc/flux_fields.hpp) compiled for the host: a stand-alone program
(tests/flux_fields_main.cpp, its own main) built with g++ against the stand-in tests/host_physics/hip/hip_runtime.h, plain
and with AddressSanitizer + UndefinedBehaviorSanitizer, and run as a child process.  Nothing is loaded into Python.

The headers are the product's, copied with ONE line dropped (the AMDGPU register constraint of `relaunder`), as
tests/host_physics/Makefile does."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tps_amd import capi, cases

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "tps_amd", "csrc")
DROP = 'asm volatile("" : "+s"(lo), "+s"(hi));'
N = 257


def _gradients(rng, scales, dim, n, length=0.05):
    """random primitive gradients [d][eq][n] of the magnitudes a field of these scales has over `length`"""
    g = rng.standard_normal((dim, len(scales), n))
    return g * (np.asarray(scales)[None, :, None] / length)


def _dump(path, U, G, radius):
    neq, n = U.shape
    dim = G.shape[0]
    with open(path, "wb") as f:
        np.array([n, neq, dim], dtype=np.float64).tofile(f)
        np.ascontiguousarray(U, dtype=np.float64).tofile(f)
        np.ascontiguousarray(G, dtype=np.float64).tofile(f)
        np.ascontiguousarray(radius, dtype=np.float64).tofile(f)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("flux_fields_host"))
    rng = np.random.default_rng(20240611)
    ones = np.ones(N)
    X3 = rng.uniform(0.0, 1.0, (3, N))
    _dump(os.path.join(d, "dry3d.bin"), cases.dry_air_state(X3, seed=3), _gradients(rng, [1.2, 20, 20, 20, 300], 3, N), ones)
    X2 = rng.uniform(0.0, 1.0, (2, N))
    radius = rng.uniform(1e-3, 0.05, N)
    _dump(os.path.join(d, "axi.bin"), cases.dry_air_state(X2, seed=4, vel0=(1.0, 20.0, 3.0), nvel=3),
          _gradients(rng, [1.2, 20, 20, 20, 300], 2, N), radius)
    ph = capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL)
    U = cases.plasma_state(X2, ph, nvel=2, seed=5)
    _dump(os.path.join(d, "plasma2d.bin"), U, _gradients(rng, [U[0].mean(), 20, 20, 5000, np.abs(U[4]).mean()], 2, N), ones)
    with open(os.path.join(d, "disc.bin"), "wb") as f:
        f.write(bytes(capi.Disc(2, 0, 0, 0, 0)))
    with open(os.path.join(d, "physics.bin"), "wb") as f:
        f.write(bytes(ph))
    # the product's headers, one line dropped
    src = os.path.join(d, "src")
    os.makedirs(src)
    for h in glob.glob(os.path.join(CSRC, "*.hpp")):
        with open(h) as f, open(os.path.join(src, os.path.basename(h)), "w") as g:
            g.writelines(line for line in f if DROP not in line)
    return d


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_flux_parts_on_the_host(inputs, sanitize):
    d = inputs
    exe = os.path.join(d, "flux_fields_main_san" if sanitize else "flux_fields_main")
    # (the sanitizer runtimes are linked statically: the program needs nothing of its environment to start)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan",
           "-static-libubsan"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes", "-Wno-unused-variable",
           "-Wno-unused-but-set-variable", "-Wno-unused-function"] + san + \
          ["-I", os.path.join(HERE, "host_physics"), "-I", os.path.join(d, "src"), os.path.join(HERE, "flux_fields_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe] + [os.path.join(d, f) for f in ("disc.bin", "physics.bin", "dry3d.bin", "axi.bin", "plasma2d.bin")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("-> ok") == 4 and "FAILED" not in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
