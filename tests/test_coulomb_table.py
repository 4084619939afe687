"""The polynomial table of the eight Coulomb collision fits (tps_amd/csrc/coulomb_table.hpp) against 40-digit arithmetic.

tests/coulomb_table_main.cpp fills the table from the closure's own literals and evaluates it with the routine the kernels
use (one FMA per Horner step); it is compiled with AddressSanitizer / UndefinedBehaviorSanitizer and run as a program of its
own.  The bound is the project's bound for the composed exp / log it replaces (test_gpu_fastmath.py::
test_pow_through_exp_log): 4e-15 relative.  No GPU: the device evaluation is compared with this one bit for bit in
test_gpu_coulomb_table.py."""
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RTOL = 4e-15


def build_program(outdir):
    exe = os.path.join(str(outdir), "coulomb_table_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-Wno-unknown-pragmas", "-Wno-attributes", "-Wno-unused-variable", "-Wno-unused-but-set-variable",
           "-I" + os.path.join(HERE, "host_physics"), "-I" + os.path.join(ROOT, "tps_amd", "csrc"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "coulomb_table_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_program(exe, x):
    """(on the table?, values [n][8]) of the host evaluation; any sanitizer report fails the run"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input="".join(float(v).hex() + "\n" for v in x), capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    on = np.zeros(len(x), dtype=bool)
    g = np.full((len(x), 8), np.nan)
    lines = r.stdout.splitlines()
    assert len(lines) == len(x)
    for i, ln in enumerate(lines):
        tok = ln.split()
        on[i] = tok[0] == "1"
        if on[i]:
            g[i] = [float.fromhex(t) for t in tok[1:]]
    return on, g


def table_info(exe):
    r = subprocess.run([exe, "info"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    x0, h, ni, deg, nfit = lines[0].split()
    fits = [[float.fromhex(t) for t in ln.split()] for ln in lines[1:9]]
    return float.fromhex(x0), float.fromhex(h), int(ni), int(deg), fits


def reference(fits, x):
    """c0 [log(1 + c1 e^(c2 x))]^c3 of the reference's fits (src/collision_integrals.cpp:53-115) at 40 digits -> [n][8]"""
    import mpmath as mp

    with mp.workdps(40):
        cs = [[mp.mpf(v) for v in c] for c in fits]
        out = []
        for v in x:
            xv = mp.mpf(float(v))
            out.append([c[0] * mp.log(1 + c[1] * mp.exp(c[2] * xv)) ** c[3] for c in cs])
        return out


def worst_rel(g, ref):
    import mpmath as mp

    with mp.workdps(40):
        return max(float(abs(mp.mpf(float(g[i][f])) / ref[i][f] - 1)) for i in range(len(ref)) for f in range(8))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("coulomb_table"))


def test_layout(program):
    x0, h, ni, deg, fits = table_info(program)
    assert (h, deg) == (0.25, 9)
    assert x0 <= -4.0 and x0 + ni * h >= 40.0  # electron-free states (x ~ 36) stay on the table
    # the literals are the reference's: att11, rep22, rep23, rep24, att12 .. att15
    assert fits[0] == [0.2150, 5.2194, 1.0472, 1.2435] and fits[1] == [0.4128, 1.2436, 1.1830, 1.0123]
    assert fits[7] == [0.0232, 13.7888, 0.9148, 1.1532]


def test_accuracy(program):
    x0, h, ni, deg, fits = table_info(program)
    xend = x0 + ni * h
    rng = np.random.default_rng(18)
    edges = x0 + h * np.arange(ni + 1)
    # random arguments; every interval edge and its two neighbouring doubles (those on the table); the two range ends
    x = np.concatenate([rng.uniform(x0, xend, 20000), edges[:-1], np.nextafter(edges[1:], -np.inf), np.nextafter(edges[:-1], np.inf),
                        [x0, np.nextafter(xend, -np.inf)]])
    assert np.all((x >= x0) & (x < xend))
    on, g = run_program(program, x)
    assert on.all()
    w = worst_rel(g, reference(fits, x))
    print(f"worst relative error of the table against 40 digits, {len(x)} arguments x 8 fits: {w:.3e}")
    assert w < RTOL


def test_off_the_table(program):
    x0, h, ni, deg, fits = table_info(program)
    xend = x0 + ni * h
    x = [math.nan, np.nextafter(x0, -np.inf), xend, -math.inf, math.inf, 1e300, -1e300, x0, np.nextafter(xend, -np.inf)]
    on, _ = run_program(program, x)
    assert on.tolist() == [False] * 7 + [True, True]
