"""tps_amd/csrc/modal.hpp under AddressSanitizer + UndefinedBehaviorSanitizer: the header is plain C++, so a stand-alone
program (tests/modal_main.cpp, its own main) includes it alone, is built with g++ and the sanitizers and runs as a child
process.  It checks V V^-1 = I for every order and both node sets, the closed values of sigma, every refusal of the plan,
and the scalar restatement of the three operations (transform, shell energies and sensor, filter with decision and mean
correction) on one 2-D and one 3-D element against numbers tests/modal_util.py writes in long double, within that module's
error model.  Nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import modal_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]  # the runtimes inside the program: nothing is preloaded, nothing has to come first

# (dim, p, basis, neq, cutoff, alpha, exponent, conservative, sensor_row, threshold): a filtered 2-D Lobatto element, a filtered
# 3-D Legendre element with a sensor, a 3-D element the sensor leaves alone, a non-conservative 2-D one
CASES = [(2, 3, 1, 3, 1, 6.0, 2, 1, -1, 0.0), (3, 2, 0, 2, 0, 36.0, 16, 1, 1, 1e-3), (3, 3, 0, 2, 2, 4.0, 1, 1, 0, 0.999),
         (2, 5, 0, 1, 4, 1.5, 3, 0, 0, 1e-6)]


def _sanitizer_runtime_missing(tmp_path):
    """True where g++ cannot link a trivial program with the sanitizers (their runtime libraries are not installed)"""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + FLAGS + [str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode != 0


def _fixture(path):
    """per case: dim p basis neq cutoff alpha exponent conservative sensor_row threshold filtered | W | x | u^ of row 0 and its
    bound | E, dE of row 0 | S dS | the filtered state and its bound"""
    rng = np.random.default_rng(17)
    fmt = lambda a: " ".join("%.17g" % float(v) for v in np.asarray(a).reshape(-1))  # noqa: E731
    lines = [str(len(CASES))]
    for dim, p, basis, neq, kc, alpha, s, cons, srow, thr in CASES:
        npe = (p + 1) ** dim
        W = 0.5 + rng.random(npe)  # positive and uneven, as on a warped element
        x = rng.standard_normal((neq, npe))
        en = mu.energies(x[0], p, basis, dim)
        ref = mu.modal_filter(x, W, dim, p, basis, None, kc, alpha, s, bool(cons), srow, thr)
        lines.append(f"{dim} {p} {basis} {neq} {kc} {alpha!r} {s} {cons} {srow} {thr!r} {int(ref['filtered'][0])}")
        lines += [fmt(W), fmt(x), fmt(en["uhat"]), fmt(en["duhat"]), fmt(en["E"]), fmt(en["dE"]),
                  fmt([en["S"][0], en["dS"][0]]), fmt(ref["x"]), fmt(ref["bound"])]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_the_fixture_crosses_both_decisions():
    got = []
    rng = np.random.default_rng(17)
    for dim, p, basis, neq, kc, alpha, s, cons, srow, thr in CASES:
        npe = (p + 1) ** dim
        W, x = 0.5 + rng.random(npe), rng.standard_normal((neq, npe))
        got.append(bool(mu.modal_filter(x, W, dim, p, basis, None, kc, alpha, s, bool(cons), srow, thr)["filtered"][0]))
    assert got == [True, True, False, True]


def test_modal_operations_are_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    exe = str(tmp_path / "modal_host")
    b = subprocess.run(["g++"] + FLAGS + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "modal_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    fixture = str(tmp_path / "modal_fixture.txt")
    _fixture(fixture)
    r = subprocess.run([exe, fixture], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MODAL CLEAN" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
