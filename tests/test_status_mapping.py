"""guarded() of tps_amd/csrc/status.hpp -- the wrapper every entry point of the C ABI runs its body in -- maps an exception
to a status of include/tpsrhs.h by its TYPE and keeps its text for tpsrhs_last_error.  A stand-alone program
(tests/status_main.cpp, its own main) includes the header alone, throws one exception of each class through guarded() and
prints what came back; the plain runtime_error's text says "halo" and "no HIP device" and must still be a mesh error.  The
second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process;
nothing is loaded into Python."""
import os
import subprocess

import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID_ARGUMENT, UNSUPPORTED, MESH, DEVICE, NO_DEVICE, HALO = range(7)  # tpsrhs_status, include/tpsrhs.h
WANT = [
    ("ok", OK, "-"),
    ("Unsupported", UNSUPPORTED, "order 9 is not built"),
    ("DeviceError", DEVICE, "hipMalloc: out of memory"),
    ("NoDevice", NO_DEVICE, "nothing to run on"),
    ("HaloError", HALO, "the exchange callback failed"),
    ("invalid_argument", INVALID_ARGUMENT, "NULL mesh"),
    ("runtime_error", MESH, "mesh: a halo face, and no HIP device, in the text only"),
    ("logic_error", INVALID_ARGUMENT, "two predicates disagree"),
    ("bad_alloc", INVALID_ARGUMENT, "std::bad_alloc"),
    ("ok_again", OK, "-"),
]


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "status_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    want = [f"{what} status {st} text {text}" for what, st, text in WANT]
    want += ["last std::bad_alloc", f"fail {MESH} said directly", "STATUS DONE"]
    got = r.stdout.splitlines()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {k + 1}: got {g!r}, expected {w!r}"
    assert len(got) == len(want)


def test_every_exception_class_has_its_status(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "status"))


def test_status_mapping_is_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "status_sanitize"))
