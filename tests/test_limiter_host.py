"""tps_amd/csrc/limiter.hpp under AddressSanitizer + UndefinedBehaviorSanitizer: the header is plain C++, so a stand-alone
program (tests/limiter_main.cpp, its own main) includes it alone, is built with g++ and the sanitizers and runs as a child
process -- the row step and the pressure step of the conservative limiter on elements of 4, 9, 27, 64 and 216 nodes against
closed forms (untouched, limited, clamped, NaN; the three pressure outcomes).  Nothing is loaded into Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]  # the runtimes inside the program: nothing is preloaded, nothing has to come first


def _sanitizer_runtime_missing(tmp_path):
    """True where g++ cannot link a trivial program with the sanitizers (their runtime libraries are not installed)"""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + FLAGS + [str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode != 0


def test_limiter_operations_are_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    exe = str(tmp_path / "limiter_host")
    b = subprocess.run(["g++"] + FLAGS + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "limiter_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LIMITER CLEAN" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
