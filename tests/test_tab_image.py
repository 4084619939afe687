"""The packed image of a block's 1-D tables (tps_amd/csrc/tab_image.hpp::make_tab_image) that the staged prologue of the 3-D
p = 3 sweeps copies to LDS word by word, against what the lanes of a block copy there themselves (tab_lane_copy, the body of
kernels.hpp::load_tables): the same bits in every member, 1 / w included.  tests/tab_image_main.cpp is host code only,
compiled with AddressSanitizer / UndefinedBehaviorSanitizer and run as a program of its own.  No GPU: that the device's
division gives the host's bits is what test_gpu_staged_prologue.py pins."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEMBERS = ("x", "w", "iw", "D", "b0", "b1", "xq", "wq", "B", "xv", "wv")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("tab_image")), "tab_image_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-I" + os.path.join(ROOT, "tps_amd", "csrc"), os.path.join(HERE, "tab_image_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(r.stdout)
    assert not r.stderr, r.stderr[-3000:]  # any sanitizer report
    rows = {}
    for ln in r.stdout.splitlines():
        tok = ln.split()
        dim, p, nc, doubles = (int(t) for t in tok[:4])
        rows[(dim, p, nc)] = dict(doubles=doubles, differing=dict(zip(MEMBERS, (int(t) for t in tok[4:15]))),
                                  iw=int(tok[16]), untouched=int(tok[18]))
    return r.returncode, rows


def test_image_of_the_staged_shape_equals_the_lane_copy(report):
    _, rows = report
    row = rows[(3, 3, 0)]
    # x, w, iw, b0, b1: 4 each; D 16; xq, wq: 5 each; B 20; xv, wv: 4 each -- two rounds of a 64-lane block
    assert row["doubles"] == 74
    assert row["differing"] == dict.fromkeys(MEMBERS, 0)
    assert row["iw"] == 0  # iw == 1.0 / w, bit for bit
    assert row["untouched"] == 0  # the lanes wrote every word of the LDS copy: nothing was compared with poison


def test_every_built_shape(report):
    status, rows = report
    assert len(rows) == 16
    for key, row in rows.items():
        assert row["differing"] == dict.fromkeys(MEMBERS, 0) and row["iw"] == 0 and row["untouched"] == 0, (key, row)
    assert status == 0
