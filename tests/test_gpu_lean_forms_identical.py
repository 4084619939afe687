"""The one-hex form of the lean 3-D face kernel (kernels.hpp::visc_phase_lean1) claims the SAME floating-point operations in
the same order as the general form (visc_phase_lean3d): only the integer work around them differs.  This test pins that claim
bit for bit.  It builds the metric's kernel family once more with -DTPSRHS_LEAN_GENERAL=1 (the general form everywhere;
tools/build_variant.sh, two minutes of hipcc, kept under tps_amd/csrc/_ab/ until a header changes), runs one Mult of the same
seeded case in two child processes -- the regular family library, and the variant found through TPSRHS_FAMILY_PATH -- and
compares y, Up and gradUp byte by byte.  The case is the argon cylinder at p = 3 with a viscous isothermal wall: interior faces,
wall faces (two passes of the face kernel), inlet and outlet faces, scrambled orientations."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tps_amd", "csrc")
VARIANT = os.path.join(CSRC, "_ab", "lean_general")
UNIT = "plasma_3d_n3a"
pytestmark = pytest.mark.gpu

CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
from parity_util import hip_mult
from tps_amd import capi, cases, meshgen
c = cases.argon_cyl3d(3, 11, 3, 3, wall_type=capi.VISC_ISOTH)
c.mesh = meshgen.scramble_orientations(c.mesh, 5)
got = hip_mult(c.mesh, c.disc, c.physics, c.bcs, c.state(seed=21, amp=0.01))
assert np.all(np.isfinite(got["y"]))
np.savez(sys.argv[1], y=got["y"], Up=got["Up"], gradUp=got["gradUp"])
"""


def _variant_library():
    lib = os.path.join(VARIANT, f"libtpsrhs_{UNIT}.so")
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, UNIT + ".hip")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        subprocess.run([os.path.join(ROOT, "tools", "build_variant.sh"), "lean_general",
                        "-DTPSRHS_LEAN_GENERAL=1 -mllvm -disable-machine-licm", UNIT], check=True, timeout=900)
    return lib


def _mult(tmp_path, tag, family_path):
    out = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    env.pop("TPSRHS_FAMILY_PATH", None)
    if family_path:
        env["TPSRHS_FAMILY_PATH"] = family_path
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code, out], check=True, env=env, timeout=300)
    return np.load(out)


def test_one_hex_form_equals_general_form_bit_for_bit(tmp_path):
    lib = _variant_library()
    one_hex = _mult(tmp_path, "one_hex", "")
    general = _mult(tmp_path, "general", os.path.dirname(lib))
    for k in ("Up", "gradUp", "y"):
        a, b = one_hex[k], general[k]
        assert a.shape == b.shape
        diff = np.abs(a - b).max()
        print(k, a.shape, "max |difference|", diff)
        assert a.tobytes() == b.tobytes(), f"{k}: the two forms differ, max |difference| {diff}"
