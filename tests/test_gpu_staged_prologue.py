"""The staged prologue of the 3-D p = 3 sweeps (kernels.hpp::stage_issue / stage_store) moves the same words to the same places
of LDS as the three loaders it replaces (load_face_info, load_tables, load_vertices), 1 / w now divided on the host: no
result may move by a bit.  This test builds the metric's kernel family, and the core library for dry air, once more with
-DTPSRHS_STAGED_PROLOGUE=0 (tools/build_variant.sh, tools/build_core_variant.sh; minutes of hipcc, kept under
tps_amd/csrc/_ab/ until a header changes), runs the same seeded case in two child processes -- the regular libraries, and
the variant found through TPSRHS_FAMILY_PATH / TPSRHS_LIB -- and compares one Mult (y, Up, gradUp) and the state after two
RK4 steps byte by byte.  The case is the cylinder at p = 3 with a viscous isothermal wall and scrambled orientations: 99
hexes, one per block, interior, wall, inlet and outlet faces."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tps_amd", "csrc")
AB = os.path.join(CSRC, "_ab")
FLAG = "-DTPSRHS_STAGED_PROLOGUE=0"
pytestmark = pytest.mark.gpu

CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import torch
from parity_util import hip_mult
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import RHSoperator
if sys.argv[2] == "argon":
    c = cases.argon_cyl3d(3, 11, 3, 3, wall_type=capi.VISC_ISOTH)
    U = c.state(seed=21, amp=0.01)
else:
    c = cases.cyl3d(3, 11, 3, 3, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    U = c.state(seed=21)
c.mesh = meshgen.scramble_orientations(c.mesh, 5)
got = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U)
assert np.all(np.isfinite(got["y"]))
# a stable explicit step: a tenth of the fastest local time scale of the residual
dt = 0.1 / (np.abs(got["y"]) / np.maximum(np.abs(U), 1e-300 + 1e-6 * np.abs(U).max(axis=1, keepdims=True))).max()
op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
t = 0.0
for _ in range(2):
    t = op.rk4_step(x, t, dt)
torch.cuda.synchronize()
rk4 = x.cpu().numpy().reshape(U.shape)
op.close()
assert np.all(np.isfinite(rk4))
np.savez(sys.argv[1], y=got["y"], Up=got["Up"], gradUp=got["gradUp"], dt=np.float64(dt), rk4=rk4)
"""


def _stale(lib, unit):
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, unit + ".hip")]
    return not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs)


def _family_variant():
    lib = os.path.join(AB, "unstaged", "libtpsrhs_plasma_3d_n3a.so")
    if _stale(lib, "plasma_3d_n3a"):
        subprocess.run([os.path.join(ROOT, "tools", "build_variant.sh"), "unstaged", FLAG + " -mllvm -disable-machine-licm",
                        "plasma_3d_n3a"], check=True, timeout=900)
    return lib


def _core_variant():
    lib = os.path.join(AB, "unstaged_core", "libtpsrhs.so")
    if _stale(lib, "tpsrhs"):
        subprocess.run([os.path.join(ROOT, "tools", "build_core_variant.sh"), "unstaged_core", FLAG], check=True, timeout=900)
    return lib


def _run(tmp_path, tag, kind, **env_over):
    out = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ)
    for k in ("TPSRHS_FAMILY_PATH", "TPSRHS_LIB"):
        env.pop(k, None)
    env.update(env_over)
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", code, out, kind], check=True, env=env, timeout=300)
    return np.load(out)


def _same_bytes(staged, loaders):
    for k in ("Up", "gradUp", "y", "dt", "rk4"):
        a, b = staged[k], loaders[k]
        assert a.shape == b.shape
        diff = np.abs(a - b).max()
        print(k, a.shape, "max |difference|", diff)
        assert a.tobytes() == b.tobytes(), f"{k}: staged prologue and loaders differ, max |difference| {diff}"


def test_reacting_sweeps_do_not_move_by_a_bit(tmp_path):
    lib = _family_variant()
    _same_bytes(_run(tmp_path, "staged", "argon"), _run(tmp_path, "loaders", "argon", TPSRHS_FAMILY_PATH=os.path.dirname(lib)))


def test_dry_air_sweeps_do_not_move_by_a_bit(tmp_path):
    lib = _core_variant()
    _same_bytes(_run(tmp_path, "staged", "dry"), _run(tmp_path, "loaders", "dry", TPSRHS_LIB=lib, TPSRHS_FAMILY_PATH=CSRC))
