"""The operator owns its device memory (DevBuf members, device_buffer.hpp): ten create .. destroy cycles in one process, each
touching every buffer the operator creates at first use -- the host staging of tpsrhs_mult_host, the stage vectors and the NaN
counter of a step, the control block and the captured graph of tpsrhs_advance, the forcing block, the plane lists of a
mixed-out sponge, the buffers a failed tpsrhs_set_forcing lets go again -- leave the same state bit for bit as the first
cycle; a failed tpsrhs_set_forcing leaves the forcing in force; and the same under TPSRHS_POISON=1 in a fresh process.
The failed call: on the box the Mult after it equals the Mult before it bit for bit.  With a non-reflecting outlet no two
consecutive Mults are equal (each advances the boundary state), so there, and on the box as well, every second cycle leaves
the failing call out, and all ten cycles must agree: a cycle with the failed call in it computes what one without it does.
The drift of the free device memory between cycle 2 and cycle 10 is printed, not asserted: the card may be shared.
Second case: the loader of the kernel families (TPSRHS_FAMILY_PATH) skips a directory without the family and refuses a
shared object that is no family of this build.
Third case: the operator owns its post-processing state as well (statistics, samplers and probe records, the monitor, the
samplers tpsrhs_transfer caches on the source): four cycles of a destination and a source operator that use all of it and
are destroyed in either order read the same bytes, in this process and under TPSRHS_POISON=1 in a fresh one.  The drift
of the free device memory is printed as in the first case, which sets no bound on it (the card may be shared).

Run as a program (the child process of the poisoned cases) it prints the digest of the final state of each workload, or,
with the argument `observers`, the digest of the third case."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import numpy as np
import pytest

from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
CYCLES = 10


def _workload(kind):
    if kind == "box":  # 3 x 3 x 3 hexahedra at p = 2, dry air, Navier-Stokes, one isothermal wall (both x ends)
        mesh = meshgen.box_hex(3, 3, 3, lengths=(2.0, 1.0, 0.5), periodic=(False, True, True),
                               bdr_attr={(d, s): 3 for d in range(3) for s in (0, 1)})
        c = cases.Case("lifecycle_box", mesh, capi.Disc(2, 0, 0, 0, 0), capi.dry_air_physics(capi.NS),
                       [capi.make_bc(3, capi.WALL, capi.VISC_ISOTH, [300.0])])
    else:  # the cylinder with a non-reflecting outlet: boundary state, patch sums, the face lists
        c = cases.cyl3d(3, 8, 3, 2, capi.NS, capi.VISC_ISOTH)
        c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_P_NR, [101000.0, 0, 0, 0, 0.0, 0.0, 1.0, 0.0])
    return c, c.state(seed=7)


def _mixed_out_zone(**kw):
    z = dict(type=capi.SPONGE_PLANAR, solution_type=capi.SPONGE_MIXEDOUT, normal=(-1.0, 0.0, 0.0), point0=(1.9, 0.0, 0.0),
             point_init=(1.0, 0.0, 0.0), tol=0.06, mult_factor=2.0, target_U=[])
    z.update(kw)
    return z


def _cycle(kind, side, with_failing_call):
    """create .. destroy; returns the bytes of everything the cycle computed"""
    import ctypes as C

    import torch
    from tps_amd.rhs_operator import RHSoperator

    c, U = _workload(kind)
    out = []
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
        y = torch.empty_like(x)
        op.Mult(x, y)
        out.append(y.cpu().numpy().tobytes())
        xh, yh = np.ascontiguousarray(U).ravel().copy(), np.empty(U.size)
        st = op._lib.tpsrhs_mult_host(op._h, xh.ctypes.data_as(C.c_void_p), yh.ctypes.data_as(C.c_void_p), 0.0, None)
        assert st == 0, op._lib.tpsrhs_last_error()
        out.append(yh.tobytes())
        op.rk4_step(x, 0.0, 1e-9)
        op.advance(x, 1e-9, 1e-9, 4, True)  # control block, captured step graph
        op.setForcing(capi.make_forcing(heat_sources=[dict(value=1.0e5, radius=0.3, point1=(0.2, 0.5, 0.0), point2=(1.8, 0.5, 0.4))]))
        op.Mult(x, y)
        out.append(y.cpu().numpy().tobytes())
        # the plane x = 1: a layer of nodes of the box; around the cylinder a band wide enough to hold some
        op.setForcing(capi.make_forcing(sponge_zones=[_mixed_out_zone(tol=0.06 if kind == "box" else 0.5)]))
        op.Mult(x, y)
        before = y.cpu().numpy().tobytes()
        if with_failing_call:
            with pytest.raises(Exception, match="no node"):
                op.setForcing(capi.make_forcing(sponge_zones=[_mixed_out_zone(point_init=(1.013, 0, 0), tol=1e-6)]))
        op.Mult(x, y)  # the forcing of before the failed call, and its buffers, are still in force
        out += [before, y.cpu().numpy().tobytes()]
        if kind == "box":  # (no state from one Mult to the next)
            assert out[-1] == before
        op.setJouleHeating(torch.full((op.NDofs,), 3.0e4, dtype=torch.float64, device=op.device))  # nvel = 3: legal
        op.Mult(x, y)
        out.append(y.cpu().numpy().tobytes())
        out.append(x.cpu().numpy().tobytes())
        side.synchronize()
        op.close()
    for b in out:
        assert np.all(np.isfinite(np.frombuffer(b)))
    return b"".join(out)


def _ten_cycles(kind):
    """(digest of cycle 1, digest of cycle CYCLES, free-memory drift between the ends of cycle 2 and cycle CYCLES); the odd
    cycles hold the failing tpsrhs_set_forcing, the even ones do not"""
    import torch

    side = torch.cuda.Stream()  # one stream for all cycles: a new hardware queue's scratch arena is the runtime's to keep
    first = last = None
    free2 = 0
    for k in range(1, CYCLES + 1):
        last = hashlib.sha256(_cycle(kind, side, with_failing_call=k % 2 == 1)).hexdigest()
        first = first or last
        assert last == first, f"cycle {k} ({'with' if k % 2 else 'without'} the failing call) differs from cycle 1"
        if k == 2:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free2 = torch.cuda.mem_get_info()[0]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    drift = free2 - torch.cuda.mem_get_info()[0]
    print(f"lifecycle {kind}: digest {last} free-memory drift cycle 2 -> {CYCLES}: {drift} bytes")
    return first, last, drift


@pytest.mark.parametrize("kind", ["box", "cylinder_nr"])
def test_ten_cycles_leave_the_same_state(kind):
    first, last, _ = _ten_cycles(kind)
    assert first == last


def test_ten_cycles_with_poisoned_allocations():
    """TPSRHS_POISON=1 in a fresh process: every buffer starts as NaN, whatever an earlier cycle left in the allocator"""
    env = dict(os.environ, TPSRHS_POISON="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("LIFECYCLE SAME") == 2


def _observers_cycle(side, destination_first):
    """two operators, every kind of post-processing state on them, three steps; returns the bytes of everything read"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    def box(order):  # 2 x 2 x 2 hexahedra, dry air, Navier-Stokes, isothermal walls all round
        mesh = meshgen.box_hex(2, 2, 2, periodic=(False, False, False), bdr_attr={(d, e): 3 for d in range(3) for e in (0, 1)})
        return cases.Case(f"observers_p{order}", mesh, capi.Disc(order, 0, 0, 0, 0), capi.dry_air_physics(capi.NS),
                          [capi.make_bc(3, capi.WALL, capi.VISC_ISOTH, [300.0])])

    out = []
    with torch.cuda.stream(side):
        cd, cs = box(1), box(2)
        dst = RHSoperator(cd.mesh, cd.disc, cd.physics, cd.bcs, stream=side)
        src = RHSoperator(cs.mesh, cs.disc, cs.physics, cs.bcs, stream=side)
        x = torch.tensor(np.ascontiguousarray(cd.state(seed=7)).ravel(), dtype=torch.float64, device=dst.device)
        xs = torch.tensor(np.ascontiguousarray(cs.state(seed=8)).ravel(), dtype=torch.float64, device=src.device)
        dst.configureStatistics(1, 0, variances=True)
        dst.configureStatistics(1, 0, variances=True)  # reconfigured: the first state goes, with its fields
        pts = np.array([[0.3, 0.7, 2.0], [0.2, 0.6, 2.0], [0.4, 0.9, 2.0]])  # (dim, npts): the third lies outside the box
        sampler = dst.createSampler(pts, fill=-1.0)
        dst.configureProbes(sampler, 1, 2)  # three steps into two rows: the third record is dropped
        dst.configureMonitor(1, 4)
        moved, missing = dst.transferFrom(src, xs)  # locates the p = 1 nodes in the p = 2 operator and keeps the sampler there
        assert missing == 0 and src.transferStats() == (1, 0)
        out.append(moved.cpu().numpy().tobytes())
        time, dt, bad = dst.advance(x, 0.0, 1e-9, 3, True, integrator="forwardEuler")
        assert bad == 0
        mean, vari, ns_mean, ns_vari, it = dst.getStatistics()
        assert (ns_mean, ns_vari, it) == (3, 3, 3)
        out += [mean.cpu().numpy().tobytes(), vari.cpu().numpy().tobytes()]
        elem, ref, nfound = sampler.info()
        assert nfound == 2 and elem[2] == -1
        out += [elem.tobytes(), ref.tobytes(), sampler.sample(x).cpu().numpy().tobytes()]
        iters, times, values, ndropped = dst.readProbes()
        assert list(iters) == [1, 2] and ndropped == 1
        out += [times.tobytes(), values.tobytes()]
        mon = dst.readMonitor()
        assert list(mon["iters"]) == [1, 2, 3] and mon["ndropped"] == 0
        out += [mon[k].tobytes() for k in ("times", "dts", "totals", "mins", "maxs")]
        out += [x.cpu().numpy().tobytes(), np.array([time, dt]).tobytes()]
        side.synchronize()
        for op in ((dst, src) if destination_first else (src, dst)):
            op.close()
    for b in out[:3] + out[4:]:  # (out[3]: the elements, integers)
        assert np.all(np.isfinite(np.frombuffer(b)))
    return b"".join(out)


OBSERVER_CYCLES = 4


def _observer_cycles():
    """the one digest of OBSERVER_CYCLES cycles; the odd cycles destroy the destination first, the even ones the source"""
    import torch

    side = torch.cuda.Stream()
    first, free1 = None, 0
    for k in range(1, OBSERVER_CYCLES + 1):
        digest = hashlib.sha256(_observers_cycle(side, destination_first=k % 2 == 1)).hexdigest()
        first = first or digest
        assert digest == first, f"cycle {k} differs from cycle 1"
        if k == 1:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free1 = torch.cuda.mem_get_info()[0]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"lifecycle observers: digest {first} free-memory drift cycle 1 -> {OBSERVER_CYCLES}: {free1 - torch.cuda.mem_get_info()[0]} bytes")
    return first


def test_post_processing_state_goes_with_its_operator_in_either_order():
    digest = _observer_cycles()
    env = dict(os.environ, TPSRHS_POISON="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "observers"], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"OBSERVERS {digest}" in r.stdout


def _family_case(stranger, empty):
    """in a process that has loaded no kernel family yet (a loaded one is kept, and the search is not repeated)"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    mesh = meshgen.box_quad(3, 3)
    ph = capi.argon_ternary_physics(capi.NS, True, capi.CONSTANT, None)
    disc = capi.Disc(2, 0, 0, 0, 0)
    os.environ["TPSRHS_FAMILY_PATH"] = stranger
    lib = capi.load()
    try:
        RHSoperator(mesh, disc, ph, [])
        sys.exit("a shared object that is no kernel family was accepted")
    except RuntimeError as e:
        assert getattr(e, "status", None) == 2, e  # TPSRHS_ERR_UNSUPPORTED
        assert b"built against another operator layout" in lib.tpsrhs_last_error(), e
    os.environ["TPSRHS_FAMILY_PATH"] = empty
    op = RHSoperator(mesh, disc, ph, [])  # nothing there: the family next to the library is loaded
    x = torch.tensor(cases.Case("family", mesh, disc, ph, []).state(seed=1, amp=0.01).ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    op.Mult(x, y)
    assert bool(torch.isfinite(y).all())
    op.close()
    print("FAMILY OK")


def test_family_path_is_searched_and_strangers_are_refused(tmp_path):
    unit = "plasma_2d_n3a"  # the planar 2-D ambipolar ternary mixture at p = 2
    stranger, empty = tmp_path / "stranger", tmp_path / "empty"
    stranger.mkdir()
    empty.mkdir()
    (tmp_path / "empty.cpp").write_text("")
    subprocess.run(["g++", "-shared", "-fPIC", str(tmp_path / "empty.cpp"), "-o", str(stranger / f"libtpsrhs_{unit}.so")], check=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "family", str(stranger), str(empty)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "FAMILY OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    if sys.argv[1:2] == ["family"]:
        _family_case(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if sys.argv[1:2] == ["observers"]:
        print("OBSERVERS", _observer_cycles())
        sys.exit(0)
    for kind in ("box", "cylinder_nr"):
        first, last, _ = _ten_cycles(kind)
        if first != last:
            sys.exit(f"lifecycle {kind}: cycle {CYCLES} differs from cycle 1")
        print("LIFECYCLE SAME", kind)
