"""Monitor records inside the device time loop (tpsrhs_monitor_configure / tpsrhs_monitor_read): every record holds the
right iteration, the device-side time and next dt, and the integrals and extrema of exactly the state reached after that
many steps; the loop's solution is untouched; the buffer never overflows; two-step graphs split as for the probes; the
totals drift no more than the CPU oracle's own time loop lets them; the axisymmetric totals carry the radial weight."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import integrals_util as iu
from tps_amd import capi, cases, mesh_io
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
EPS = iu.EPS
CUBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "periodic-cube.mesh")
DT = 2.0e-5


@functools.lru_cache(maxsize=None)
def _cube():
    """periodic-cube.mesh, Euler, p = 2, Gauss-Legendre: (mesh, disc, physics, bcs, U)"""
    m = mesh_io.read_mfem_mesh(CUBE)
    U = cases.dry_air_state(node_coordinates(m, 2), seed=3)
    U.setflags(write=False)
    return m, capi.Disc(2, 0, 0, 0, 0), capi.dry_air_physics(capi.EULER), [], U


@functools.lru_cache(maxsize=None)
def _cylinder(nr_outlet):
    c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    if nr_outlet:  # a non-reflecting outlet: its boundary state swaps once per Mult
        c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_P_NR, [101000.0, 0, 0, 0, 0.0, 0.0, 1.0, 0.0])
    U = c.state(seed=2)
    U.setflags(write=False)
    return c.mesh, c.disc, c.physics, c.bcs, U


def _run(setup, calls, integrator=capi.RK4, monitor=None, variable=False, env=None, monkeypatch=None, dt0=DT):
    """One operator and one x on a capturable side stream; calls: the steps of each advance call.
    -> dict(x, end=[(time, dt, census) per call], records, totals / mins / maxs of the final x by the direct calls)"""
    import torch

    from tps_amd.rhs_operator import RHSoperator

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    mesh, disc, ph, bcs, U = setup
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = RHSoperator(mesh, disc, ph, bcs, stream=side)
        if monitor is not None:
            op.configureMonitor(*monitor)
        x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
        t, dt, ends = 0.0, dt0, []
        for n in calls:
            t, dt, bad = op.advance(x, t, dt, n, not variable, 0.12 if variable else 0.0, 0.05 if variable else 0.0,
                                    integrator=integrator)
            ends.append((t, dt, bad))
        out = dict(x=x.cpu().numpy(), end=ends, records=op.readMonitor() if monitor is not None else None,
                   totals=op.integrate(x)[0].cpu().numpy())
        out["mins"], out["maxs"], _ = (a.cpu().numpy() for a in op.nodalStats(x))
        side.synchronize()
        op.close()
    return out


# ---- 1. constant step --------------------------------------------------------------------------------------------------------
def test_constant_step_records():
    """12 RK4 steps, interval 3, capacity 3: records after 3, 6, 9 steps, the one after 12 is dropped"""
    on = _run(_cube(), [12], monitor=(3, 3))
    off = _run(_cube(), [12])
    r = on["records"]
    assert list(r["iters"]) == [3, 6, 9] and r["ndropped"] == 1
    assert np.isfinite(on["x"]).all() and on["end"][0][2] == 0
    assert np.array_equal(on["x"], off["x"]) and on["end"] == off["end"]  # the monitor leaves the solution alone
    assert (r["dts"] == DT).all()
    t = 0.0
    for k in range(3):
        for _ in range(3):
            t += DT
        assert abs(r["times"][k] - t) <= 4 * EPS * t, (k, r["times"][k], t)
        ref = _run(_cube(), [3 * (k + 1)])  # a separate run of exactly that many steps
        assert r["times"][k] == ref["end"][0][0]
        for name in ("totals", "mins", "maxs"):
            assert np.array_equal(r[name][k], ref[name]), (name, k, r[name][k], ref[name])


# ---- 2. conservation ---------------------------------------------------------------------------------------------------------
def test_totals_drift_like_the_oracle():
    """The drift of the totals over 9 steps, measured against the CPU oracle: the same 9 RK4 steps with the oracle
    (tests/integrators_util.py), integrated by the restatement, give drift_oracle; per equation the device's drift may be
    16 max(drift_oracle, K eps S1) -- the factor 16 is the margin for FMA contraction and another face-summation order."""
    import integrators_util as ti
    from oracle_lib import Oracle

    mesh, disc, ph, bcs, U = _cube()
    on = _run(_cube(), [9], monitor=(9, 1))
    start = _run(_cube(), [0])
    assert list(on["records"]["iters"]) == [9]
    drift_device = np.abs(on["records"]["totals"][0] - start["totals"])
    o = Oracle(mesh, disc, ph, threads=8)
    x9, _, _, bad = ti.advance(o, capi.RK4, np.array(U), 0.0, DT, 9)
    assert bad == 0
    before, after = iu.integrate(mesh, 2, 0, U), iu.integrate(mesh, 2, 0, x9)
    drift_oracle = np.abs(after["sum"] - before["sum"])
    floor = before["K"] * EPS * before["S1"]
    print("totals               :", start["totals"])
    print("drift, device        :", drift_device)
    print("drift, oracle        :", drift_oracle)
    print("K eps S1             :", floor)
    print("drift / (eps S1), dev:", drift_device / (EPS * before["S1"]), " oracle:", drift_oracle / (EPS * before["S1"]))
    iu.check("initial totals", start["totals"], np.zeros(5), dict(before, sumsq=np.zeros(5)))
    assert (drift_device <= 16 * np.maximum(drift_oracle, floor)).all()


# ---- 3. variable step --------------------------------------------------------------------------------------------------------
def test_variable_step_history():
    """6 steps of the Navier-Stokes cylinder with dt from the CFL condition, a record after every step: the recorded dt and
    time are those six one-step calls return, bit for bit"""
    one = _run(_cylinder(False), [6], monitor=(1, 8), variable=True)
    six = _run(_cylinder(False), [1] * 6, variable=True)
    r = one["records"]
    assert list(r["iters"]) == [1, 2, 3, 4, 5, 6] and r["ndropped"] == 0
    assert np.array_equal(r["dts"], [e[1] for e in six["end"]])
    assert np.array_equal(r["times"], [e[0] for e in six["end"]])
    assert len(set(r["dts"])) == 6  # the step does vary
    assert np.array_equal(one["x"], six["x"])
    assert np.array_equal(r["totals"][5], one["totals"]) and np.array_equal(r["mins"][5], one["mins"])


# ---- 4. two-step graphs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK3_SSP], ids=["forwardEuler", "rk3"])
def test_two_step_graphs_split_for_a_record(monkeypatch, integrator):
    """a non-reflecting outlet and an odd number of Mults per step: the graph holds two steps (the first step runs alone, then
    the pairs 2-3, 4-5, 6-7, 8-9), and with interval 3 the record after step 6 falls between the steps of a pair, which then
    runs as two plain steps; the records after steps 3 and 9 follow a replayed pair"""
    graph = _run(_cylinder(True), [10], integrator, monitor=(3, 4), variable=True, env={"TPSRHS_GRAPH": "1"}, monkeypatch=monkeypatch)
    loop = _run(_cylinder(True), [10], integrator, monitor=(3, 4), variable=True, env={"TPSRHS_GRAPH": "0"}, monkeypatch=monkeypatch)
    off = _run(_cylinder(True), [10], integrator, variable=True, env={"TPSRHS_GRAPH": "1"}, monkeypatch=monkeypatch)
    assert list(graph["records"]["iters"]) == [3, 6, 9] and graph["records"]["ndropped"] == 0
    for name in ("iters", "times", "dts", "totals", "mins", "maxs"):
        assert np.array_equal(graph["records"][name], loop["records"][name]), name
    assert np.isfinite(graph["x"]).all()
    assert np.array_equal(graph["x"], loop["x"]) and np.array_equal(graph["x"], off["x"]) and graph["end"] == loop["end"] == off["end"]


# ---- 5. axisymmetric totals -----------------------------------------------------------------------------------------------
def test_axisymmetric_totals_carry_the_radial_weight():
    c = cases.dry_air_axisym(3, 5, 3)
    U = c.state(seed=6)
    r = _run((c.mesh, c.disc, c.physics, c.bcs, U), [2], monitor=(2, 1), dt0=1.0e-6)
    assert list(r["records"]["iters"]) == [2]
    x = r["x"].reshape(5, -1)
    ref = iu.integrate(c.mesh, 3, 0, x, radial=True)
    plain = iu.integrate(c.mesh, 3, 0, x, radial=False)
    iu.check("axisymmetric totals", r["records"]["totals"][0], np.zeros(5), dict(ref, sumsq=np.zeros(5)))
    assert np.array_equal(r["records"]["totals"][0], r["totals"])  # RHSoperator.integrate defaults to the same flag
    assert (np.abs(ref["sum"] - plain["sum"]) > 0.5 * np.abs(ref["sum"])).all()  # (the two weights are far apart)
    assert np.array_equal(r["records"]["mins"][0], x.min(axis=1)) and np.array_equal(r["records"]["maxs"][0], x.max(axis=1))


# ---- 6. reset, reconfigure, off, destroy -------------------------------------------------------------------------------------
def test_reset_reconfigure_off_and_destroy():
    import torch

    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    lib = capi.load()
    mesh, disc, ph, bcs, U = _cube()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = RHSoperator(mesh, disc, ph, bcs, stream=side)
        bad = capi.ERR_INVALID_ARGUMENT
        for args in ((-1, 4), (1, -4), (1, 0)):
            assert lib.tpsrhs_monitor_configure(op._h, *args) == bad
        assert lib.tpsrhs_monitor_configure(None, 1, 4) == bad
        assert lib.tpsrhs_monitor_read(op._h, None, None, None, None, None, None, None, None, 0) == bad  # not configured
        assert "not configured" in lib.tpsrhs_last_error().decode()
        assert lib.tpsrhs_monitor_read(None, None, None, None, None, None, None, None, None, 0) == bad
        op.configureMonitor(2, 3)
        x = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
        t, dt, _ = op.advance(x, 0.0, DT, 5, True)
        assert lib.tpsrhs_monitor_read(op._h, None, None, None, None, None, None, None, None, 0) == 0  # every pointer may be NULL
        first = op.readMonitor(reset=True)
        assert list(first["iters"]) == [2, 4] and first["ndropped"] == 0
        again = op.readMonitor()
        assert len(again["iters"]) == 0 and again["totals"].shape == (0, 5) and again["ndropped"] == 0
        t, dt, _ = op.advance(x, t, dt, 5, True)  # the step counter went on: 6, 8, 10
        later = op.readMonitor()
        assert list(later["iters"]) == [6, 8, 10] and later["ndropped"] == 0
        assert np.array_equal(later["totals"][2], op.integrate(x)[0].cpu().numpy())
        # a full buffer: nothing is written past the end (guard regions behind the capacity of 3 records)
        t, dt, _ = op.advance(x, t, dt, 4, True)
        guard = 16
        tot = np.full(3 * 5 + guard, 12345.0)
        its, tms = np.full(3 + guard, -77, dtype=np.int64), np.full(3 + guard, 12345.0)
        nrec, ndrop = C.c_int64(0), C.c_int64(0)
        assert lib.tpsrhs_monitor_read(op._h, C.byref(nrec), C.byref(ndrop), its.ctypes.data, tms.ctypes.data, None,
                                       tot.ctypes.data, None, None, 0) == 0
        assert (nrec.value, ndrop.value) == (3, 2)
        assert np.array_equal(tot[:15].reshape(3, 5), later["totals"]) and (tot[15:] == 12345.0).all()
        assert list(its[:3]) == [6, 8, 10] and (its[3:] == -77).all() and (tms[3:] == 12345.0).all()
        # tpsrhs_step neither counts nor records
        op.readMonitor(reset=True)
        op.step(x, t, dt, "rk4")
        assert len(op.readMonitor()["iters"]) == 0
        # reconfigure: the counter starts again, the buffer has the new capacity
        op.configureMonitor(1, 2)
        t, dt, _ = op.advance(x, t, dt, 3, True)
        rec = op.readMonitor()
        assert list(rec["iters"]) == [1, 2] and rec["ndropped"] == 1
        # off
        op.configureMonitor(0, 0)
        with pytest.raises(TpsRhsError) as e:
            op.readMonitor()
        assert e.value.status == bad
        before = x.clone()
        op.advance(x, t, dt, 3, True)  # the loop of an operator without a monitor is the loop it was
        assert not torch.equal(before, x)
        # destroy with the monitor on and records held
        op.configureMonitor(1, 4)
        op.advance(x, t, dt, 3, True)
        side.synchronize()
        op.close()
