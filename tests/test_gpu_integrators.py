"""Forward Euler, RK2 and RK3-SSP in the device time loop (tpsrhs_step, tpsrhs_advance_with) against the numpy
restatement of tests/integrators_util.py, which tests/test_integrators_oracle.py pins on the CPU.

Cases, step sizes and tolerances are those of the RK4 tests in test_gpu_rk4.py, named at each test."""
import ctypes as C

import numpy as np
import pytest

import integrators_util as iu
from oracle_lib import Oracle
from parity_util import rel_maxnorm
from tps_amd import capi, cases

pytestmark = pytest.mark.gpu

NEW = [capi.FORWARD_EULER, capi.RK2, capi.RK3_SSP]
_name = lambda i: iu.NAMES[i]  # noqa: E731
_REF = {}  # restatement runs, computed once and shared


def _device_state(op, U):
    import torch

    return torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)


def _steps(c, U, integrator, dt, nsteps):
    import torch
    from tps_amd.rhs_operator import RHSoperator

    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = _device_state(op, U)
    t = 0.0
    for _ in range(nsteps):
        t = op.step(x, t, dt, integrator, want_max_char_speed=True, want_nan_count=True)
    torch.cuda.synchronize()
    out = x.cpu().numpy().reshape(U.shape), t, op.max_char_speed, op.nan_count
    op.close()
    return out


def _rowmax(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def _assert_step_parity(got, ref, U, what, rel_bound=1e-13):
    """the assertions of test_rk4_steps_match_oracle on the state"""
    incr, err = _rowmax(ref - U), _rowmax(got - ref)
    print(what, "increment", incr, "difference", err, "rel_maxnorm", rel_maxnorm(got, ref).max())
    assert (err <= 1e-9 * incr + 1e-15 * _rowmax(U)).all()
    assert rel_maxnorm(got, ref).max() < rel_bound


def _dry_air_case():
    c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    return c, c.state(seed=2)


def _stable_dt(o, U):
    """as test_rk4_steps_match_oracle: a tenth of the fastest local time scale of the residual"""
    y0 = o.mult(U)
    return 0.1 / (np.abs(y0) / np.maximum(np.abs(U), 1e-300 + 1e-6 * np.abs(U).max(axis=1, keepdims=True))).max()


# ---- 1. steps match the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dry_air", "argon_2T"])
@pytest.mark.parametrize("integrator", NEW, ids=_name)
def test_steps_match_restatement(integrator, kind):
    if kind == "dry_air":
        c, U = _dry_air_case()
    else:
        c = cases.argon_cyl3d(4, 12, 3, 2, True, capi.CONSTANT, "arrhenius", capi.VISC_ISOTH)
        U = c.state(seed=2, amp=0.01)
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
    if ("dt", kind) not in _REF:
        _REF["dt", kind] = _stable_dt(o, U)
    dt, nsteps = _REF["dt", kind], 3
    ref, t = U.copy(), 0.0
    for _ in range(nsteps):
        ref, t, speed, bad = iu.step(o, integrator, ref, t, dt)
    got, tg, gspeed, gbad = _steps(c, U, integrator, dt, nsteps)
    assert tg == pytest.approx(t, rel=1e-15) and gbad == bad == 0
    _assert_step_parity(got, ref, U, f"{iu.NAMES[integrator]} {kind}:")
    assert gspeed == pytest.approx(speed, rel=1e-12)


# ---- 2. RK4 through the new entries is the old path ---------------------------------------------------------------------
def test_rk4_through_the_new_entries_is_the_old_path():
    import torch
    from tps_amd.rhs_operator import RHSoperator

    c, U = _dry_air_case()
    dt0, cfl, hmin, nsteps = 2.0e-5, 0.12, 0.05, 4
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)

    def stepped(new_entry):
        x, t = _device_state(op, U), 0.0
        for _ in range(nsteps):
            if new_entry:
                t = op.step(x, t, dt0, "rk4", want_max_char_speed=True, want_nan_count=True)
            else:
                t = op.rk4_step(x, t, dt0, want_max_char_speed=True, want_nan_count=True)
        torch.cuda.synchronize()
        return x.cpu().numpy(), (t, op.max_char_speed, op.nan_count)

    (xa, sa), (xb, sb) = stepped(False), stepped(True)
    assert np.array_equal(xa, xb) and sa == sb and sa[2] == 0

    def advanced(how, constant_dt):
        x = _device_state(op, U)
        if how == "tpsrhs_advance":
            out = op.advance(x, 0.0, dt0, nsteps, constant_dt, cfl, hmin)
        elif how == "keyword":
            out = op.advance(x, 0.0, dt0, nsteps, constant_dt, cfl, hmin, integrator="rk4")
        else:  # tpsrhs_advance_with itself, with TPSRHS_RK4
            t, d, bad = C.c_double(0.0), C.c_double(dt0), C.c_int64(0)
            st = capi.load().tpsrhs_advance_with(op._h, capi.RK4, C.c_void_p(x.data_ptr()), C.byref(t), C.byref(d), nsteps,
                                                 1 if constant_dt else 0, cfl, hmin, C.byref(bad))
            assert st == 0
            out = (t.value, d.value, bad.value)
        return x.cpu().numpy(), out

    for constant_dt in (True, False):
        xa, sa = advanced("tpsrhs_advance", constant_dt)
        for how in ("keyword", "tpsrhs_advance_with"):
            xb, sb = advanced(how, constant_dt)
            assert np.array_equal(xa, xb) and sa == sb, (how, constant_dt)
        assert sa[2] == 0 and (sa[1] == dt0) == constant_dt
    op.close()


# ---- 3. clamp and census on the final state only ------------------------------------------------------------------------
def _ternary_case():
    """the case of test_rk4_counts_nans_and_clamps_species"""
    c = cases.argon_cyl3d(4, 12, 3, 1, False, capi.CONSTANT, None, capi.VISC_ISOTH)
    return c, c.state(seed=3, amp=0.005)


# This step is a hundred times the stable one (9.0e-4 s against ~1e-5 s): it moves the momentum rows by as much as they
# hold, so the difference between the device's and the oracle's Mult (relative 3e-13 of the residual, far inside the
# one-Mult parity bound) reaches the state undamped: rel_maxnorm 2.88e-13, where the stable steps of the RK4 test and of
# test_steps_match_restatement leave 1e-15 (RK4: 1.3e-15 dry air, 9.5e-16 argon).  The bound relative to the INCREMENT
# (1e-9 incr + 1e-15 max|U|) holds as it stands.  Set as the issue of this feature prescribes for a bound the device
# cannot meet: 4 x the larger of the RK4 test's observed error and this one's.
CLAMP_STEP_REL_BOUND = 4 * 2.88e-13


def test_euler_clamps_the_final_state():
    c, U = _ternary_case()
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
    rows = iu.species_rows(o)
    assert rows.stop > rows.start
    f = o.mult(U)
    us, fs = U[rows], f[rows]
    dt = 1.5 * (us[fs < 0] / -fs[fs < 0]).min()
    unclamped, _, _, _ = iu.step(o, capi.FORWARD_EULER, U, 0.0, dt, clamp=False)
    assert unclamped[rows].min() < 0.0  # without Check_Undershoot a species entry goes negative
    ref, t, speed, bad = iu.step(o, capi.FORWARD_EULER, U, 0.0, dt)
    got, tg, gspeed, gbad = _steps(c, U, capi.FORWARD_EULER, dt, 1)
    print("dt", dt, "species entries at 0: device", int((got[rows] == 0.0).sum()), "restatement", int((ref[rows] == 0.0).sum()))
    assert tg == pytest.approx(t, rel=1e-15) and gbad == bad == 0
    _assert_step_parity(got, ref, U, "forwardEuler ternary:", rel_bound=CLAMP_STEP_REL_BOUND)
    assert gspeed == pytest.approx(speed, rel=1e-12)
    assert (got[rows] >= 0.0).all() and (got[rows] == 0.0).any()


@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK3_SSP], ids=_name)
def test_census_before_clamp_with_a_nan(integrator):
    """test_rk4_counts_nans_and_clamps_species for the schemes whose last stage is the first / the third pass"""
    c, U = _ternary_case()
    U[0, 5] = np.nan  # one bad density entry poisons its element
    got, _, _, bad = _steps(c, U, integrator, 1e-9, 1)
    # the census (Check_NAN) runs before the clamp (Check_Undershoot), and max(NaN, 0) = 0 in the species rows
    assert bad >= np.isnan(got).sum() > 0
    assert not np.isnan(got[5]).any() and np.isnan(got[:5]).sum() == np.isnan(got).sum()


# ---- 4. the loop on the device, variable and constant dt ----------------------------------------------------------------
def _nr_outlet_case(order):
    c = cases.cyl3d(4, 12, 3, order, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    # a non-reflecting outlet on top: its boundary state integrates with the device-side dt too
    c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_P_NR, [101000.0, 0, 0, 0, 0.0, 0.0, 1.0, 0.0])
    return c, c.state(seed=2)


@pytest.mark.parametrize("constant_dt", [True, False])
@pytest.mark.parametrize("integrator", NEW, ids=_name)
def test_advance_keeps_the_time_loop_on_the_device(integrator, constant_dt):
    """the case and the assertions of test_gpu_rk4.test_advance_keeps_the_time_loop_on_the_device"""
    from tps_amd.rhs_operator import RHSoperator

    c, U = _nr_outlet_case(2)
    dt0, cfl, hmin, nsteps = 2.0e-5, 0.12, 0.05, 4
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)  # (a fresh one: it holds the boundary state of the outlet)
    ref, t, dt, bad = iu.advance(o, integrator, U, 0.0, dt0, nsteps, constant_dt, cfl, hmin)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = _device_state(op, U)
    tg, dtg, gbad = op.advance(x, 0.0, dt0, nsteps, constant_dt, cfl, hmin, integrator=integrator)
    got = x.cpu().numpy().reshape(U.shape)
    op.close()
    print(iu.NAMES[integrator], "time", tg, t, "next dt", dtg, dt, "rel_maxnorm", rel_maxnorm(got, ref).max())
    assert gbad == bad == 0
    assert tg == pytest.approx(t, rel=1e-13) and dtg == pytest.approx(dt, rel=1e-12)
    assert (dtg == dt0) == constant_dt
    assert rel_maxnorm(got, ref).max() < 1e-13


# ---- 5. graph replay equals the launch loop, and the key knows the scheme -----------------------------------------------
FORCING = capi.make_forcing(pressure_gradient=(2.0, 0.0, -1.0))


def _on_side_stream(monkeypatch, graph, c, U, forcing, calls, dt0, cfl, hmin):
    """`calls` = [(integrator, steps)] on ONE operator and ONE x, on a capturable side stream, variable dt; per call the
    state and (time, dt, census)"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    monkeypatch.setenv("TPSRHS_GRAPH", graph)
    side = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        if forcing is not None:
            op.setForcing(forcing)
        x = _device_state(op, U)
        t, dt = 0.0, dt0
        for integrator, nsteps in calls:
            t, dt, bad = op.advance(x, t, dt, nsteps, False, cfl, hmin, integrator=integrator)
            out.append((x.cpu().numpy().reshape(U.shape), (t, dt, bad)))
        side.synchronize()
        op.close()
    return out


# rel_maxnorm against the restatement after the six steps, bound 1e-13 as in test_gpu_rk4.  Forward Euler measures
# 1.14e-13 in the rho v row (graph and launch loop bit-equal): every Mult's device-oracle difference enters the state with
# the full weight dt, where RK4 averages four (RK4 on this case: 9.8e-14; RK2 9.6e-14, RK3 1.0e-13).  Set as the issue of this feature
# prescribes for a bound the device cannot meet: 4 x the larger of the RK4 test's observed error and this one's
# (DESIGN.md section 9).  RK2 and RK3 keep 1e-13.
REPLAY_REL_BOUND = {capi.FORWARD_EULER: 4 * 1.14e-13, capi.RK2: 1e-13, capi.RK3_SSP: 1e-13}


@pytest.mark.parametrize("integrator", NEW, ids=_name)
def test_advance_replays_a_captured_step(monkeypatch, integrator):
    """the case of test_gpu_rk4.test_advance_replays_a_captured_step, forcing term included (its pass sits inside the
    captured step).  The outlet's boundary-state buffers swap once per Mult: Euler and RK3 replay pairs of steps."""
    c, U = _nr_outlet_case(3)
    dt0, cfl, hmin, nsteps = 2.0e-5, 0.12, 0.05, 6
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
    o.set_forcing(FORCING)
    ref, t, dt, _ = iu.advance(o, integrator, U, 0.0, dt0, nsteps, False, cfl, hmin)
    (xg, sg), = _on_side_stream(monkeypatch, "1", c, U, FORCING, [(integrator, nsteps)], dt0, cfl, hmin)
    (xp, sp), = _on_side_stream(monkeypatch, "0", c, U, FORCING, [(integrator, nsteps)], dt0, cfl, hmin)
    assert np.array_equal(xg, xp) and sg == sp
    print(iu.NAMES[integrator], "time", sg[0], t, "next dt", sg[1], dt, "rel_maxnorm", rel_maxnorm(xg, ref).max())
    assert sg[0] == pytest.approx(t, rel=1e-13) and sg[1] == pytest.approx(dt, rel=1e-12) and sg[2] == 0
    assert rel_maxnorm(xg, ref).max() < REPLAY_REL_BOUND[integrator]


@pytest.mark.parametrize("forcing", [True, False], ids=["forcing", "trace_chain"])
def test_a_graph_of_one_scheme_is_never_replayed_for_another(monkeypatch, forcing):
    """rk4, forwardEuler, rk3, rk4 on one operator and one x: with the graph, every call after the first finds the graph of
    another scheme in the operator.  Without the forcing term the RK4 calls also chain their traces (ta_chain), which
    the schemes in between must leave neither valid nor used."""
    c, U = _nr_outlet_case(3)
    dt0, cfl, hmin = 2.0e-5, 0.12, 0.05
    calls = [("rk4", 4), ("forwardEuler", 4), ("rk3", 4), ("rk4", 4)]
    f = FORCING if forcing else None
    graph = _on_side_stream(monkeypatch, "1", c, U, f, calls, dt0, cfl, hmin)
    plain = _on_side_stream(monkeypatch, "0", c, U, f, calls, dt0, cfl, hmin)
    for call, (xg, sg), (xp, sp) in zip(calls, graph, plain):
        assert np.isfinite(xg).all() and sg[2] == 0, call
        assert np.array_equal(xg, xp) and sg == sp, call


# ---- 6. order in dt on the device ---------------------------------------------------------------------------------------
def test_time_loop_converges_at_the_order_of_each_scheme():
    """the setup of test_integrators_oracle.py through advance(..., integrator=...); the reference is the RK4 path"""
    from tps_amd.rhs_operator import RHSoperator

    mesh, disc, ph, U, t_end = iu.order_case()
    op = RHSoperator(mesh, disc, ph, [])

    def run(nsteps, integrator):
        x = _device_state(op, U)
        t, _, bad = op.advance(x, 0.0, t_end / nsteps, nsteps, True, integrator=integrator)
        assert bad == 0 and t == pytest.approx(t_end, rel=1e-12)
        return x.cpu().numpy()

    ref = run(160, "rk4")
    orders = {i: iu.observed_orders(lambda n: run(n, i), ref) for i in NEW}
    op.close()
    for i, (p1, p2, errs) in orders.items():
        print(iu.NAMES[i], "errors", errs, "orders", p1, p2)
    for i, (p1, p2, _) in orders.items():
        order = iu.ORDER[i]
        assert order - 0.4 < p1 < order + 0.4 and order - 0.4 < p2 < order + 0.4, iu.NAMES[i]


# ---- 7. status codes ----------------------------------------------------------------------------------------------------
def test_status_codes_come_before_any_device_work():
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    c, U = _dry_air_case()
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = _device_state(op, U)
    for integrator, status in (("rk6", capi.ERR_UNSUPPORTED), (capi.RK6, capi.ERR_UNSUPPORTED), (5, capi.ERR_INVALID_ARGUMENT),
                               (0, capi.ERR_INVALID_ARGUMENT)):
        with pytest.raises(TpsRhsError) as e:
            op.step(x, 0.0, 1e-7, integrator)
        assert e.value.status == status, integrator
        with pytest.raises(TpsRhsError) as e:
            op.advance(x, 0.0, 1e-7, 4, True, integrator=integrator)
        assert e.value.status == status, integrator
        if status == capi.ERR_UNSUPPORTED:
            assert "RK6" in str(e.value)
    with pytest.raises(ValueError):
        op.step(x, 0.0, 1e-7, "rk5")
    assert np.array_equal(x.cpu().numpy().reshape(U.shape), U)
    op.close()
