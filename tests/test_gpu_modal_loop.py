"""The modal filter inside the device time loop (tpsrhs_modal_filter_configure; tps_amd/csrc/time_loop.hip): off is off, a
threshold of +inf leaves the run as it was (RK4 across the chained and the unchained trace path), acting in the loop
(an advance against single unfiltered steps each followed by one application, bit for bit, for all four integrators, with a
second advance after reconfiguring), composed with the limiter as stages -> filter -> limiter, and the monitor seeing the
filtered state.  Small dry-air quad and hex cases at p = 2, a few steps each."""
import functools

import numpy as np
import pytest

import integrators_util as tu
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
INTEGRATORS = [capi.FORWARD_EULER, capi.RK2, capi.RK3_SSP, capi.RK4]
_name = lambda i: tu.NAMES[i]  # noqa: E731
DT, STEPS = 2.0e-6, 5
FILTER = dict(cutoff=0, alpha=2.0, exponent=2, conservative=True)  # strong: every step moves every row visibly
OTHER = dict(cutoff=1, alpha=0.5, exponent=1, conservative=False, rows=[0, 1])


@functools.lru_cache(maxsize=None)
def _case(dim):
    """dry air, periodic: box_quad(7, 3) p = 2, or box_hex(3, 3, 3) p = 2 warped (where k_flux hands its traces to the next
    stage, so that RK4 inside an advance is chained without a filter and unchained with one)"""
    mesh = meshgen.box_quad(7, 3, warp=0.05) if dim == 2 else meshgen.box_hex(3, 3, 3, warp=0.05)
    c = cases.Case("modal_loop", mesh, capi.Disc(2, 0, 0, 0, 0), capi.dry_air_physics(capi.NS, visc_mult=100.0), [])
    U = c.state(seed=3)
    U.setflags(write=False)
    return c, U


def _on_side_stream(monkeypatch, graph, c, body):
    """body(op, dev) on a fresh operator on a capturable side stream; dev(U) -> the device state"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    monkeypatch.setenv("TPSRHS_GRAPH", graph)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        out = body(op, lambda U: torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device))
        side.synchronize()
        op.close()
    return out


def _view(op, x):
    return x.view(op.num_equation, op.NDofs)


# ---- off is off --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", INTEGRATORS, ids=_name)
def test_off_is_off(monkeypatch, integrator):
    c, U = _case(2)

    def run(touch):
        def body(op, dev):
            if touch:
                op.configureModalFilter(**FILTER)
                op.configureModalFilter(off=True)
            x = dev(U)
            s = op.advance(x, 0.0, DT, STEPS, integrator=integrator)
            return x.cpu().numpy(), s, op.readModalFilter()
        return _on_side_stream(monkeypatch, "1", c, body)

    (xa, sa, ra), (xb, sb, rb) = run(False), run(True)
    assert np.isfinite(xa).all() and not np.array_equal(xa, U.ravel())
    assert np.array_equal(xa, xb) and sa == sb
    assert ra["calls"] == 0 and rb["calls"] == 0


# ---- a threshold of +inf filters nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "launches"])
@pytest.mark.parametrize("integrator,dim", [(i, 2) for i in INTEGRATORS] + [(capi.RK4, 3)],
                         ids=[_name(i) + "_2d" for i in INTEGRATORS] + ["rk4_3d_chained_against_unchained"])
def test_threshold_inf_leaves_the_run_as_it_was(monkeypatch, integrator, dim, graph):
    c, U = _case(dim)

    def run(filtered):
        def body(op, dev):
            if filtered:
                op.configureModalFilter(sensor_row=0, sensor_threshold=float("inf"), **FILTER)
            x = dev(U)
            s = op.advance(x, 0.0, DT, 6, integrator=integrator)
            return x.cpu().numpy(), s, op.readModalFilter()
        return _on_side_stream(monkeypatch, graph, c, body)

    (xa, sa, ra), (xb, sb, rb) = run(False), run(True)
    assert np.isfinite(xa).all() and not np.array_equal(xa, U.ravel())
    assert np.array_equal(xa, xb) and sa == sb
    assert ra["calls"] == 0
    assert rb["calls"] == 6 and rb["elements_seen"] == 6 * c.mesh.num_elements and rb["elements_filtered"] == 0


# ---- acting in the loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "launches"])
@pytest.mark.parametrize("integrator,dim", [(i, 2) for i in INTEGRATORS] + [(capi.RK4, 3)],
                         ids=[_name(i) + "_2d" for i in INTEGRATORS] + ["rk4_3d"])
def test_advance_with_the_filter_equals_steps_followed_by_applications(monkeypatch, integrator, dim, graph):
    c, U = _case(dim)
    ne = c.mesh.num_elements

    def advance(op, dev):
        op.configureModalFilter(**FILTER)
        x = dev(U)
        s1 = op.advance(x, 0.0, DT, STEPS, integrator=integrator)
        mid, r1 = x.cpu().numpy(), op.readModalFilter(reset=True)
        op.configureModalFilter(**OTHER)  # the graph of the first advance must not be replayed
        s2 = op.advance(x, s1[0], DT, STEPS, integrator=integrator)
        return mid, x.cpu().numpy(), s1, s2, r1, op.readModalFilter()

    def by_hand(op, dev):
        x = dev(U)
        t = 0.0
        for kw in (FILTER, OTHER):
            for _ in range(STEPS):
                t = op.step(x, t, DT, integrator)
                op.modalFilter(_view(op, x), **kw)
            if kw is FILTER:
                mid = x.cpu().numpy()
        return mid, x.cpu().numpy(), t

    mid_a, end_a, s1, s2, r1, r2 = _on_side_stream(monkeypatch, graph, c, advance)
    mid_h, end_h, t = _on_side_stream(monkeypatch, graph, c, by_hand)
    plain = _on_side_stream(monkeypatch, graph, c, lambda op, dev: (lambda x: (op.advance(x, 0.0, DT, STEPS, integrator=integrator),
                                                                              x.cpu().numpy())[1])(dev(U)))
    assert np.isfinite(end_a).all()
    assert not np.array_equal(mid_a, plain)  # the filter acts
    assert np.array_equal(mid_a, mid_h)
    assert np.array_equal(end_a, end_h)
    assert s2[0] == pytest.approx(t, rel=1e-15) and s1[2] == 0 and s2[2] == 0
    assert r1 == dict(calls=STEPS, elements_seen=STEPS * ne, elements_filtered=STEPS * ne)
    assert r2 == dict(calls=STEPS, elements_seen=STEPS * ne, elements_filtered=STEPS * ne)


# ---- with a limiter too: stages -> filter -> limiter ------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK4], ids=_name)
def test_with_a_limiter_the_step_is_stages_filter_limiter(monkeypatch, integrator):
    c, U = _case(2)

    def by_hand(op, dev, floor=None, filter_first=True):
        x = dev(U)
        t = 0.0
        for _ in range(STEPS):
            t = op.step(x, t, DT, integrator)
            if filter_first:
                op.modalFilter(_view(op, x), **FILTER)
            if floor is not None:
                op.limit(_view(op, x), [0], floor)
            if not filter_first:
                op.modalFilter(_view(op, x), **FILTER)
        return x.cpu().numpy()

    # a floor in the middle of the density's range after the filtered steps: the limiter has work in every step
    rho = _on_side_stream(monkeypatch, "1", c, by_hand).reshape(U.shape)[0]
    floor = 0.5 * (float(rho.min()) + float(rho.max()))
    assert rho.min() < floor < rho.max()

    def advance(op, dev):
        op.configureModalFilter(**FILTER)
        op.configureLimiter([0], floor)
        x = dev(U)
        op.advance(x, 0.0, DT, STEPS, integrator=integrator)
        return x.cpu().numpy(), op.readLimiter(), op.readModalFilter()

    xa, lim, mod = _on_side_stream(monkeypatch, "1", c, advance)
    xh = _on_side_stream(monkeypatch, "1", c, lambda op, dev: by_hand(op, dev, floor))
    xw = _on_side_stream(monkeypatch, "1", c, lambda op, dev: by_hand(op, dev, floor, filter_first=False))
    assert lim["calls"] == STEPS and lim["limited"][0] + lim["clamped"][0] > 0 and mod["calls"] == STEPS
    assert np.array_equal(xa, xh)
    assert not np.array_equal(xa, xw)  # the order matters on this state, and the loop has the contract's
    assert xa.reshape(U.shape)[0].min() >= floor  # the limiter has the last word on the floor


# ---- the monitor records the filtered state ---------------------------------------------------------------------------------------
def test_the_monitor_sees_the_filtered_state(monkeypatch):
    c, U = _case(2)

    def body(op, dev):
        op.configureModalFilter(**FILTER)
        op.configureMonitor(1, 8)
        x = dev(U)
        op.advance(x, 0.0, DT, 3, integrator=capi.RK4)
        return op.readMonitor(), op.readModalFilter()

    def by_hand(op, dev):
        x = dev(U)
        t, mins, maxs = 0.0, [], []
        for _ in range(3):
            t = op.step(x, t, DT, capi.RK4)
            unfiltered = _view(op, x).min(dim=1).values.cpu().numpy()
            op.modalFilter(_view(op, x), **FILTER)
            mins.append(_view(op, x).min(dim=1).values.cpu().numpy())
            maxs.append(_view(op, x).max(dim=1).values.cpu().numpy())
        return np.array(mins), np.array(maxs), unfiltered, mins[-1]

    rec, rep = _on_side_stream(monkeypatch, "1", c, body)
    mins, maxs, unfiltered, last = _on_side_stream(monkeypatch, "1", c, by_hand)
    assert rec["iters"].tolist() == [1, 2, 3] and rep["calls"] == 3
    assert np.array_equal(rec["mins"], mins) and np.array_equal(rec["maxs"], maxs)
    assert not np.array_equal(unfiltered, last)  # the extrema before and after the last application differ
