"""The conservative limiter inside the device time loop (tpsrhs_limiter_configure; tps_amd/csrc/time_loop.hip): off is off,
transparent when nothing undershoots (all four integrators, captured step graph and launch loop, RK4 across the chained and
the unchained trace path), acting in the loop (advance against single steps bit for bit, forward Euler against
limit(x0 + dt Mult(x0)) assembled with torch, the density total kept where the clamp would move it), and the observers
seeing the limited state."""
import functools

import numpy as np
import pytest

import integrals_util as iu
import integrators_util as tu
from parity_util import rel_maxnorm
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
EPS = iu.EPS
INTEGRATORS = [capi.FORWARD_EULER, capi.RK2, capi.RK3_SSP, capi.RK4]
_name = lambda i: tu.NAMES[i]  # noqa: E731
GAMMA, RHO0, P0, VEL0 = 1.4, 1.2, 101300.0, 20.0


@functools.lru_cache(maxsize=None)
def _smooth_case(dim):
    """dry air, periodic: box_quad(7, 3) p = 2, or box_hex(3, 3, 3) p = 2 (where k_flux hands its traces to the next stage,
    so that RK4 inside an advance is chained without a limiter and unchained with one)"""
    mesh = meshgen.box_quad(7, 3) if dim == 2 else meshgen.box_hex(3, 3, 3, warp=0.05)
    c = cases.Case("limiter_loop", mesh, capi.Disc(2, 0, 0, 0, 0), capi.dry_air_physics(capi.NS, visc_mult=100.0), [])
    U = c.state(seed=3)
    U.setflags(write=False)
    return c, U


@functools.lru_cache(maxsize=None)
def _wave_case():
    """dry air on box_quad(7, 3), p = 3: a 20 % density wave of one wavelength per element at uniform velocity and pressure --
    every element mean stays near RHO0 while nodes dip to 0.8 RHO0, below the floor 0.9 RHO0: the limiter scales, in every
    element, and the mean never is inadmissible.  The velocity u = VEL0 cos(2 pi 7 x) cos(2 pi 3 y) diverges where the density
    is low (du/dx = -44 VEL0 sin cos): the nodes the limiter has put on the floor are below it again after the next step and
    the limiter fires in every step.  (With a uniform velocity, along x or against it, the dissipation of the face fluxes
    lifts the troughs and it fires in the first step only; so it does with VEL0 < 0.)"""
    mesh = meshgen.box_quad(7, 3)
    c = cases.Case("limiter_wave", mesh, capi.Disc(3, 0, 0, 0, 0), capi.dry_air_physics(capi.EULER), [])
    X = node_coordinates(mesh, 3)
    cy = np.cos(2.0 * np.pi * 3.0 * X[1])
    rho = RHO0 * (1.0 + 0.2 * np.sin(2.0 * np.pi * 7.0 * X[0]) * cy)
    u = VEL0 * np.cos(2.0 * np.pi * 7.0 * X[0]) * cy
    U = np.zeros((4, X.shape[1]))
    U[0], U[1] = rho, rho * u
    U[3] = P0 / (GAMMA - 1.0) + 0.5 * rho * u * u
    U.setflags(write=False)
    return c, U


FLOOR = 0.9 * RHO0
DT_WAVE = 2.0e-6
DT_SMOOTH = {2: 2.0e-6, 3: 2.0e-6}


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


# ---- 8. off is off -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK4], ids=_name)
def test_off_is_off(monkeypatch, integrator):
    c, U = _wave_case()

    def run(touch):
        def body(op, dev):
            if touch:
                op.configureLimiter([0], FLOOR)
                op.configureLimiter(off=True)
            x = dev(U)
            s = op.advance(x, 0.0, DT_WAVE, 5, integrator=integrator)
            return x.cpu().numpy(), s
        return _on_side_stream(monkeypatch, "1", c, body)

    (xa, sa), (xb, sb) = run(False), run(True)
    assert np.array_equal(xa, xb) and sa == sb
    assert xa.reshape(U.shape)[0].min() < FLOOR  # ... and nothing was limited


# ---- 9. transparent when nothing undershoots ---------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "launches"])
@pytest.mark.parametrize("integrator,dim", [(i, 2) for i in INTEGRATORS] + [(capi.RK4, 3)],
                         ids=[_name(i) + "_2d" for i in INTEGRATORS] + ["rk4_3d_chained_against_unchained"])
def test_transparent_when_nothing_undershoots(monkeypatch, integrator, dim, graph):
    c, U = _smooth_case(dim)

    def run(limited):
        def body(op, dev):
            if limited:
                op.configureLimiter([0], 1.0e-3)  # far below the density, ~1.2
            x = dev(U)
            s = op.advance(x, 0.0, DT_SMOOTH[dim], 6, integrator=integrator)
            return x.cpu().numpy(), s, op.readLimiter()
        return _on_side_stream(monkeypatch, graph, c, body)

    (xa, sa, ra), (xb, sb, rb) = run(False), run(True)
    assert np.isfinite(xa).all() and not np.array_equal(xa, U.ravel())
    assert np.array_equal(xa, xb) and sa == sb
    assert ra["calls"] == 0
    assert rb["calls"] == 6 and rb["limited"].sum() == 0 and rb["clamped"].sum() == 0
    assert rb["pressure_limited"] == 0 and rb["pressure_unfixable"] == 0


# ---- 10. acting in the loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "launches"])
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK4], ids=_name)
def test_advance_with_a_firing_limiter_equals_single_steps(monkeypatch, integrator, graph):
    c, U = _wave_case()
    ne = c.mesh.num_elements

    def advance(op, dev):
        op.configureLimiter([0], FLOOR)
        x = dev(U)
        s = op.advance(x, 0.0, DT_WAVE, 5, integrator=integrator)
        return x.cpu().numpy(), s, op.readLimiter()

    def steps(op, dev):
        op.configureLimiter([0], FLOOR)
        x = dev(U)
        t, fired = 0.0, []
        for _ in range(5):
            t = op.step(x, t, DT_WAVE, integrator)
            fired.append(int(op.readLimiter(reset=True)["limited"][0]))
        return x.cpu().numpy(), t, fired

    xa, sa, ra = _on_side_stream(monkeypatch, graph, c, advance)
    xs, ts, fired = _on_side_stream(monkeypatch, graph, c, steps)
    print(f"{_name(integrator)}: elements limited per step {fired} of {ne}; in the advance {ra['limited'][0]}")
    assert np.array_equal(xa, xs) and sa[0] == pytest.approx(ts, rel=1e-15) and sa[2] == 0
    assert fired[0] == ne and min(fired) > 0  # the limiter fires in every step
    assert ra["calls"] == 5 and ra["limited"][0] == sum(fired) and ra["clamped"].sum() == 0
    assert xa.reshape(U.shape)[0].min() >= FLOOR


def test_one_euler_step_is_the_limited_euler_update():
    import torch
    from tps_amd.rhs_operator import RHSoperator

    c, U = _wave_case()
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x0 = torch.tensor(U.ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x0)
    op.Mult(x0, y)
    update = x0 + DT_WAVE * y
    plain = update.cpu().numpy().reshape(U.shape)
    total_plain = op.integrate(update)[0].cpu().numpy()
    ref_t = update.clone()
    op.limit(ref_t, [0], FLOOR)
    ref = ref_t.cpu().numpy().reshape(U.shape)
    op.readLimiter(reset=True)
    op.configureLimiter([0], FLOOR)
    x = x0.clone()
    op.step(x, 0.0, DT_WAVE, capi.FORWARD_EULER)
    rep = op.readLimiter()
    total = op.integrate(x)[0].cpu().numpy()
    got = x.cpu().numpy().reshape(U.shape)
    op.close()
    assert rep["calls"] == 1 and rep["limited"][0] == c.mesh.num_elements and rep["clamped"].sum() == 0
    # the tolerance of tests/test_gpu_integrators.py for its forward-Euler comparison (_assert_step_parity)
    rowmax = lambda a: np.abs(a).reshape(a.shape[0], -1).max(axis=1)  # noqa: E731
    incr, err = rowmax(ref - U), rowmax(got - ref)
    print("increment", incr, "difference", err, "rel_maxnorm", rel_maxnorm(got, ref).max())
    assert (err <= 1e-9 * incr + 1e-15 * rowmax(U)).all()
    assert rel_maxnorm(got, ref).max() < 1e-13
    # the density total is that of x0 + dt Mult(x0), within the bounds of the two integrate calls ...
    ra = iu.integrate(c.mesh, 3, 0, plain[:1])
    rb = iu.integrate(c.mesh, 3, 0, got[:1])
    bound = ra["K"] * EPS * (ra["S1"][0] + rb["S1"][0])
    print(f"|total - total of the plain update| / bound = {abs(total[0] - total_plain[0]) / bound:.3f}")
    assert abs(total[0] - total_plain[0]) <= bound
    # ... where the clamp max(v, floor) of the same array moves it by more than 1000 times that
    clamp = iu.integrate(c.mesh, 3, 0, np.maximum(plain[:1], FLOOR))["sum"][0]
    assert abs(clamp - ra["sum"][0]) > 1000 * bound
    assert got[0].min() >= FLOOR and plain[0].min() < FLOOR


# ---- 11. observers see the limited state ---------------------------------------------------------------------------------------
def test_the_monitor_sees_the_limited_state(monkeypatch):
    c, U = _wave_case()

    def body(op, dev):
        op.configureLimiter([0], FLOOR)
        op.configureMonitor(1, 8)
        x = dev(U)
        op.advance(x, 0.0, DT_WAVE, 4, integrator=capi.RK4)
        return op.readMonitor()

    rec = _on_side_stream(monkeypatch, "1", c, body)
    assert rec["iters"].tolist() == [1, 2, 3, 4]
    assert (rec["mins"][:, 0] >= FLOOR).all() and U[0].min() < FLOOR
