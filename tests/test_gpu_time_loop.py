"""The device time loop as a SEQUENCE of calls on one operator: tpsrhs_advance, rk4_step, Mult, setForcing and writes
to x by the caller, in the orders a driver makes them.

The loop keeps state between stages, steps and calls, and every piece of it is a cache that can go stale without
producing a NaN:
  - k_flux's epilogue forms the next stage's face-node traces (RkDev::ta_out, kernels.hpp); inside advance stage 4 hands
    them to the next step (TraceChain, trace_chain.hpp; launch_all asks it what each Mult reads and writes);
  - advance captures one step into a hipGraph and replays it, also in later calls whose StepKey matches (StepGraph);
  - consecutive sweeps alternate their direction (sweep_parity); a captured graph keeps the one it was captured with.

Every scenario makes the same calls three times:
  - fused: a default operator (traces from the epilogue, alternating sweeps, the captured step graph) on a capturable
    side stream, so that advance(..., >= 3 steps) takes the graph;
  - plain: a fresh operator with TPSRHS_FUSE_TRACES=0, TPSRHS_GRAPH=0, TPSRHS_SWEEP_ALT=0 -- every stage sweeps its own
    traces, one launch loop, one sweep direction;
  - the oracle (Oracle.advance / rk4_step / mult / set_forcing), the host restatement of M2ulPhyS::solveStep.
fused and plain must agree bit for bit after EVERY call (state, Mult result, time, dt, NaN census): the caches change
where the numbers come from, never the numbers.  Both must match the oracle: dry air within the bound of
test_gpu_rk4.py (rel_maxnorm < 1e-13), the plasma within _plasma_bound below.

Why StepKey is enough to decide a replay, and why the trace buffers swap an even number of times per step, is argued at
the top of tps_amd/csrc/trace_chain.hpp, next to the state it is about; tests/test_trace_chain.py drives that state
machine on the host.  The scenarios here cross each point of the argument on the device: test_calls_between_advances[forcing]
crosses config_epoch both ways, [mult] flips the sweep parity under a captured graph.
"""
import numpy as np
import pytest

from oracle_lib import Oracle
from parity_util import RHS_RTOL, rel_maxnorm
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu

FUSED = {"TPSRHS_FUSE_TRACES": "1", "TPSRHS_GRAPH": "1", "TPSRHS_SWEEP_ALT": "1"}
PLAIN = {"TPSRHS_FUSE_TRACES": "0", "TPSRHS_GRAPH": "0", "TPSRHS_SWEEP_ALT": "0"}
EPB = {1: 3, 2: 2, 3: 1}  # elements per block of the 3-D collocated kernels (Cfg::EPB, kernels.hpp)
TOUCH = 1.0 + 1e-6        # the caller's write to the leading seventh of x between two calls
EPS = np.finfo(np.float64).eps


def _tol(amp):
    """the one-Mult parity bound of test_gpu_parity._tol for perturbations of relative size amp"""
    return RHS_RTOL * 0.05 / amp


def _plasma_bound(amp, r):
    """Per equation, max |device - oracle| after the calls so far.  The state is x0 plus the step increments
    dt/6 (k1 + 2 k2 + 2 k3 + k4).  The kernels and the oracle evaluate every k to within _tol(amp) of the row's largest
    residual (the one-Mult parity bound of test_gpu_parity), so each increment carries at most _tol(amp) of its own size:
    the bound sums max |x_k - x_(k-1)| over the steps taken (`moved`).  On top come the roundings of the stage
    combinations, which the two sides order differently (the device recovers the RK4 accumulator from the stage states,
    kernels.hpp RkDev; the oracle accumulates z as MFEM's RK4Solver does): the device's three stage differences carry half
    an ulp of x each, the oracle's accumulator three roundings, and both a last one -- under 4 ulp of x per step."""
    return _tol(amp) * r["moved"] + 4 * r["steps"] * EPS * r["xmax"]


def _dry_air_bound(r):
    return 1e-13 * r["xmax"]  # rel_maxnorm < 1e-13, as in test_gpu_rk4.py


def _active_species(ph):
    if ph.working_fluid != capi.USER_DEFINED:
        return 0
    return ph.mixture.num_species - (2 if ph.mixture.ambipolar else 1)


def _finite_max(a):
    return np.where(np.isfinite(a), np.abs(a), 0.0).max(axis=1)


def _device(monkeypatch, c, U, calls, env, dt0, cfl, hmin, poison=False):
    """`calls` on one operator created and run under `env`, on a capturable side stream.  Per call: the state, the Mult
    result (None for the other calls) and (time, dt, NaN census of the call)."""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TPSRHS_POISON", "1" if poison else "0")
    side = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
        y = torch.empty_like(x)
        t, dt, bad = 0.0, dt0, 0
        for call in calls:
            y_out = None
            if call[0] == "advance":
                t, dt, bad = op.advance(x, t, dt, call[1], call[2], cfl, hmin)
            elif call[0] == "rk4_step":
                t = op.rk4_step(x, t, dt, want_nan_count=True)
                bad = op.nan_count
            elif call[0] == "mult":
                op.Mult(x, y)
                y_out = y.cpu().numpy().reshape(U.shape)
            elif call[0] == "touch":
                x[: x.numel() // 7] *= TOUCH
            elif call[0] == "forcing":
                op.setForcing(call[1])
            elif call[0] == "new_tensor":
                x_new = x.clone()
                assert x_new.data_ptr() != x.data_ptr()
                x = x_new
            else:
                raise ValueError(call[0])
            out.append((x.cpu().numpy().reshape(U.shape), y_out, (t, dt, bad)))
        side.synchronize()
        op.close()
    return out


def _oracle(c, U, calls, dt0, cfl, hmin, device_clamp=False):
    """The same calls on the oracle.  advance goes one step at a time (tpsoracle_advance is that loop), which gives the
    per-step increments of _plasma_bound and, per step, the species entries Check_Undershoot set to 0.
    device_clamp: Check_Undershoot as the reference's device build has it, max(NaN, 0) = fmax = 0 (the kernels'), where
    the host build's std::max -- the oracle's -- keeps the NaN; the two differ on NaN species entries only."""
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
    sp = slice(c.mesh.dim + 2, c.mesh.dim + 2 + _active_species(c.physics))
    x, t, dt, bad = np.array(U, dtype=np.float64), 0.0, dt0, 0
    moved, steps, clamped = np.zeros(U.shape[0]), 0, []
    out = []

    def step(xn, b):
        nonlocal x, moved, steps, bad
        if device_clamp:
            xn[sp] = np.where(np.isnan(xn[sp]), 0.0, xn[sp])
        moved = moved + _finite_max(xn - x)
        steps += 1
        bad += b
        # (an RK4 update does not land on exactly 0.0: a zero species entry is one the clamp of this step set)
        clamped.append(int(np.count_nonzero(xn[sp] == 0.0)))
        x = xn

    for call in calls:
        if call[0] == "advance":
            bad = 0
            for _ in range(call[1]):
                xn, t, dt, b = o.advance(x, t, dt, 1, call[2], cfl, hmin)
                step(xn, b)
        elif call[0] == "rk4_step":
            bad = 0
            xn, t, _, b = o.rk4_step(x, t, dt)
            step(xn, b)
        elif call[0] == "touch":
            x = x.copy()
            flat = x.reshape(-1)
            flat[: flat.size // 7] *= TOUCH
        elif call[0] == "forcing":
            o.set_forcing(call[1])
        elif call[0] not in ("mult", "new_tensor"):  # (a Mult of these cases changes no oracle state)
            raise ValueError(call[0])
        out.append({"x": x.copy(), "state": (t, dt, bad), "moved": moved.copy(), "steps": steps, "xmax": _finite_max(x),
                    "clamped": list(clamped)})
    return o, out


def _check(calls, fused, plain, ref, bound, oracle, rhs_tol, nan=False):
    """fused == plain bit for bit after every call; both within `bound` of the oracle"""
    for i, (call, (xf, yf, sf), (xp, yp, sp), r) in enumerate(zip(calls, fused, plain, ref)):
        where = f"call {i} ({call[0]})"
        assert np.array_equal(xf, xp, equal_nan=nan), where + ": the fused / graph run and the plain run differ"
        assert sf == sp, where
        if yf is not None:
            assert np.array_equal(yf, yp), where
            err_y = rel_maxnorm(yf, oracle.mult(xf))  # the oracle's Mult of the very state the device had
            print(f"{where}: Mult vs oracle rel err {err_y.max():.2e}")
            assert err_y.max() < rhs_tol, where
        xr, (t, dt, bad) = r["x"], r["state"]
        assert sf[0] == pytest.approx(t, rel=1e-13) and sf[1] == pytest.approx(dt, rel=1e-12), where
        assert sf[2] == bad, where + f": NaN census {sf[2]}, the oracle's {bad}"
        ok = np.isfinite(xr)
        assert np.isfinite(xf[ok]).all(), where + ": a NaN where the oracle has a number"
        err = np.where(ok, np.abs(xf - xr), 0.0).max(axis=1)
        lim = bound(r)
        print(f"{where}: t {sf[0]:.6e} dt {sf[1]:.4e} NaN {sf[2]}; max|device - oracle| / bound per equation",
              np.array2string(err / np.maximum(lim, 1e-300), precision=3))
        assert (err <= lim).all(), where


def _run(monkeypatch, c, U, calls, dt0, cfl, hmin, bound, rhs_tol, nan=False, poison=False, oracle_run=None):
    fused = _device(monkeypatch, c, U, calls, FUSED, dt0, cfl, hmin, poison)
    plain = _device(monkeypatch, c, U, calls, PLAIN, dt0, cfl, hmin, poison)
    o, ref = oracle_run if oracle_run is not None else _oracle(c, U, calls, dt0, cfl, hmin, device_clamp=nan)
    if poison:  # a trace record the epilogue did not write is a NaN, not an old value
        for xf, yf, _ in fused + plain:
            assert np.isfinite(xf).all() and (yf is None or np.isfinite(yf).all())
    _check(calls, fused, plain, ref, bound, o, rhs_tol, nan)
    return fused, ref


def _plasma_case(order, two_t=False):
    """the argon ternary plasma of the headline (ARGON_MINIMAL transport, Arrhenius chemistry, isothermal walls).
    p = 3: a small O-grid cylinder.  p = 1, 2: a box of 5 x 5 x 5 scrambled hexes walled in on all sides -- 125 elements,
    odd and not a multiple of 3, so that the last block of every sweep is only partly filled at both orders."""
    if order == 3:
        c = cases.argon_cyl3d(3, 6, 3, order, two_t)
    else:
        walls = {(d, s): 3 for d in range(3) for s in (0, 1)}
        mesh = meshgen.scramble_orientations(
            meshgen.box_hex(5, 5, 5, lengths=(1.0, 0.8, 1.2), periodic=(False,) * 3, bdr_attr=walls, warp=0.1), 3)
        c = cases.Case(f"argon_box_p{order}", mesh, capi.Disc(order, 0, 0, 0, 0), capi.argon_ternary_physics(capi.NS, two_t),
                       [capi.make_bc(3, capi.WALL, capi.VISC_ISOTH, [3000.0])])
    amp = 0.005 if order == 1 else 0.01  # (keeps the interpolated species densities positive, as in test_gpu_parity)
    return c, c.state(seed=11 + order, amp=amp), amp


def _stable_steps(c, U):
    """dt0: a tenth of the fastest local time scale of the residual (as test_gpu_rk4 takes it: the electron energy
    exchange of the two-temperature plasma is much stiffer than the acoustic limit); cfl, hmin: the CFL-controlled step
    cfl hmin / (max char speed dim) starts at dt0 too"""
    o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
    y0 = o.mult(U)
    dt0 = 0.1 / (np.abs(y0) / np.maximum(np.abs(U), 1e-300 + 1e-6 * np.abs(U).max(axis=1, keepdims=True))).max()
    cfl = 0.5
    return dt0, cfl, dt0 * o.max_char_speed * c.mesh.dim / cfl


_ORACLE_RUNS = {}  # scenarios 1 and 7 make the same calls: one oracle run each


def _plasma_advance(monkeypatch, order, two_t, constant_dt, poison):
    c, U, amp = _plasma_case(order, two_t)
    ne = c.mesh.num_elements
    print(f"argon {'2T' if two_t else '1T'} p = {order}: {ne} hexes, ne % EPB = {ne} % {EPB[order]} = {ne % EPB[order]}")
    if order < 3:
        assert ne % EPB[order] != 0 and ne % 2 == 1  # a partly filled last block at p = 1 and at p = 2
    dt0, cfl, hmin = _stable_steps(c, U)
    calls = [("advance", 4, constant_dt)]
    key = (order, two_t, constant_dt)
    if key not in _ORACLE_RUNS:
        _ORACLE_RUNS[key] = _oracle(c, U, calls, dt0, cfl, hmin)
    _run(monkeypatch, c, U, calls, dt0, cfl, hmin, lambda r: _plasma_bound(amp, r), _tol(amp), poison=poison,
         oracle_run=_ORACLE_RUNS[key])


# ---- 1. plasma advance against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("constant_dt", [True, False])
@pytest.mark.parametrize("order,two_t", [(3, False), (3, True), (2, True), (1, False)])
def test_plasma_advance_matches_oracle(monkeypatch, order, two_t, constant_dt):
    _plasma_advance(monkeypatch, order, two_t, constant_dt, poison=False)


# ---- 7. the same with every device allocation poisoned: partly filled blocks in the flux epilogue -----------------------
@pytest.mark.parametrize("order,two_t", [(2, True), (1, False)])
def test_partial_blocks_poisoned(monkeypatch, order, two_t):
    _plasma_advance(monkeypatch, order, two_t, False, poison=True)


# ---- 2. one captured graph replayed by later calls ----------------------------------------------------------------------
def test_graph_reused_across_calls(monkeypatch):
    """Three calls on one operator and the same x.  The second and the third REPLAY the graph the first captured: x is the
    same tensor, constant_dt, cfl and hmin are the same (coef), nothing sets the forcing or the mixing length in between
    (epoch), and without non-reflecting faces bstate_cur never moves.  Only dt and the time differ between the calls, and
    the graph reads those from device memory."""
    c, U, amp = _plasma_case(3)
    dt0, cfl, hmin = _stable_steps(c, U)
    calls = [("advance", 5, False), ("advance", 5, False), ("advance", 4, False)]
    _run(monkeypatch, c, U, calls, dt0, cfl, hmin, lambda r: _plasma_bound(amp, r), _tol(amp))


# ---- 3. calls between two advances ---------------------------------------------------------------------------------------
PRESSURE_GRADIENT = capi.make_forcing(pressure_gradient=(2.0e3, 0.0, -1.0e3))
BETWEEN = {
    "mult": [("mult",)],  # an odd number of sweeps: the next advance replays a graph of the other sweep direction
    "rk4_step": [("rk4_step",)],
    "outside_write": [("touch",)],
    # config_epoch twice: chaining off (the separate stage kernel) and on again, a graph captured each time
    "forcing": [("forcing", PRESSURE_GRADIENT), ("advance", 4, False), ("forcing", capi.make_forcing())],
    "new_tensor": [("new_tensor",)],  # a new StepKey.x
}


@pytest.mark.parametrize("between", list(BETWEEN))
def test_calls_between_advances(monkeypatch, between):
    c, U, amp = _plasma_case(3)
    dt0, cfl, hmin = _stable_steps(c, U)
    calls = [("advance", 4, False)] + BETWEEN[between] + [("advance", 4, False)]
    _run(monkeypatch, c, U, calls, dt0, cfl, hmin, lambda r: _plasma_bound(amp, r), _tol(amp))
    if between == "forcing":  # the term is large enough to be seen: its share of the momentum residual
        o = Oracle(c.mesh, c.disc, c.physics, c.bcs)
        y0 = o.mult(U)
        o.set_forcing(PRESSURE_GRADIENT)
        assert rel_maxnorm(o.mult(U), y0)[1] > 1e-6


# ---- 4. short runs: the plain loop with chained traces, then a graph -----------------------------------------------------
def test_short_runs_chain_traces_without_a_graph(monkeypatch):
    c, U, amp = _plasma_case(3)
    dt0, cfl, hmin = _stable_steps(c, U)
    calls = [("advance", 1, True), ("advance", 2, True), ("advance", 3, True)]
    _run(monkeypatch, c, U, calls, dt0, cfl, hmin, lambda r: _plasma_bound(amp, r), _tol(amp))


# ---- 5. non-reflecting outlet: the boundary-state swap and k_bc_mean across the graph boundary ---------------------------
@pytest.mark.parametrize("order", [2, 3])
def test_nonreflecting_outlet_across_calls(monkeypatch, order):
    c = cases.cyl3d(4, 12, 3, order, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_P_NR, [101000.0, 0, 0, 0, 0.0, 0.0, 1.0, 0.0])
    # six steps in all, as test_gpu_rk4.test_advance_replays_a_captured_step: the bound of test_gpu_rk4 is stated for that
    # many (the rounding differences grow by ~4 % of it per step: p = 3 reaches 1.02e-13 in the rho v row after eight)
    calls = [("advance", 3, False), ("advance", 3, False)]
    _run(monkeypatch, c, c.state(seed=2), calls, 2.0e-5, 0.12, 0.05, _dry_air_bound, RHS_RTOL)


# ---- 6. the species clamp and a NaN inside chained steps -----------------------------------------------------------------
def test_species_clamp_in_chained_steps(monkeypatch):
    """Check_Undershoot in stage 4 feeds both x and the next step's traces.  The metastable density of a four-species
    argon mixture varies over four decades from node to node (as in test_gpu_parity.test_species_clamp_active), and the
    RK4 update takes entries of it below 0 in every step."""
    order = 2
    mesh = meshgen.scramble_orientations(meshgen.box_hex(3, 4, 3, lengths=(1.0, 0.8, 1.2), warp=0.1), 5)
    ph = capi.argon_levels_physics(1, True, capi.NS, capi.CONSTANT, False, True)
    c = cases.Case("argon_levels_box", mesh, capi.Disc(order, 0, 0, 0, 0), ph, [])
    U = cases.plasma_state(node_coordinates(mesh, order), ph, nvel=3, seed=21, amp=0.01)
    im = 3 + 2 + 1  # rho Y of Ar_m (mixture order Ar.+1, Ar_m, E, Ar; ambipolar: the first two are active)
    U[im] = U[im].mean() * 10.0 ** np.random.default_rng(8).uniform(-4.0, 0.0, size=U.shape[1])
    k = Oracle(c.mesh, c.disc, c.physics, c.bcs).mult(U)[im]
    # 1.5 times the step in which forward Euler would take the first metastable entry to 0: the RK4 update then takes a
    # few entries below 0 in every step, at a step still far below the acoustic limit of the mesh (~1e-5 s)
    dt = 1.5 * (U[im][k < 0] / -k[k < 0]).min()
    calls = [("advance", 4, True), ("advance", 3, True)]
    _, ref = _run(monkeypatch, c, U, calls, dt, 1.0, 1.0, lambda r: _plasma_bound(0.01, r), _tol(0.01))
    clamped = ref[-1]["clamped"]
    print("species entries clamped to 0 in steps 1..7:", clamped)
    assert sum(clamped[1:]) > 0


def test_nan_census_in_chained_steps(monkeypatch):
    """One NaN density entry: the census of the call equals the oracle's, the NaN reaches the same entries, and every entry
    it has not reached matches the oracle.  The oracle clamps as the reference's device build does (_oracle device_clamp:
    a NaN species entry becomes 0, which changes the census of the later steps -- 9056 against 9120 here).  A long box
    keeps part of the mesh finite over the three steps that take the graph (the gradient and the flux sweep each carry
    the NaN one element further per stage)."""
    order = 1
    attrs = {(d, s): 1 for d in range(3) for s in (0, 1)}
    mesh = meshgen.box_hex(32, 2, 2, lengths=(3.2, 0.2, 0.2), periodic=(False, False, False), bdr_attr=attrs)
    ph = capi.argon_ternary_physics(capi.NS, False, capi.CONSTANT, None)
    c = cases.Case("argon_box", mesh, capi.Disc(order, 0, 0, 0, 0), ph, [capi.make_bc(1, capi.WALL, capi.VISC_ISOTH, [3000.0])])
    U = cases.plasma_state(node_coordinates(mesh, order), ph, nvel=3, seed=3, amp=0.005)
    dt0, cfl, hmin = _stable_steps(c, U)
    U[0, 5] = np.nan  # one bad density entry in the first element
    calls = [("advance", 3, True)]
    fused, ref = _run(monkeypatch, c, U, calls, dt0, cfl, hmin, lambda r: _plasma_bound(0.005, r), _tol(0.005), nan=True)
    xf, xr = fused[-1][0], ref[-1]["x"]
    print("NaN census", fused[-1][2][2], "NaN entries", np.isnan(xf).sum(), "(oracle", np.isnan(xr).sum(), ") finite",
          np.isfinite(xf).sum())
    assert fused[-1][2][2] > 0 and np.isnan(xr).any() and np.isfinite(xr).sum() > xr.size // 8
    assert np.array_equal(np.isnan(xf), np.isnan(xr)) and not np.isnan(xf[5]).any()  # (row 5: the ion density)
