"""Running mean and velocity covariances sampled in the device time loop (tpsrhs_stats_*, k_stats_sample) against the
numpy restatement of tests/statistics_util.py, which tests/test_statistics_restatement.py pins on the CPU.

The restatement is fed the outputs of tpsrhs_eval_pointwise (quantities 0 and 1: primitives and pressure) for the same
states: those kernels are older than this feature and tested elsewhere; the recurrence, the row order, the counters and
where the time loop puts its samples are what is under test.  Shapes are those of tests/test_gpu_integrators.py, plus one
axisymmetric mesh with an odd number of nodes, where the rows of the fields are not all 16-byte aligned and the scalar
form of the kernel runs."""
import ctypes as C

import numpy as np
import pytest

import statistics_util as su
from tps_amd import capi, cases

pytestmark = pytest.mark.gpu

KINDS = ["dry_air", "argon_2T", "axisym", "axisym_odd"]
S = 5


def _case(kind):
    """-> (case, state(seed), nvel)"""
    if kind == "dry_air":
        c = cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
        c.physics.dry_air.visc_mult = 100.0
        return c, (lambda seed: c.state(seed=seed)), 3
    if kind == "argon_2T":
        c = cases.argon_cyl3d(4, 12, 3, 2, True, capi.CONSTANT, "arrhenius", capi.VISC_ISOTH)
        return c, (lambda seed: c.state(seed=seed, amp=0.01)), 3
    if kind == "axisym":  # dim = 2, nvel = 3: six covariances, the pressure in row 4
        c = cases.dry_air_axisym(4, 6, 2)
        return c, (lambda seed: c.state(seed=seed)), 3
    c = cases.dry_air_axisym(3, 5, 2)  # 15 elements of 9 nodes: NDofs is odd
    assert (c.mesh.num_elements * 9) % 2 == 1
    return c, (lambda seed: c.state(seed=seed)), 3


def _nr_outlet_case(order):
    c = cases.cyl3d(4, 12, 3, order, capi.NS, capi.VISC_ISOTH)
    c.physics.dry_air.visc_mult = 100.0
    # a non-reflecting outlet on top: its boundary state integrates with the device-side dt too
    c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_P_NR, [101000.0, 0, 0, 0, 0.0, 0.0, 1.0, 0.0])
    return c, c.state(seed=2)


def _device_state(op, U):
    import torch

    return torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)


def _operator(c, **kw):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs, **kw)


def _prim_p(op, x):
    """(primitives (neq, n), pressure (n)) of the device state x from tpsrhs_eval_pointwise"""
    import torch

    lib, n = capi.load(), op.NDofs
    prim = torch.empty(op.num_equation * n, dtype=torch.float64, device=op.device)
    p = torch.empty(n, dtype=torch.float64, device=op.device)
    assert lib.tpsrhs_eval_pointwise(op._h, 0, n, C.c_void_p(x.data_ptr()), C.c_void_p(prim.data_ptr())) == 0
    assert lib.tpsrhs_eval_pointwise(op._h, 1, n, C.c_void_p(x.data_ptr()), C.c_void_p(p.data_ptr())) == 0
    return prim.cpu().numpy().reshape(op.num_equation, n), p.cpu().numpy()


def _stats(op):
    mean, vari, nm, nv, it = op.getStatistics()
    return mean.cpu().numpy(), (vari.cpu().numpy() if vari is not None else None), nm, nv, it


def _assert_within(got_mean, got_vari, samples, nvel, what, extra_rel=0.0):
    mean, vari, _, _ = su.run(samples, nvel)
    mean_b, vari_b = su.bounds(samples, nvel, extra_rel)
    em, ev = np.abs(got_mean - mean).max(axis=1), np.abs(got_vari - vari).max(axis=1)
    print(what, "mean: |diff| / bound per row", np.array2string(em / mean_b, precision=3))
    print(what, "vari: |diff| / bound per row", np.array2string(ev / vari_b, precision=3))
    assert np.isfinite(got_mean).all() and np.isfinite(got_vari).all()
    assert (em <= mean_b).all() and (ev <= vari_b).all()


# ---- 1. add_sample against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_add_sample_matches_restatement(kind):
    c, state, nvel = _case(kind)
    op = _operator(c)
    op.configureStatistics(1)
    assert op.numVariances() == su.num_variances(nvel)
    samples = []
    for seed in range(1, S + 1):
        x = _device_state(op, state(seed))
        op.addSample(x)
        samples.append(_prim_p(op, x))
    mean, vari, nm, nv, it = _stats(op)
    op.close()
    assert (nm, nv, it) == (S, S, 0)  # add_sample does not count steps
    assert mean.shape == samples[0][0].shape and vari.shape == (su.num_variances(nvel), mean.shape[1])
    _assert_within(mean, vari, samples, nvel, kind)


def test_mean_only():
    """compute_variances = 0: the same mean, bit for bit, and no covariance field"""
    c, state, nvel = _case("dry_air")
    op = _operator(c)
    means = []
    for variances in (True, False):
        op.configureStatistics(1, variances=variances)
        for seed in range(1, 4):
            op.addSample(_device_state(op, state(seed)))
        mean, vari, nm, nv, _ = _stats(op)
        assert (vari is None) == (not variances) and op.numVariances() == (su.num_variances(nvel) if variances else 0)
        assert nm == nv == 3
        means.append(mean)
    assert np.array_equal(means[0], means[1])
    m = _device_state(op, means[0])  # a covariance field for an operator that keeps none
    assert capi.load().tpsrhs_stats_set(op._h, C.c_void_p(m.data_ptr()), C.c_void_p(m.data_ptr()), 3, 3) == capi.ERR_INVALID_ARGUMENT
    assert capi.load().tpsrhs_stats_get(op._h, None, C.c_void_p(m.data_ptr()), None, None, None) == capi.ERR_INVALID_ARGUMENT
    op.close()


# ---- 2. the first sample is the state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("kind", KINDS)
def test_first_sample_is_the_state(monkeypatch, kind, poison):
    monkeypatch.setenv("TPSRHS_POISON", "1" if poison else "0")
    c, state, nvel = _case(kind)
    op = _operator(c)
    op.configureStatistics(4, start_iter=9)
    mean, vari, nm, nv, it = _stats(op)  # fresh fields are zero, not what the allocation held
    assert not mean.any() and not vari.any() and (nm, nv, it) == (0, 0, 0)
    x = _device_state(op, state(3))
    op.addSample(x)
    prim, p = _prim_p(op, x)
    mean, vari, nm, nv, _ = _stats(op)
    op.close()
    assert np.isfinite(mean).all() and np.isfinite(vari).all()
    assert np.array_equal(mean, su.sample_of(prim, p, nvel))
    assert np.array_equal(mean[1 + nvel], p) and not np.array_equal(prim[1 + nvel], p)
    assert not vari.any() and nm == nv == 1


# ---- 3. statistics do not touch the solution, and replay equals the launch loop -------------------------------------------
GRAPH = {"TPSRHS_GRAPH": "1"}
LOOP = {"TPSRHS_GRAPH": "0"}
FUSED = {"TPSRHS_FUSE_TRACES": "1", "TPSRHS_GRAPH": "1", "TPSRHS_SWEEP_ALT": "1"}
PLAIN = {"TPSRHS_FUSE_TRACES": "0", "TPSRHS_GRAPH": "0", "TPSRHS_SWEEP_ALT": "0"}


def _on_side_stream(monkeypatch, env, c, U, integrator, nsteps, constant_dt, dt0, cfl, hmin, stats=None, per_call=None):
    """One operator and one x on a capturable side stream; `stats` = the arguments of configureStatistics or None;
    per_call: steps per advance call (default: all in one).  -> x, (time, dt, census), statistics or None, and the
    state after every call"""
    import torch

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = _operator(c, stream=side)
        if stats is not None:
            op.configureStatistics(**stats)
        x = _device_state(op, U)
        t, dt, bad, after = 0.0, dt0, 0, []
        for _ in range(0, nsteps, per_call or nsteps):
            t, dt, b = op.advance(x, t, dt, per_call or nsteps, constant_dt, cfl, hmin, integrator=integrator)
            bad += b
            after.append(x.clone())
        st = _stats(op) if stats is not None else None
        out = x.cpu().numpy().reshape(U.shape)
        after = [a.cpu().numpy().reshape(U.shape) for a in after]
        side.synchronize()
        op.close()
    return out, (t, dt, bad), st, after


def _assert_stats_equal(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("interval", [2, 3])
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK3_SSP], ids=["forwardEuler", "rk3"])
def test_sampling_leaves_the_solution_alone_nr_outlet(monkeypatch, integrator, interval):
    """Odd numbers of Mults per step and non-reflecting faces: the graph holds two steps.  After the first plain step the
    pairs end at steps 3, 5, 7.  interval 2: the samples after steps 2, 4, 6 fall inside a pair, the one after step 8
    follows the odd remainder.  interval 3: the sample after step 3 is at a pair's end, the one after step 6 inside one."""
    c, U = _nr_outlet_case(2)
    args = (c, U, integrator, 8, False, 2.0e-5, 0.12, 0.05)
    cfg = dict(sample_interval=interval, start_iter=0, iter0=0)
    xg, sg, stg, _ = _on_side_stream(monkeypatch, GRAPH, *args, stats=cfg)
    xl, sl, stl, _ = _on_side_stream(monkeypatch, LOOP, *args, stats=cfg)
    xg0, sg0, _, _ = _on_side_stream(monkeypatch, GRAPH, *args)
    xl0, sl0, _, _ = _on_side_stream(monkeypatch, LOOP, *args)
    assert np.isfinite(xg).all() and sg[2] == 0
    assert np.array_equal(xg, xg0) and sg == sg0 and np.array_equal(xl, xl0) and sl == sl0
    assert np.array_equal(xg, xl) and sg == sl
    _assert_stats_equal(stg, stl)
    assert stg[2] == stg[3] == 8 // interval and stg[4] == 8
    assert np.isfinite(stg[0]).all() and np.isfinite(stg[1]).all() and stg[1].any()


def test_sampling_leaves_the_trace_chain_alone_rk4(monkeypatch):
    """RK4 without forcing chains its traces from step to step (ta_chain): the sample between two steps reads x only.
    The fused / graph run equals the run with every stage's own trace sweep, one launch loop and one sweep direction."""
    c, state, _ = _case("dry_air")
    U = state(2)
    args = (c, U, capi.RK4, 7, False, 2.0e-5, 0.12, 0.05)
    cfg = dict(sample_interval=2, start_iter=0, iter0=0)
    xf, sf, stf, _ = _on_side_stream(monkeypatch, FUSED, *args, stats=cfg)
    xp, sp, stp, _ = _on_side_stream(monkeypatch, PLAIN, *args, stats=cfg)
    xf0, sf0, _, _ = _on_side_stream(monkeypatch, FUSED, *args)
    xp0, sp0, _, _ = _on_side_stream(monkeypatch, PLAIN, *args)
    assert np.isfinite(xf).all() and sf[2] == 0
    assert np.array_equal(xf, xf0) and sf == sf0 and np.array_equal(xp, xp0) and sp == sp0
    assert np.array_equal(xf, xp) and sf == sp
    _assert_stats_equal(stf, stp)
    assert stf[2] == stf[3] == 3 and stf[4] == 7


# ---- 4. the loop samples the right steps with the right states ------------------------------------------------------------
@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK3_SSP, capi.RK4], ids=["forwardEuler", "rk3", "rk4"])
def test_loop_samples_the_right_steps(monkeypatch, integrator):
    """iter0 = 10, interval 2, start 13: of the iterations 11 ... 17 only 14 and 16 are sampled -- steps 4 and 6 of the
    call.  The states come from a second run of the same steps, one per call in a plain launch loop, so the bound is the
    rounding bound of test 1 plus the time loop's own reproducibility bound (1e-13 of the row's scale, test_gpu_rk4.py)."""
    import torch

    c, state, nvel = _case("dry_air")
    U = state(2)
    args = (c, U, integrator, 7, True, 2.0e-5, 0.0, 0.0)
    xa, sa, sta, _ = _on_side_stream(monkeypatch, GRAPH, *args, stats=dict(sample_interval=2, start_iter=13, iter0=10))
    xb, sb, _, after = _on_side_stream(monkeypatch, LOOP, *args, per_call=1)
    assert len(after) == 7 and sa[2] == sb[2] == 0
    assert sta[2] == sta[3] == 2 and sta[4] == 17
    op = _operator(c)
    samples = [_prim_p(op, _device_state(op, after[k - 1])) for k in (4, 6)]
    torch.cuda.synchronize()
    op.close()
    _assert_within(sta[0], sta[1], samples, nvel, f"integrator {integrator}", extra_rel=1e-13)


# ---- 5. continuation ------------------------------------------------------------------------------------------------------
def test_continuation_and_restart_rms():
    c, state, nvel = _case("dry_air")

    def fresh():
        op = _operator(c)
        op.configureStatistics(1)
        return op

    one = fresh()
    xs = [_device_state(one, state(seed)) for seed in range(1, 5)]
    samples = [_prim_p(one, x) for x in xs]
    for x in xs:
        one.addSample(x)
    whole = _stats(one)
    one.close()

    first = fresh()
    for x in xs[:2]:
        first.addSample(x)
    mean, vari, nm, nv, _ = first.getStatistics()
    assert (nm, nv) == (2, 2)
    second = fresh()
    second.setStatistics(mean, vari, nm, nv, iter0=40)
    first.close()
    for x in xs[2:]:
        second.addSample(x)
    cont = _stats(second)
    assert np.array_equal(cont[0], whole[0]) and np.array_equal(cont[1], whole[1]) and cont[2:4] == (4, 4) and cont[4] == 40

    # restartRMS: the covariances start again, the mean goes on.  With ns_vari = 0 the recurrence gives
    # vari = d_i d_j / 1 with d against the mean of all three samples -- not 0: the mean has a history
    second.setStatistics(mean, None, nm)
    got = _stats(second)
    assert got[2:4] == (2, 0) and not got[1].any() and np.array_equal(got[0], mean.cpu().numpy())
    second.addSample(xs[2])
    got = _stats(second)
    second.close()
    assert got[2:4] == (3, 1)
    ref = su.Statistics(mean.shape[0], mean.shape[1], nvel, mean=mean.cpu().numpy(), vari=vari.cpu().numpy(), ns_mean=2, ns_vari=2)
    ref.restart_rms()
    ref.add(*samples[2])
    mean_b, vari_b = su.bounds(samples[:3], nvel)
    assert (np.abs(got[0] - ref.mean).max(axis=1) <= mean_b).all()
    assert (np.abs(got[1] - ref.vari).max(axis=1) <= vari_b).all()


# ---- 6. status codes ------------------------------------------------------------------------------------------------------
def test_status_codes():
    from tps_amd.rhs_operator import TpsRhsError

    lib = capi.load()
    c, state, _ = _case("dry_air")
    op = _operator(c)
    x = _device_state(op, state(1))
    U = x.cpu().numpy()
    nm, nv, it, n = C.c_int(7), C.c_int(7), C.c_int64(7), C.c_int(7)

    def all_refuse(where):
        for name, call in (("add_sample", lambda: lib.tpsrhs_stats_add_sample(op._h, C.c_void_p(x.data_ptr()))),
                           ("get", lambda: lib.tpsrhs_stats_get(op._h, None, None, C.byref(nm), C.byref(nv), C.byref(it))),
                           ("set", lambda: lib.tpsrhs_stats_set(op._h, C.c_void_p(x.data_ptr()), None, 1, 0)),
                           ("set_iter", lambda: lib.tpsrhs_stats_set_iter(op._h, 3)),
                           ("num_variances", lambda: lib.tpsrhs_stats_num_variances(op._h, C.byref(n)))):
            assert call() == capi.ERR_INVALID_ARGUMENT, (where, name)
            msg = lib.tpsrhs_last_error().decode()
            assert "tpsrhs_stats_" + name in msg and "not configured" in msg, (where, msg)
        assert (nm.value, nv.value, it.value, n.value) == (7, 7, 7, 7)  # nothing was written
        for f in (lambda: op.addSample(x), op.getStatistics, lambda: op.setStatistics(x, None, 1)):
            with pytest.raises(TpsRhsError) as e:
                f()
            assert e.value.status == capi.ERR_INVALID_ARGUMENT

    all_refuse("before configure")
    op.configureStatistics(2)
    op.addSample(x)
    for interval, start in ((-1, 0), (2, -1)):
        assert lib.tpsrhs_stats_configure(op._h, interval, start, 1) == capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_stats_set_iter(op._h, -1) == capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_stats_set(op._h, None, None, 1, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.tpsrhs_stats_set(op._h, C.c_void_p(x.data_ptr()), None, -1, 0) == capi.ERR_INVALID_ARGUMENT
    assert _stats(op)[2:] == (1, 1, 0)  # the refused calls changed nothing
    op.configureStatistics(0)
    all_refuse("after configure(0)")
    # the time loop of an operator without statistics is the loop it was
    t, dt, bad = op.advance(x, 0.0, 1e-7, 2, True)
    assert bad == 0 and dt == 1e-7 and not np.array_equal(x.cpu().numpy(), U)
    op.close()
