"""The yardstick of tests/test_gpu_integrators.py, pinned on the CPU: the numpy restatements of forward Euler, RK2 and
RK3-SSP over the oracle's Mult (tests/integrators_util.py) converge at the order of their scheme.

The setup is that of test_gpu_rk4.test_time_loop_is_fourth_order_in_dt: the spatial operator is the same in all runs,
so the differences between them are purely temporal.  Runs of 10 / 20 / 40 steps against 160 steps of the RK4
restatement; the window is that test's, +-0.4 around the order.  Observed: Euler 1.20 / 1.10, RK2 1.79 / 1.89,
RK3 3.05 / 3.03 (RK4 itself: 3.89 / 3.95)."""
import numpy as np
import pytest

import integrators_util as iu
from oracle_lib import Oracle
from tps_amd import capi

_CACHE = {}


def _setup():
    if not _CACHE:
        mesh, disc, ph, U, t_end = iu.order_case()
        o = Oracle(mesh, disc, ph, [])
        ref, t, _, bad = iu.advance(o, capi.RK4, U, 0.0, t_end / 160, 160)
        assert bad == 0 and t == pytest.approx(t_end, rel=1e-12)
        _CACHE.update(o=o, U=U, t_end=t_end, ref=ref)
    return _CACHE["o"], _CACHE["U"], _CACHE["t_end"], _CACHE["ref"]


@pytest.mark.parametrize("integrator", [capi.FORWARD_EULER, capi.RK2, capi.RK3_SSP, capi.RK4], ids=lambda i: iu.NAMES[i])
def test_restatement_converges_at_the_order_of_its_scheme(integrator):
    o, U, t_end, ref = _setup()

    def run(nsteps):
        x, t, _, bad = iu.advance(o, integrator, U, 0.0, t_end / nsteps, nsteps)
        assert bad == 0 and t == pytest.approx(t_end, rel=1e-12)
        return x

    p1, p2, errs = iu.observed_orders(run, ref)
    print(iu.NAMES[integrator], "errors", errs, "orders", p1, p2)
    order = iu.ORDER[integrator]
    assert order - 0.4 < p1 < order + 0.4 and order - 0.4 < p2 < order + 0.4


def test_rk4_restatement_is_the_oracle_s_rk4_step():
    """the restatement's RK4 (the reference of the orders above) against the oracle's own tpsoracle_rk4_step"""
    o, U, t_end, _ = _setup()
    dt = t_end / 10
    mine, t1, s1, b1 = iu.step(o, capi.RK4, U, 0.0, dt)
    theirs, t2, s2, b2 = o.rk4_step(U, 0.0, dt)
    assert t1 == t2 and b1 == b2 == 0 and s1 == pytest.approx(s2, rel=1e-14)
    scale = np.abs(U).max(axis=1, keepdims=True)
    assert (np.abs(mine - theirs) <= 4 * np.finfo(np.float64).eps * scale).all()
