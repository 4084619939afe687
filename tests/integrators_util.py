"""The reference's explicit integrators restated in numpy over ``Oracle.mult``: what ``tpsrhs_step`` and
``tpsrhs_advance_with`` are tested against.

The schemes are MFEM's (``linalg/ode.cpp``, third party, MFEM >= 4.4: ForwardEulerSolver, RK2Solver(1.0), RK3SSPSolver,
RK4Solver), which ``M2ulPhyS`` builds from ``time/integrator`` (``src/M2ulPhyS.cpp:721-739, 2722-2736``), written in
MFEM's order of operations, one numpy expression per MFEM vector operation:

    forward Euler   k = f(x);  x = x + dt*k
    RK2(a = 1)      k = f(x);  x1 = x + (dt/2)*k;  y = x + dt*k;  k = f(y);  x = x1 + (dt/2)*k
    RK3-SSP         k = f(x);  y = x + dt*k
                    k = f(y);  y = y + dt*k;  y = (3/4)*x + (1/4)*y
                    k = f(y);  y = y + dt*k;  x = (1/3)*x + (2/3)*y

``step`` is ``timeIntegrator->Step(*U, time, dt); Check_NAN(); Check_Undershoot();`` of ``M2ulPhyS::solveStep``
(``src/M2ulPhyS.cpp:2004-2008``): the census, then the clamp of the species rows, once, on the final state; ``advance``
is the loop around it with ``dt = CFL hmin / max_char_speed / dim`` (``:2013-2016``).  The oracle's non-reflecting
boundary state advances by the ``dt`` of ``set_dt`` in every ``mult``, as the reference's does in every ``Mult``.
"""
import numpy as np

from tps_amd import capi


def forward_euler(f, x, dt):
    k = f(x)
    return x + dt * k


def rk2(f, x, dt):
    k = f(x)
    x1 = x + (dt / 2) * k
    y = x + dt * k
    k = f(y)
    return x1 + (dt / 2) * k


def rk3_ssp(f, x, dt):
    k = f(x)
    y = x + dt * k
    k = f(y)
    y = y + dt * k
    y = (3 / 4) * x + (1 / 4) * y
    k = f(y)
    y = y + dt * k
    return (1 / 3) * x + (2 / 3) * y


def rk4(f, x, dt):
    k = f(x)
    y = x + (dt / 2) * k
    z = x + (dt / 6) * k
    k = f(y)
    y = x + (dt / 2) * k
    z = z + (dt / 3) * k
    k = f(y)
    y = x + dt * k
    z = z + (dt / 3) * k
    k = f(y)
    return z + (dt / 6) * k


SCHEMES = {capi.FORWARD_EULER: forward_euler, capi.RK2: rk2, capi.RK3_SSP: rk3_ssp, capi.RK4: rk4}
ORDER = {capi.FORWARD_EULER: 1, capi.RK2: 2, capi.RK3_SSP: 3, capi.RK4: 4}
NAMES = {capi.FORWARD_EULER: "forwardEuler", capi.RK2: "rk2", capi.RK3_SSP: "rk3", capi.RK4: "rk4"}


def num_active_species(physics):
    if physics.working_fluid != capi.USER_DEFINED:
        return 0
    return physics.mixture.num_species - (2 if physics.mixture.ambipolar else 1)


def species_rows(o):
    """the rows Check_Undershoot clamps: nvel + 2 ... nvel + 2 + numActiveSpecies"""
    nvel = 3 if o.disc.axisymmetric else o.dim
    return slice(nvel + 2, nvel + 2 + num_active_species(o.physics))


def census_then_clamp(o, x):
    """Check_NAN, then Check_Undershoot, on the final state of a step -> (state, NaN count)"""
    bad = int(np.isnan(x).sum())
    x = x.copy()
    rows = species_rows(o)
    x[rows] = np.maximum(x[rows], 0.0)
    return x, bad


def step(o, integrator, x, time, dt, clamp=True):
    """-> (new x, new time, max_char_speed of the step's last mult, NaN count); clamp=False: the state before
    Check_Undershoot"""
    o.set_dt(dt)
    xn = SCHEMES[integrator](o.mult, np.array(x, dtype=np.float64), dt)
    speed = o.max_char_speed
    bad = int(np.isnan(xn).sum())
    if clamp:
        xn, bad = census_then_clamp(o, xn)
    return xn, time + dt, speed, bad


def advance(o, integrator, x, time, dt, num_steps, constant_dt=True, cfl=0.0, hmin=0.0):
    """the host loop -> (new x, time, next dt, NaN count of all steps)"""
    bad = 0
    for _ in range(num_steps):
        x, time, speed, b = step(o, integrator, x, time, dt)
        bad += b
        if not constant_dt:
            dt = cfl * hmin / speed / o.dim
    return x, time, dt, bad


def order_case():
    """the setup of test_time_loop_is_fourth_order_in_dt: (mesh, disc, physics, U, t_end)"""
    from tps_amd import cases, meshgen
    from tps_amd.rhs_operator import node_coordinates

    mesh = meshgen.box_hex(3, 3, 3, lengths=(1.0, 0.8, 1.2), warp=0.05)
    ph = capi.dry_air_physics(capi.NS, visc_mult=2.0e3)
    U = cases.dry_air_state(node_coordinates(mesh, 2), seed=5)
    return mesh, capi.Disc(2, 0, 0, 0, 0), ph, U, 4.0e-4


def observed_orders(run, reference):
    """run(nsteps) -> state; the two observed orders from 10 / 20 / 40 steps against `reference`"""
    e1, e2, e3 = (np.abs(run(n) - reference).max() for n in (10, 20, 40))
    return np.log2(e1 / e2), np.log2(e2 / e3), (e1, e2, e3)
