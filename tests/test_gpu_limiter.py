"""The conservative positivity limiter on the device (tpsrhs_limiter_weights, tpsrhs_limit; tps_amd/csrc/limiter.hip) against
the numpy restatement of tests/limiter_util.py: the weights, one application with all four outcomes of the row step, the
conservation of every element integral, bounds and idempotence, the pressure step of dry air, the default rows of the
mixtures, NaN elements.  Every mesh is warped or carries a radial weight, so that the weights vary inside an element, and
every element count is odd, so that the last block of k_limit is partial.  The node counts 4, 9, 16 (2-D p = 1 .. 3) and 27,
64, 216 (3-D p = 2, 3, 5) cross the sub-wave groups of 4, 16 and 32 lanes, the full wave and two / four values per lane."""
import functools

import numpy as np
import pytest

import integrals_util as iu
import limiter_util as lu
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
EPS = lu.EPS
LD = np.longdouble


def _walls(mesh):
    return [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]


@functools.lru_cache(maxsize=None)
def _case(kind, order, basis):
    if kind == "quad":
        mesh, ph, axi = meshgen.box_quad(7, 3, warp=0.1), capi.dry_air_physics(capi.EULER), 0
    elif kind == "hex":
        mesh, ph, axi = meshgen.box_hex(3, 3, 3, warp=0.1), capi.dry_air_physics(capi.EULER), 0
    elif kind == "annulus":
        mesh, ph, axi = meshgen.annulus_quad(5, 3), capi.dry_air_physics(capi.EULER), 1
    elif kind == "ternary":
        mesh, ph, axi = meshgen.box_quad(5, 3, warp=0.1), capi.argon_ternary_physics(), 0
    else:
        assert kind == "six2t"
        mesh, ph, axi = meshgen.box_quad(5, 3, warp=0.1), capi.argon_six_species_physics(), 0
    return cases.Case(f"limiter_{kind}", mesh, capi.Disc(order, basis, basis, axi, 0), ph, _walls(mesh))


DRY_AIR = [("quad", 1, 0), ("quad", 2, 0), ("quad", 3, 0), ("quad", 1, 1), ("quad", 2, 1), ("quad", 3, 1),
           ("hex", 2, 0), ("hex", 3, 0), ("hex", 5, 0), ("hex", 3, 1), ("annulus", 2, 0)]
MIXTURES = [("ternary", 2, 0), ("six2t", 2, 0)]
ALL = DRY_AIR + MIXTURES


def _id(k):
    return f"{k[0]}_p{k[1]}_{'lobatto' if k[2] else 'legendre'}"


def _operator(c):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs)


def _dev(op, a):
    import torch

    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=op.device)


def _npe(c):
    return (c.disc.order + 1) ** c.mesh.dim


@functools.lru_cache(maxsize=None)
def _reference_weights(key):
    c = _case(*key)
    W, A = lu.weights(c.mesh, c.disc.order, c.disc.basis_type, radial=bool(c.disc.axisymmetric))
    W.setflags(write=False)
    A.setflags(write=False)
    return W, A


@functools.lru_cache(maxsize=None)
def _device_weights(key):
    """limiterWeights() of the case, fetched once: what the restatement of the operation is given (test 1 pins them)"""
    op = _operator(_case(*key))
    w = op.limiterWeights().cpu().numpy()
    op.close()
    w.setflags(write=False)
    return w


def _nvel(c):
    return 3 if c.disc.axisymmetric else c.mesh.dim


def _synthetic(key, rows, floors, with_clamped=True, seed=5):
    """a dry-air state (nvel + 2, NDofs): the listed rows carry the four outcomes element by element, the others random numbers"""
    c = _case(*key)
    neq = _nvel(c) + 2
    rng = np.random.default_rng(seed)
    ne, npe = c.mesh.num_elements, _npe(c)
    x = rng.standard_normal((neq, ne * npe))
    v, kinds = lu.four_outcome_rows(rng, ne, npe, len(rows), floors, with_clamped)
    for i, r in enumerate(rows):
        x[r] = v[i]
    return x, kinds


def _tolerance(x_rows, npe):
    """100 N eps max|v| per element and row, broadcast to the nodes: the mean carries at most N eps relative error and theta
    amplifies it by at most max|v| / (mean - m) <= 10 (the construction, asserted in the test)"""
    vmax = np.abs(x_rows.reshape(x_rows.shape[0], -1, npe)).max(axis=2, keepdims=True)
    return np.broadcast_to(100 * npe * EPS * vmax, (x_rows.shape[0], vmax.shape[1], npe)).reshape(x_rows.shape[0], -1)


# ---- 1. weights -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL, ids=_id)
def test_weights_match_the_rule_of_integrate(key):
    import torch

    c = _case(*key)
    p, dim = c.disc.order, c.mesh.dim
    W, A = _reference_weights(key)
    op = _operator(c)
    w = op.limiterWeights()
    rng = np.random.default_rng(21)
    f = rng.standard_normal((1, op.NDofs))
    total = op.integrate(_dev(op, f))[0].cpu().numpy()[0]
    op.close()
    got = w.cpu().numpy()
    # per node: the error model of tpsrhs_integrate's contract applied to one basis function
    bound = ((p + 2) ** dim + 8 * dim * (p + 1)) * EPS * A.astype(np.float64)
    err = np.abs(got.astype(LD) - W).astype(np.float64)
    print(f"{_id(key)}: max |W - ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # sum_n W_n f_n against integrate(f), within that contract's stated bound (the weights' own error is inside it: K holds
    # the terms of one basis function and ne more)
    ref = iu.integrate(c.mesh, p, c.disc.basis_type, f, radial=bool(c.disc.axisymmetric))
    dot = float((got.astype(LD) * f[0].astype(LD)).sum())
    print(f"{_id(key)}: |W.f - integrate(f)| / (eps S1) = {abs(dot - total) / (EPS * ref['S1'][0]):.3f} (bound {ref['K']})")
    assert abs(dot - total) <= ref["K"] * EPS * ref["S1"][0]
    if c.disc.basis_type == 0:
        assert (got > 0.0).all()
    assert torch.isfinite(w).all()


# ---- 2. one application, 3. conservation, 4. bounds and idempotence ------------------------------------------------------------
@pytest.mark.parametrize("key", DRY_AIR, ids=_id)
def test_one_application_matches_the_restatement_and_conserves(key):
    import torch

    c = _case(*key)
    npe, nvel = _npe(c), _nvel(c)
    rows, floors = [0, nvel + 1], [0.25, -0.5]
    x, kinds = _synthetic(key, rows, floors)
    w = _device_weights(key)
    ref = lu.limit(x, w, npe, rows, floors)
    assert all((ref["outcome"] == k).any() for k in (lu.UNTOUCHED, lu.SCALED, lu.CLAMPED))
    # the construction the tolerance rests on: where outcome 3 occurs, mean - m >= 0.1 max|v|
    for i, r in enumerate(rows):
        v = x[r].reshape(-1, npe)
        s = ref["outcome"][i] == lu.SCALED
        assert ((ref["mean"][i] - v.min(axis=1))[s] >= 0.1 * np.abs(v).max(axis=1)[s]).all()
    op = _operator(c)
    xd = _dev(op, x)
    before = op.integrate(xd)[0].cpu().numpy()
    op.limit(xd, rows, floors)
    rep = op.readLimiter(reset=True)
    got = xd.cpu().numpy()
    after = op.integrate(xd)[0].cpu().numpy()
    # 4. a second application changes no bit and counts nothing
    op.limit(xd, rows, floors)
    rep2 = op.readLimiter()
    again = xd.cpu().numpy()
    op.close()
    # 2. against the restatement; untouched elements and unlisted rows bit-equal; the counters exactly
    tol = _tolerance(x[rows], npe)
    err = np.abs(got[rows] - ref["x"][rows])
    print(f"{_id(key)}: max |device - numpy| / (100 N eps max|v|) = {(err / tol).max():.4f}")
    assert (err <= tol).all()
    untouched = np.repeat(ref["outcome"] == lu.UNTOUCHED, npe, axis=1)
    assert np.array_equal(got[rows][untouched], x[rows][untouched])
    others = [r for r in range(x.shape[0]) if r not in rows]
    assert np.array_equal(got[others], x[others])
    assert rep["calls"] == 1 and rep["pressure_limited"] == 0 and rep["pressure_unfixable"] == 0
    assert np.array_equal(rep["limited"], ref["limited"]) and np.array_equal(rep["clamped"], ref["clamped"])
    # 4. every listed row >= its floor everywhere
    for r, f in zip(rows, floors):
        assert (got[r] >= f).all()
    assert np.array_equal(again, got)
    assert rep2["calls"] == 1 and rep2["limited"].sum() == 0 and rep2["clamped"].sum() == 0
    # 3. per element of outcome 3: sum W v before and after within (N + 4) eps sum W |v|
    moved = np.zeros(len(rows), dtype=LD)
    slack = np.zeros(len(rows))
    for i, r in enumerate(rows):
        a, b = lu.element_integrals(w, got[r], npe), lu.element_integrals(w, x[r], npe)
        s1 = lu.element_integrals(w, np.abs(x[r]), npe).astype(np.float64)
        sc = ref["outcome"][i] == lu.SCALED
        drift = np.abs(a - b).astype(np.float64)
        print(f"{_id(key)} row {r}: max element drift / (eps sum W|v|) = {(drift[sc] / (EPS * s1[sc])).max():.3f} (bound {npe + 4})")
        assert (drift[sc] <= (npe + 4) * EPS * s1[sc]).all()
        cl = ref["outcome"][i] == lu.CLAMPED
        # with clamped elements the total moves by the amount numpy predicts for them
        moved[i] = (lu.element_integrals(w, ref["x"][r], npe) - b)[cl].sum()
        slack[i] = ((npe + 4) * EPS * s1[sc]).sum() + (npe * EPS * s1[cl]).sum()
    radial = bool(c.disc.axisymmetric)
    rb = iu.integrate(c.mesh, c.disc.order, c.disc.basis_type, x[rows], radial=radial)
    ra = iu.integrate(c.mesh, c.disc.order, c.disc.basis_type, got[rows], radial=radial)
    bound = rb["K"] * EPS * (rb["S1"] + ra["S1"]) + slack
    change = (after[rows] - before[rows]) - moved.astype(np.float64)
    print(f"{_id(key)}: |total change - predicted| / bound = {np.abs(change) / bound}")
    assert (np.abs(change) <= bound).all()
    assert (np.abs(moved.astype(np.float64)) > 1000 * bound).all()  # the clamp's drift is far outside the rounding


@pytest.mark.parametrize("key", DRY_AIR, ids=_id)
def test_totals_are_kept_when_no_element_is_clamped(key):
    c = _case(*key)
    npe, nvel = _npe(c), _nvel(c)
    rows, floors = [0, nvel + 1], [0.25, -0.5]
    x, _ = _synthetic(key, rows, floors, with_clamped=False, seed=6)
    op = _operator(c)
    xd = _dev(op, x)
    before = op.integrate(xd)[0].cpu().numpy()
    op.limit(xd, rows, floors)
    rep = op.readLimiter()
    after = op.integrate(xd)[0].cpu().numpy()
    got = xd.cpu().numpy()
    op.close()
    assert rep["clamped"].sum() == 0 and rep["limited"][rows].min() > 0
    radial = bool(c.disc.axisymmetric)
    rb = iu.integrate(c.mesh, c.disc.order, c.disc.basis_type, x, radial=radial)
    ra = iu.integrate(c.mesh, c.disc.order, c.disc.basis_type, got, radial=radial)
    bound = rb["K"] * EPS * (rb["S1"] + ra["S1"])  # the sum of the two documented bounds
    print(f"{_id(key)}: |after - before| / bound = {np.abs(after - before) / bound}")
    assert (np.abs(after - before) <= bound).all()
    # ... where the clamp max(v, floor) would have moved the total far outside them
    for r, f in zip(rows, floors):
        clamp = iu.integrate(c.mesh, c.disc.order, c.disc.basis_type, np.maximum(x[r], f)[None], radial=radial)["sum"][0]
        assert abs(clamp - rb["sum"][r]) > 1000 * bound[r]


# ---- 5. pressure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", DRY_AIR, ids=_id)
def test_pressure_step_of_dry_air(key):
    c = _case(*key)
    npe, nvel, ne = _npe(c), _nvel(c), c.mesh.num_elements
    gamma = c.physics.dry_air.specific_heat_ratio
    rng = np.random.default_rng(9)
    n = ne * npe
    # rho ~ 1, momenta ~ 0.1, p ~ 1; element e % 3 == 1: one node with p = 0.05 (a dip the scaling repairs);
    # e % 3 == 2: every node at p ~ 0.1 (the mean pressure below the floor: unfixable)
    rho = 1.0 + 0.1 * rng.random(n)
    mom = 0.1 * rng.standard_normal((nvel, n))
    p = (1.0 + 0.2 * rng.random(n)).reshape(ne, npe)
    e = np.arange(ne)
    p[e % 3 == 2] = 0.1 + 0.02 * rng.random(((e % 3 == 2).sum(), npe))
    dip = np.where(e % 3 == 1)[0]
    p[dip, rng.integers(npe, size=dip.size)] = 0.05
    x = np.zeros((nvel + 2, n))
    x[0], x[1:nvel + 1] = rho, mom
    x[nvel + 1] = p.reshape(-1) / (gamma - 1.0) + 0.5 * (mom * mom).sum(axis=0) / rho
    fp, rows, floors = 0.5, [0], [0.5]
    w = _device_weights(key)
    ref = lu.limit(x, w, npe, rows, floors, fp, nvel, gamma)
    assert all((ref["p_outcome"] == k).any() for k in (lu.P_UNTOUCHED, lu.P_SCALED, lu.P_UNFIXABLE))
    op = _operator(c)
    xd = _dev(op, x)
    op.limit(xd, rows, floors, pressure_floor=fp)
    rep = op.readLimiter()
    got = xd.cpu().numpy()
    op.close()
    assert rep["pressure_limited"] == ref["pressure_limited"] and rep["pressure_unfixable"] == ref["pressure_unfixable"]
    assert rep["limited"].sum() == 0 and rep["clamped"].sum() == 0
    pg = lu.pressure(got, nvel, gamma).reshape(ne, npe)
    fixable = ref["p_outcome"] != lu.P_UNFIXABLE
    print(f"{_id(key)}: min p / f_p on the fixable elements = {pg[fixable].min() / fp:.15f}")
    assert (pg[fixable] >= fp * (1.0 - 1e-12)).all()
    assert (got[0] >= floors[0]).all()
    same = np.repeat(ref["p_outcome"] != lu.P_SCALED, npe)
    assert np.array_equal(got[:, same], x[:, same])
    sc = ref["p_outcome"] == lu.P_SCALED
    for r in range(nvel + 2):  # all row means are kept
        a, b = lu.element_integrals(w, got[r], npe), lu.element_integrals(w, x[r], npe)
        s1 = lu.element_integrals(w, np.abs(x[r]), npe).astype(np.float64)
        assert (np.abs(a - b).astype(np.float64)[sc] <= (npe + 4) * EPS * s1[sc]).all()
    tol = 100 * npe * EPS * np.abs(x).reshape(nvel + 2, ne, npe).max(axis=2, keepdims=True)  # theta's denominator is >= 0.3 pbar here
    assert (np.abs(got - ref["x"]).reshape(nvel + 2, ne, npe) <= tol).all()


# ---- 6. default rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MIXTURES, ids=_id)
def test_default_rows_are_the_species_rows(key):
    c = _case(*key)
    npe, nvel = _npe(c), _nvel(c)
    nsp = c.physics.mixture.num_species - (2 if c.physics.mixture.ambipolar else 1)
    sp = list(range(nvel + 2, nvel + 2 + nsp))
    op = _operator(c)
    neq = op.num_equation
    assert neq == nvel + 2 + nsp + (1 if c.physics.mixture.two_temperature else 0)
    rng = np.random.default_rng(13)
    x = rng.standard_normal((neq, op.NDofs))  # every row dips below 0 in every element
    v, _ = lu.four_outcome_rows(rng, c.mesh.num_elements, npe, nsp, [0.0] * nsp)
    x[sp] = v
    w = op.limiterWeights().cpu().numpy()
    ref = lu.limit(x, w, npe, sp, [0.0] * nsp)
    xd = _dev(op, x)
    op.limit(xd)  # num_rows = -1
    rep = op.readLimiter()
    got = xd.cpu().numpy()
    op.close()
    others = [r for r in range(neq) if r not in sp]
    assert np.array_equal(got[others], x[others])  # with the electron energy of the two-temperature mixture, bit for bit
    assert (got[sp] >= 0.0).all()
    assert np.array_equal(rep["limited"], ref["limited"]) and np.array_equal(rep["clamped"], ref["clamped"])
    assert rep["limited"][others].sum() == 0 and rep["clamped"][others].sum() == 0 and rep["limited"][sp].min() > 0
    assert (np.abs(got[sp] - ref["x"][sp]) <= _tolerance(x[sp], npe)).all()


# ---- 7. NaN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", DRY_AIR, ids=_id)
def test_a_nan_node_leaves_its_element_untouched(key):
    c = _case(*key)
    npe, nvel = _npe(c), _nvel(c)
    rows, floors = [0, nvel + 1], [0.25, -0.5]
    x, kinds = _synthetic(key, rows, floors)
    bad = [1, 2, 6]  # elements that would have been scaled / clamped in one row or the other
    for e in bad:
        x[0, e * npe + (e % npe)] = np.nan
    w = _device_weights(key)
    ref = lu.limit(x, w, npe, rows, floors)
    assert (ref["outcome"][0][bad] == lu.NAN).all()
    op = _operator(c)
    xd = _dev(op, x)
    op.limit(xd, rows, floors)
    rep = op.readLimiter()
    got = xd.cpu().numpy()
    op.close()
    for e in bad:
        assert np.array_equal(got[0, e * npe:(e + 1) * npe], x[0, e * npe:(e + 1) * npe], equal_nan=True)
    assert np.array_equal(rep["limited"], ref["limited"]) and np.array_equal(rep["clamped"], ref["clamped"])
    ok = ~np.isnan(ref["x"][rows])
    assert np.array_equal(np.isnan(got[rows]), ~ok)
    assert (np.abs(got[rows] - ref["x"][rows])[ok] <= _tolerance(np.nan_to_num(x[rows]), npe)[ok]).all()
    untouched = np.repeat(ref["outcome"] == lu.UNTOUCHED, npe, axis=1)
    assert np.array_equal(got[rows][untouched], x[rows][untouched])


# ---- the refusals through the C ABI, on real operators --------------------------------------------------------------------
def _refused(status, fragment, call):
    """call() returns a status of the C ABI: the expected one, with `fragment` in tpsrhs_last_error"""
    lib = capi.load()
    st = call()
    msg = lib.tpsrhs_last_error().decode()
    assert st == status and fragment in msg, (st, msg)


def test_refusals_through_the_c_abi():
    """NULL arguments (limiter.hip), and the plan's refusals with the facts of real operators: dry air, the ambipolar ternary
    mixture, the six-species two-temperature mixture.  Nothing is counted and no bit of x moves."""
    import ctypes as C

    from tps_amd.rhs_operator import TpsRhsError

    lib = capi.load()
    INVALID, UNSUPPORTED = capi.ERR_INVALID_ARGUMENT, capi.ERR_UNSUPPORTED
    op = _operator(_case("quad", 2, 0))
    x0 = np.random.default_rng(3).standard_normal((op.num_equation, op.NDofs)) - 2.0
    xd = _dev(op, x0)
    xp, lim, rep = C.c_void_p(xd.data_ptr()), capi.make_limiter([0], 0.1), capi.LimiterReport()
    _refused(INVALID, "tpsrhs_limit", lambda: lib.tpsrhs_limit(None, C.byref(lim), xp))
    _refused(INVALID, "tpsrhs_limit", lambda: lib.tpsrhs_limit(op._h, C.byref(lim), None))
    _refused(INVALID, "tpsrhs_limit", lambda: lib.tpsrhs_limit(op._h, None, xp))
    _refused(INVALID, "tpsrhs_limiter_weights", lambda: lib.tpsrhs_limiter_weights(None, xp))
    _refused(INVALID, "tpsrhs_limiter_weights", lambda: lib.tpsrhs_limiter_weights(op._h, None))
    _refused(INVALID, "tpsrhs_limiter_configure", lambda: lib.tpsrhs_limiter_configure(None, C.byref(lim)))
    _refused(INVALID, "tpsrhs_limiter_read", lambda: lib.tpsrhs_limiter_read(None, C.byref(rep), 0))
    _refused(INVALID, "tpsrhs_limiter_read", lambda: lib.tpsrhs_limiter_read(op._h, None, 0))
    for kw, fragment in ((dict(rows=[4]), "outside"), (dict(rows=[-1]), "outside"), (dict(rows=[1, 1]), "twice"),
                         (dict(rows=[0], floors=[float("nan")]), "NaN"), (dict(rows=[0], floors=0.1, pressure_floor=-1.0), "pressure_floor"),
                         (dict(rows=[0], floors=0.1, pressure_floor=float("nan")), "pressure_floor"),
                         (dict(rows=[3], floors=0.1, pressure_floor=1.0), "row 0"),
                         (dict(rows=[0], floors=0.0, pressure_floor=1.0), "row 0")):
        for call in (lambda: op.limit(xd, **kw), lambda: op.configureLimiter(**kw)):
            with pytest.raises(TpsRhsError) as e:
                call()
            assert e.value.status == INVALID and fragment in str(e.value), str(e.value)
    for n in (-2, op.num_equation + 1):
        bad = capi.make_limiter([0], 0.1)
        bad.num_rows = n
        _refused(INVALID, "num_rows", lambda: lib.tpsrhs_limit(op._h, C.byref(bad), xp))
    op.limit(xd)  # num_rows = -1 on dry air: a valid, empty limiter
    r = op.readLimiter()
    assert r["calls"] == 1 and r["limited"].sum() == 0 and r["clamped"].sum() == 0
    assert np.array_equal(xd.cpu().numpy(), x0)
    op.close()
    for kind, nsp in (("ternary", 1), ("six2t", 5)):
        op = _operator(_case(kind, 2, 0))
        xd = _dev(op, np.ones((op.num_equation, op.NDofs)))
        with pytest.raises(TpsRhsError) as e:
            op.limit(xd, [0], 0.1, pressure_floor=1.0)
        assert e.value.status == UNSUPPORTED and "dry air" in str(e.value)
        with pytest.raises(TpsRhsError) as e:
            op.configureLimiter([0], 0.1, pressure_floor=1.0)
        assert e.value.status == UNSUPPORTED
        if nsp > 1:  # some species rows but not all: refused in the loop, allowed in one application
            with pytest.raises(TpsRhsError) as e:
                op.configureLimiter([4, 6], 0.0)
            assert e.value.status == INVALID and "2 of the 5 species rows" in str(e.value)
            op.limit(xd, [4, 6], 0.0)
        op.configureLimiter()  # the default rows
        op.configureLimiter(off=True)
        assert op.readLimiter()["limited"].sum() == 0
        op.close()
