"""The Legendre modal filter and smoothness sensor on the device (tpsrhs_modal_transform, tpsrhs_modal_energy,
tpsrhs_modal_filter_apply; tps_amd/csrc/modal.hip) against closed forms and the long-double restatement of
tests/modal_util.py, within that module's error model (derived there, not tuned).  The cases are the limiter's table --
4 / 9 / 16 nodes (2-D p = 1 .. 3, both bases), 27 / 64 / 216 nodes (3-D p = 2, 3, 5), the axisymmetric annulus, the ternary
and the six-species two-temperature mixtures -- plus the unwarped quad and hex boxes; every element count is odd, so the
last block of every kernel is partial."""
import ctypes as C
import functools

import numpy as np
import pytest

import integrals_util as iu
import limiter_util as lu
import modal_util as mu
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu
EPS, LD = mu.EPS, mu.LD


def _walls(mesh):
    return [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]


@functools.lru_cache(maxsize=None)
def _case(kind, order, basis):
    if kind in ("quad", "quad_flat"):
        mesh, ph, axi = meshgen.box_quad(7, 3, warp=0.1 if kind == "quad" else 0.0), capi.dry_air_physics(capi.EULER), 0
    elif kind in ("hex", "hex_flat"):
        mesh, ph, axi = meshgen.box_hex(3, 3, 3, warp=0.1 if kind == "hex" else 0.0), capi.dry_air_physics(capi.EULER), 0
    elif kind == "annulus":
        mesh, ph, axi = meshgen.annulus_quad(5, 3), capi.dry_air_physics(capi.EULER), 1
    elif kind == "ternary":
        mesh, ph, axi = meshgen.box_quad(5, 3, warp=0.1), capi.argon_ternary_physics(), 0
    else:
        assert kind == "six2t"
        mesh, ph, axi = meshgen.box_quad(5, 3, warp=0.1), capi.argon_six_species_physics(), 0
    return cases.Case(f"modal_{kind}", mesh, capi.Disc(order, basis, basis, axi, 0), ph, _walls(mesh))


WARPED = [("quad", 1, 0), ("quad", 2, 0), ("quad", 3, 0), ("quad", 1, 1), ("quad", 2, 1), ("quad", 3, 1),
          ("hex", 2, 0), ("hex", 3, 0), ("hex", 5, 0), ("hex", 3, 1)]
AXI = [("annulus", 2, 0)]
MIXTURES = [("ternary", 2, 0), ("six2t", 2, 0)]
FLAT = [("quad_flat", 2, 0), ("quad_flat", 3, 1), ("hex_flat", 2, 0), ("hex_flat", 3, 1)]
ALL = WARPED + AXI + MIXTURES + FLAT


def _id(k):
    return f"{k[0]}_p{k[1]}_{'lobatto' if k[2] else 'legendre'}"


def _operator(c):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs)


def _dev(op, a):
    import torch

    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device=op.device)


def _shape(key):
    c = _case(*key)
    dim, p = c.mesh.dim, c.disc.order
    return c, dim, p, c.disc.basis_type, (p + 1) ** dim, c.mesh.num_elements


@functools.lru_cache(maxsize=None)
def _device_weights(key):
    """limiterWeights() of the case, fetched once (tests/test_gpu_limiter.py pins them): what the restatement is given"""
    op = _operator(_case(*key))
    w = op.limiterWeights().cpu().numpy()
    op.close()
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _reference_weights(key):
    c = _case(*key)
    W, _ = lu.weights(c.mesh, c.disc.order, c.disc.basis_type, radial=bool(c.disc.axisymmetric))
    W.setflags(write=False)
    return W


def _within(name, got, ref, bound, floor=0.0):
    """|got - ref| <= bound + eps |ref| (the rounding of the long-double reference to double), printed before it is asserted"""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    tol = np.asarray(bound, dtype=LD) + LD(EPS) * np.abs(np.asarray(ref, dtype=LD)) + floor
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print(f"{name}: max |device - reference| / bound = {float(np.nanmax(ratio)):.4f}")
    assert (err <= tol).all(), name


# ---- 1. transform ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL, ids=_id)
def test_transform_forward_inverse_and_unit_modes(key):
    c, dim, p, basis, npe, ne = _shape(key)
    V, Vi = mu.matrices(p, basis)
    rng = np.random.default_rng(31)
    v = rng.standard_normal((3, ne * npe))
    # the tensor Legendre mode (e mod npe) sampled at the nodes of element e: its coefficients are that unit vector
    z = mu.node_coordinates_ref(p, basis, dim)
    modes = np.zeros((ne, npe), dtype=LD)
    for e in range(ne):
        m, val = e % npe, np.ones(npe, dtype=LD)
        for d in range(dim):
            val = val * mu.legendre((m // (p + 1) ** d) % (p + 1), z[d])
        modes[e] = val
    vm = modes.astype(np.float64)
    op = _operator(c)
    vd = _dev(op, v)
    fwd = op.modalTransform(vd)
    back = op.modalTransform(fwd, inverse=True)
    inplace = vd.clone()
    st = capi.load().tpsrhs_modal_transform(op._h, 0, 3, C.c_void_p(inplace.data_ptr()), C.c_void_p(inplace.data_ptr()))
    assert st == 0
    one_row = op.modalTransform(vd[1].contiguous())
    unit = op.modalTransform(_dev(op, vm.reshape(-1)))
    fwd, back, inplace, one_row, unit = (t.cpu().numpy() for t in (fwd, back, inplace, one_row, unit))
    op.close()
    vv = v.reshape(3, ne, npe)
    _within(f"{_id(key)} forward", fwd.reshape(vv.shape), mu.tensor_apply(Vi, vv, dim), mu.apply_bound(Vi, vv, dim))
    assert np.array_equal(inplace, fwd) and np.array_equal(one_row, fwd[1])
    # inverse(forward(v)) = v: the inverse's own bound on what it was given, and the forward's bound carried through |V|
    fw = fwd.reshape(vv.shape)
    carried = mu.tensor_apply(np.abs(V), mu.apply_bound(Vi, vv, dim), dim)
    _within(f"{_id(key)} inverse(forward)", back.reshape(vv.shape), vv, mu.apply_bound(V, fw, dim) + carried)
    # closed form: the unit vectors; the samples were rounded to double (half an ulp each, carried through |V^-1|)
    want = np.zeros((ne, npe))
    want[np.arange(ne), np.arange(ne) % npe] = 1.0
    rounding = mu.tensor_apply(np.abs(Vi), 0.5 * LD(EPS) * np.abs(modes), dim)
    _within(f"{_id(key)} unit modes", unit.reshape(ne, npe), want, mu.apply_bound(Vi, vm, dim) + rounding)


# ---- 2. filter against closed forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WARPED + AXI + FLAT, ids=_id)
def test_filter_against_closed_forms(key):
    c, dim, p, basis, npe, ne = _shape(key)
    n1 = p + 1
    V, _ = mu.matrices(p, basis)
    rng = np.random.default_rng(37)
    z = mu.node_coordinates_ref(p, basis, dim)
    alpha, s = 2.0, 2
    op = _operator(c)
    neq = op.num_equation
    shell, _ = mu.shells(p, dim)
    for kc in sorted({0, p - 1}):
        # row 0: degree <= k_c per direction, comes back as it is.  row 1: P_p along direction e mod dim, constant in the
        # others, comes back multiplied by sigma_p = exp(-alpha).  The other rows: not listed.
        coef = rng.standard_normal((ne, npe)).astype(LD)
        coef[:, shell > kc] = 0
        low = mu.tensor_apply(V, coef, dim)
        top = np.stack([(1 + e) * mu.legendre(p, z[e % dim]) for e in range(ne)])
        x = rng.standard_normal((neq, ne * npe))
        x[0], x[1] = low.astype(np.float64).reshape(-1), top.astype(np.float64).reshape(-1)
        xd = _dev(op, x)
        op.modalFilter(xd, rows=[0, 1], cutoff=kc, alpha=alpha, exponent=s, conservative=False)
        got = xd.cpu().numpy()
        F = mu.filter_matrix(p, basis, kc, alpha, s)
        for r, exact, factor in ((0, low, LD(1)), (1, top, np.exp(-LD(alpha)))):
            v = x[r].reshape(ne, npe)
            delta = 0.5 * LD(EPS) * np.abs(exact)  # the samples were rounded to double
            bound = mu.apply_bound(F, v, dim) + mu.tensor_apply(np.abs(F), delta, dim) + factor * delta
            _within(f"{_id(key)} k_c={kc} row {r}", got[r].reshape(ne, npe), factor * v.astype(LD), bound)
        assert np.array_equal(got[2:], x[2:])
        assert float(np.abs(got[1] - x[1]).max()) > 0.5 * float(np.abs(x[1]).max())  # exp(-2) is far from 1
    rep = op.readModalFilter()
    op.close()
    ncalls = len({0, p - 1})
    assert rep == dict(calls=ncalls, elements_seen=ncalls * ne, elements_filtered=ncalls * ne)
    assert n1 == p + 1


# ---- 3. filter against the restatement, 4. conservation ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL, ids=_id)
def test_filter_matches_the_restatement_and_conserves(key):
    c, dim, p, basis, npe, ne = _shape(key)
    w = _device_weights(key)
    radial = bool(c.disc.axisymmetric)
    rng = np.random.default_rng(41)
    op = _operator(c)
    neq = op.num_equation
    x = rng.standard_normal((neq, ne * npe)) + 0.5
    subset = [neq - 1, 1]
    for kc, rows in ((0, None), (p - 1, subset)):
        kw = dict(cutoff=kc, alpha=3.0, exponent=2, conservative=True)
        ref = mu.modal_filter(x, w, dim, p, basis, rows, **kw)
        xd = _dev(op, x)
        before = op.integrate(xd)[0].cpu().numpy()
        op.modalFilter(xd, rows=rows, **kw)
        after = op.integrate(xd)[0].cpu().numpy()
        got = xd.cpu().numpy()
        listed = list(range(neq)) if rows is None else rows
        others = [r for r in range(neq) if r not in listed]
        _within(f"{_id(key)} k_c={kc} rows={rows}", got[listed], ref["x"][listed], ref["bound"][listed])
        assert np.array_equal(got[others], x[others])
        assert float(np.abs(got[listed] - x[listed]).max()) > 1e-3  # the filter acts
        # every element integral: sum W (u~ + c - u) = 0 exactly for the weights as given, so the drift is at most sum |W| bound_n
        for r in listed:
            drift = np.abs(mu.element_integrals(w, got[r], npe) - mu.element_integrals(w, x[r], npe))
            allowed = mu.element_integrals(np.abs(w), ref["bound"][r] + LD(EPS) * np.abs(ref["x"][r]), npe)
            print(f"{_id(key)} row {r}: max element drift / allowed = {float((drift / allowed).max()):.4f}")
            assert (drift <= allowed).all()
        # the tpsrhs_integrate totals: the two documented bounds of integrate and the drift above
        rb = iu.integrate(c.mesh, p, basis, x[listed], radial=radial)
        ra = iu.integrate(c.mesh, p, basis, got[listed], radial=radial)
        slack = np.array([float(mu.element_integrals(np.abs(w), ref["bound"][r] + LD(EPS) * np.abs(ref["x"][r]), npe).sum()) for r in listed])
        bound = rb["K"] * EPS * (rb["S1"] + ra["S1"]) + slack
        change = np.abs(after[listed] - before[listed])
        print(f"{_id(key)} k_c={kc}: |total after - before| / bound = {change / bound}")
        assert (change <= bound).all()
    op.close()


@pytest.mark.parametrize("key", [("quad", 2, 0), ("quad", 3, 1), ("hex", 2, 0), ("hex", 3, 1)] + AXI + FLAT, ids=_id)
def test_without_the_correction_only_affine_elements_keep_their_integrals(key):
    """conservative = 0 keeps the reference-space mean, which is the physical mean where |det J| (times r) is constant over
    the element.  That holds on the unwarped boxes -- and on the warped box_quad too: its warp moves x by a function of y
    and y by a function of x, which leaves every element a parallelogram (the bilinear map has no xi eta term).  There the
    integrals stay; on the warped hexes and on the axisymmetric annulus (weight r) they move, by what the restatement says,
    far outside the rounding: the flag acts."""
    c, dim, p, basis, npe, ne = _shape(key)
    Wref = _reference_weights(key)  # long double: on an affine element proportional to the reference weights to ~1e-19
    rng = np.random.default_rng(43)
    op = _operator(c)
    neq = op.num_equation
    x = rng.standard_normal((neq, ne * npe)) + 0.5
    kw = dict(cutoff=0, alpha=3.0, exponent=2, conservative=False)
    ref = mu.modal_filter(x, np.ones(ne * npe), dim, p, basis, None, **kw)
    xd = _dev(op, x)
    op.modalFilter(xd, **kw)
    got = xd.cpu().numpy()
    op.close()
    _within(f"{_id(key)} plain filter", got, ref["x"], ref["bound"])
    flat = key[0].endswith("_flat") or key[0] == "quad"  # affine elements
    big = 0.0
    for r in range(neq):
        drift = mu.element_integrals(Wref, got[r], npe) - mu.element_integrals(Wref, x[r], npe)
        drift_ref = mu.element_integrals(Wref, ref["x"][r], npe) - mu.element_integrals(Wref, x[r], npe)
        allowed = mu.element_integrals(np.abs(Wref), ref["bound"][r] + LD(EPS) * np.abs(ref["x"][r]), npe)
        print(f"{_id(key)} row {r}: max |drift - restatement's| / allowed = {float((np.abs(drift - drift_ref) / allowed).max()):.4f}; "
              f"max |restatement's drift| / allowed = {float((np.abs(drift_ref) / allowed).max()):.3g}")
        assert (np.abs(drift - drift_ref) <= allowed).all()
        if flat:  # the reference-space mean is the physical mean: the integral stays
            assert (np.abs(drift) <= allowed + LD(1e-17) * np.abs(mu.element_integrals(np.abs(Wref), np.abs(x[r]), npe))).all()
        big = max(big, float((np.abs(drift_ref) / allowed).max()))
    if not flat:  # the flag acts: the drift is far outside the rounding
        assert big > 1000.0


# ---- 5. energies and sensor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL, ids=_id)
def test_energies_and_sensor(key):
    import torch

    c, dim, p, basis, npe, ne = _shape(key)
    n1 = p + 1
    V, _ = mu.matrices(p, basis)
    shell, _ = mu.shells(p, dim)
    rng = np.random.default_rng(47)
    u = rng.standard_normal(ne * npe)
    # single-shell fields: element e holds modes of shell e mod (p + 1) only
    coef = rng.standard_normal((ne, npe)).astype(LD)
    for e in range(ne):
        coef[e, shell != e % n1] = 0
    single = mu.tensor_apply(V, coef, dim).astype(np.float64).reshape(-1)
    zero_nan = u.copy()
    zero_nan[:npe] = 0.0                 # element 0: zero
    zero_nan[2 * npe + npe // 2] = np.nan  # element 2: one NaN node
    op = _operator(c)
    out = []
    for f in (u, single, zero_nan):
        E, S = op.modalEnergy(_dev(op, f))
        out.append((E.cpu().numpy(), S.cpu().numpy()))
    # either output alone, through the C ABI
    lib = capi.load()
    fd = _dev(op, u)
    Eo = torch.empty((ne, n1), dtype=torch.float64, device=op.device)
    So = torch.empty(ne, dtype=torch.float64, device=op.device)
    assert lib.tpsrhs_modal_energy(op._h, C.c_void_p(fd.data_ptr()), C.c_void_p(Eo.data_ptr()), None) == 0
    assert lib.tpsrhs_modal_energy(op._h, C.c_void_p(fd.data_ptr()), None, C.c_void_p(So.data_ptr())) == 0
    assert np.array_equal(Eo.cpu().numpy(), out[0][0]) and np.array_equal(So.cpu().numpy(), out[0][1])
    sumsq = op.integrate(_dev(op, u[None]))[1].cpu().numpy()[0] if key[0].endswith("_flat") else None
    op.close()
    ref = mu.energies(u, p, basis, dim)
    _within(f"{_id(key)} E", out[0][0], ref["E"], ref["dE"])
    _within(f"{_id(key)} S", out[0][1], ref["S"], ref["dS"])
    assert ((out[0][1] > 0) & (out[0][1] < 1)).all()
    # single shells: S = 1 for shell p and 0 otherwise, up to what the rounded samples leave in the other shells
    rs = mu.energies(single, p, basis, dim)
    _within(f"{_id(key)} single-shell E", out[1][0], rs["E"], rs["dE"])
    _within(f"{_id(key)} single-shell S", out[1][1], rs["S"], rs["dS"])
    want = (np.arange(ne) % n1 == p).astype(np.float64)
    print(f"{_id(key)} single shells: max |S - (0 or 1)| = {np.abs(out[1][1] - want).max():.3g}")
    # the construction: in the restatement the other shells hold the squares of the samples' rounding only; the device is
    # within dS of the restatement (asserted above), which is a few hundred eps at most
    assert float(np.abs(rs["S"] - want).max()) < 1e-17 and float(rs["dS"].max()) < 1e5 * EPS
    assert (np.abs(out[1][1] - want) <= (rs["dS"] + np.abs(rs["S"] - want)).astype(np.float64) + EPS).all()
    # zero element: S = 0 and E = 0 exactly; the NaN node: a NaN sensor in its element only
    Ez, Sz = out[2]
    assert Sz[0] == 0.0 and (Ez[0] == 0.0).all()
    assert np.isnan(Sz[2]) and np.isnan(Ez[2]).all()
    rest = [e for e in range(ne) if e not in (0, 2)]
    assert np.array_equal(Sz[rest], out[0][1][rest]) and np.array_equal(Ez[rest], out[0][0][rest])
    if sumsq is not None:
        # Parseval against existing device code: |K| sum_m E_m summed over the elements of the unwarped box equals
        # tpsrhs_integrate's sum of squares, whose rule is exact for degree 2p
        vol = mu.element_integrals(_reference_weights(key), np.ones(ne * npe), npe)
        total = float((vol * out[0][0].astype(LD).sum(axis=1)).sum())
        ri = iu.integrate(c.mesh, p, basis, u[None])
        bound = 2 * ri["K"] * EPS * ri["S2"][0] + float((vol * (ref["dE"].sum(axis=1) + n1 * LD(EPS) * ref["E"].sum(axis=1))).sum())
        print(f"{_id(key)} Parseval: |K| sum E = {total:.16g}, integrate(u^2) = {sumsq:.16g}, |difference| / bound = {abs(total - sumsq) / bound:.4f}")
        assert abs(total - sumsq) <= bound


# ---- 6. selective filtering ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL, ids=_id)
def test_selective_filtering(key):
    c, dim, p, basis, npe, ne = _shape(key)
    w = _device_weights(key)
    V, _ = mu.matrices(p, basis)
    shell, _ = mu.shells(p, dim)
    rng = np.random.default_rng(53)
    op = _operator(c)
    neq = op.num_equation
    srow, thr = min(1, neq - 1), 1e-3
    # the sensor row: odd elements rough (shell p ten times the rest), even elements smooth (nothing in shell p)
    coef = rng.standard_normal((ne, npe)).astype(LD)
    rough = np.arange(ne) % 2 == 1
    coef[np.ix_(rough, shell == p)] *= 10
    coef[np.ix_(~rough, shell == p)] = 0
    x = rng.standard_normal((neq, ne * npe))
    x[srow] = mu.tensor_apply(V, coef, dim).astype(np.float64).reshape(-1)
    kw = dict(cutoff=0, alpha=36.0, exponent=4, conservative=True, sensor_row=srow, sensor_threshold=thr)
    ref = mu.modal_filter(x, w, dim, p, basis, None, **kw)
    # the condition of the test: every decision is at least a factor 100 from the threshold in the restatement
    S = ref["S"].astype(np.float64)
    print(f"{_id(key)}: S rough >= {S[rough].min():.3g}, S smooth <= {S[~rough].max():.3g}")
    assert (S[rough] >= 0.1).all() and (S[~rough] <= thr / 100).all() and np.array_equal(ref["filtered"], rough)
    xd = _dev(op, x)
    op.readModalFilter(reset=True)
    op.modalFilter(xd, **kw)  # rows = -1: the sensor row is among the filtered rows and decides from its incoming values
    rep = op.readModalFilter()
    got = xd.cpu().numpy()
    sel = np.repeat(rough, npe)
    _within(f"{_id(key)} rough elements", got[:, sel], ref["x"][:, sel], ref["bound"][:, sel])
    assert np.array_equal(got[:, ~sel], x[:, ~sel])
    assert float(np.abs(got[srow, sel] - x[srow, sel]).max()) > 1.0  # the top shell of the rough elements is gone
    assert rep == dict(calls=1, elements_seen=ne, elements_filtered=int(rough.sum()))
    # a second application adds; reset works
    op.modalFilter(xd, **kw)
    rep2 = op.readModalFilter(reset=True)
    assert rep2["calls"] == 2 and rep2["elements_seen"] == 2 * ne and rep2["elements_filtered"] <= 2 * int(rough.sum())
    assert op.readModalFilter() == dict(calls=0, elements_seen=0, elements_filtered=0)
    # threshold +inf filters nothing
    xd = _dev(op, x)
    op.modalFilter(xd, **dict(kw, sensor_threshold=float("inf")))
    assert np.array_equal(xd.cpu().numpy(), x)
    assert op.readModalFilter() == dict(calls=1, elements_seen=ne, elements_filtered=0)
    # a NaN sensor: not filtered
    xn = x.copy()
    xn[srow, npe + 1] = np.nan  # element 1, a rough one
    xd = _dev(op, xn)
    op.readModalFilter(reset=True)
    op.modalFilter(xd, **kw)
    gn = xd.cpu().numpy()
    assert op.readModalFilter()["elements_filtered"] == int(rough.sum()) - 1
    assert np.array_equal(gn[:, npe:2 * npe], xn[:, npe:2 * npe], equal_nan=True)
    assert np.array_equal(gn[:, 2 * npe:], got[:, 2 * npe:])
    op.close()


# ---- 7. refusals through the C ABI ---------------------------------------------------------------------------------------------------
def _refused(status, fragment, call):
    lib = capi.load()
    st = call()
    msg = lib.tpsrhs_last_error().decode()
    assert st == status and fragment in msg, (st, msg)


def test_refusals_through_the_c_abi():
    from tps_amd.rhs_operator import TpsRhsError

    lib = capi.load()
    INVALID = capi.ERR_INVALID_ARGUMENT
    op = _operator(_case("quad", 2, 0))
    neq = op.num_equation
    x0 = np.random.default_rng(3).standard_normal((neq, op.NDofs))
    xd = _dev(op, x0)
    xp, f, rep = C.c_void_p(xd.data_ptr()), capi.make_modal_filter(), capi.ModalFilterReport()
    _refused(INVALID, "tpsrhs_modal_transform", lambda: lib.tpsrhs_modal_transform(None, 0, 1, xp, xp))
    _refused(INVALID, "tpsrhs_modal_transform", lambda: lib.tpsrhs_modal_transform(op._h, 0, 1, None, xp))
    _refused(INVALID, "tpsrhs_modal_transform", lambda: lib.tpsrhs_modal_transform(op._h, 0, 1, xp, None))
    _refused(INVALID, "nrows", lambda: lib.tpsrhs_modal_transform(op._h, 0, 0, xp, xp))
    _refused(INVALID, "tpsrhs_modal_energy", lambda: lib.tpsrhs_modal_energy(None, xp, xp, xp))
    _refused(INVALID, "tpsrhs_modal_energy", lambda: lib.tpsrhs_modal_energy(op._h, None, xp, xp))
    _refused(INVALID, "both NULL", lambda: lib.tpsrhs_modal_energy(op._h, xp, None, None))
    _refused(INVALID, "tpsrhs_modal_filter_apply", lambda: lib.tpsrhs_modal_filter_apply(None, C.byref(f), xp))
    _refused(INVALID, "tpsrhs_modal_filter_apply", lambda: lib.tpsrhs_modal_filter_apply(op._h, None, xp))
    _refused(INVALID, "tpsrhs_modal_filter_apply", lambda: lib.tpsrhs_modal_filter_apply(op._h, C.byref(f), None))
    _refused(INVALID, "tpsrhs_modal_filter_configure", lambda: lib.tpsrhs_modal_filter_configure(None, C.byref(f)))
    _refused(INVALID, "tpsrhs_modal_filter_read", lambda: lib.tpsrhs_modal_filter_read(None, C.byref(rep), 0))
    _refused(INVALID, "tpsrhs_modal_filter_read", lambda: lib.tpsrhs_modal_filter_read(op._h, None, 0))
    nan, inf = float("nan"), float("inf")
    for kw, fragment in ((dict(rows=[neq]), "outside"), (dict(rows=[-1]), "outside"), (dict(rows=[1, 1]), "twice"),
                         (dict(cutoff=-1), "cutoff"), (dict(cutoff=2), "cutoff"), (dict(alpha=0.0), "alpha"),
                         (dict(alpha=-1.0), "alpha"), (dict(alpha=nan), "alpha"), (dict(alpha=inf), "alpha"),
                         (dict(exponent=0), "exponent"), (dict(sensor_row=-2), "sensor_row"), (dict(sensor_row=neq), "sensor_row"),
                         (dict(sensor_row=0, sensor_threshold=nan), "sensor_threshold")):
        for call in (lambda: op.modalFilter(xd, **kw), lambda: op.configureModalFilter(**kw)):
            with pytest.raises(TpsRhsError) as e:
                call()
            assert e.value.status == INVALID and fragment in str(e.value), str(e.value)
    for n in (-2, neq + 1):
        bad = capi.make_modal_filter()
        bad.num_rows = n
        _refused(INVALID, "num_rows", lambda: lib.tpsrhs_modal_filter_apply(op._h, C.byref(bad), xp))
        _refused(INVALID, "num_rows", lambda: lib.tpsrhs_modal_filter_configure(op._h, C.byref(bad)))
    # nothing was counted and no bit of x moved; +inf as a threshold is valid
    assert op.readModalFilter() == dict(calls=0, elements_seen=0, elements_filtered=0)
    assert np.array_equal(xd.cpu().numpy(), x0)
    op.configureModalFilter(sensor_row=0, sensor_threshold=inf)
    op.configureModalFilter(off=True)
    op.close()
