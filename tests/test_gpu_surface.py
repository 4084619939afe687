"""tpsrhs_surface_* (tps_amd/csrc/surface.hpp) on the device against closed forms and the numpy restatement of
tests/surface_util.py.  Every comparison of an integral uses the DERIVED bound of that module -- |error| <= K_s eps S,
K_s = NQ^(dim-1) + nf_p + 8 dim (p + 1) + 16, plus 8 eps |exact| against a closed form -- and prints the achieved error
as a fraction of the bound.  With TPSRHS_SURFACE_RATIOS=<file> the largest ratio per test is also written there."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import integrals_util as iu
import surface_util as sfu
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
EPS = sfu.EPS
_RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_file():
    yield
    path = os.environ.get("TPSRHS_SURFACE_RATIOS")
    if path:
        worst = {}
        for name, ratio in _RATIOS:
            test = name.split(":")[0]
            worst[test] = max(worst.get(test, 0.0), ratio)
        with open(path, "w") as f:
            f.write("largest |device - reference| / bound per test (bound: K_s eps S of include/tpsrhs.h, + 8 eps |exact| against a closed form)\n")
            for test, ratio in worst.items():
                f.write(f"{test:60s} {ratio:.4f}\n")


def _walls(mesh):
    return [capi.make_bc(int(a), capi.WALL, capi.INV) for a in sorted(set(int(a) for a in mesh.bdr_attributes))]


def _case(mesh, order, basis=0):
    return cases.Case("surface", mesh, capi.Disc(order, basis, basis, 0, 0), capi.dry_air_physics(capi.EULER), _walls(mesh))


def _operator(c, **kw):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, c.physics, c.bcs, **kw)


def _dev(op, a):
    import torch

    return torch.tensor(np.ascontiguousarray(a).ravel(), dtype=torch.float64, device=op.device)


def _all_forms(op, surf, F, **kw):
    """F (nrows, NDofs) with nrows a multiple of dim: SCALAR and NORMAL of its rows, FLUX of its rows taken dim at a time"""
    d = _dev(op, F)
    return (surf.integrate(d, "scalar", **kw).cpu().numpy(), surf.integrate(d, "flux", **kw).cpu().numpy(),
            surf.integrate(d, "normal", **kw).cpu().numpy())


def _restate_all(mesh, order, basis, faces, npatch, F, radial=False):
    dim = mesh.dim
    return (sfu.integrate(mesh, order, basis, *faces, npatch, F, sfu.SCALAR, radial),
            sfu.integrate(mesh, order, basis, *faces, npatch, F.reshape(-1, dim, F.shape[1]), sfu.FLUX, radial),
            sfu.integrate(mesh, order, basis, *faces, npatch, F, sfu.NORMAL, radial))


# ---- 1. planar, non-affine boundary: closed forms --------------------------------------------------------------------------
def _planar_check(dim, order, basis, nvec, name):
    mesh = sfu.planar_box(dim, (3, 2, 2)[:dim])
    op = _operator(_case(mesh, order, basis))
    faces = sfu.box_patches(mesh)
    surf = op.createSurface(attributes=[1 + k for k in range(2 * dim)])
    assert surf.info()[1] == faces[0].size
    X = node_coordinates(mesh, order, basis)
    polys = [sfu.polynomial_terms(dim, order, 1000 * order + 10 * dim + k) for k in range(nvec * dim)]
    F = np.stack([iu.polynomial(dim, order, 1000 * order + 10 * dim + k)[0](X) for k in range(nvec * dim)])
    got = _all_forms(op, surf, F)
    if nvec == 1:  # nrows = 1
        one = surf.integrate(_dev(op, F[0]), "scalar").cpu().numpy()
        assert one.shape == (2 * dim, 1) and np.array_equal(one[:, 0], got[0][:, 0])
    surf.close()
    op.close()
    ref = _restate_all(mesh, order, basis, faces, 2 * dim, F)
    exact = np.array([[sfu.box_face_integral(*polys[k], p >> 1, p & 1) for k in range(nvec * dim)] for p in range(2 * dim)])
    unit = np.zeros((2 * dim, dim))
    for p in range(2 * dim):
        unit[p, p >> 1] = 2 * (p & 1) - 1
    exact_flux = np.array([[unit[p, p >> 1] * exact[p, v * dim + (p >> 1)] for v in range(nvec)] for p in range(2 * dim)])
    for form, g, r, ex in (("scalar", got[0], ref[0], exact), ("flux", got[1], ref[1], exact_flux),
                           ("normal", got[2], ref[2], exact[:, :, None] * unit[:, None, :])):
        sfu.check(f"{name}: {form} restatement", g, r, log=_RATIOS)
        sfu.check(f"{name}: {form} closed form", g, r, exact=ex, log=_RATIOS)


@pytest.mark.parametrize("basis,order", [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 1), (1, 2), (1, 3)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("dim", [2, 3])
def test_polynomials_over_planar_box_faces(dim, basis, order):
    """3 x 2 quadrilaterals / 3 x 2 x 2 hexahedra on the unit box, every vertex moved within the box face, edge or interior it
    lies in: planar boundary faces that are no parallelograms.  A polynomial of total degree <= p: SCALAR is its closed-form
    integral over each box face, NORMAL that number times the face's unit normal (the other components against the bound),
    FLUX the closed form of the normal component."""
    _planar_check(dim, order, basis, 1, f"test_polynomials_over_planar_box_faces[{dim}d basis {basis} p{order}]")


def test_thirty_seven_rows_take_several_passes():
    """37 rows: three passes of SCALAR and of FLUX (16 accumulators a launch), eight of NORMAL (five rows each in 3-D)"""
    dim, order = 3, 2
    mesh = sfu.planar_box(dim, (3, 2, 2))
    op = _operator(_case(mesh, order))
    faces = sfu.box_patches(mesh)
    surf = op.createSurface(faces=faces)
    X = node_coordinates(mesh, order)
    polys = [sfu.polynomial_terms(dim, order, 500 + k) for k in range(37)]
    F = np.stack([sfu.polynomial_eval(*polys[k], X) for k in range(37)])
    d = _dev(op, F)
    sc = surf.integrate(d, "scalar").cpu().numpy()
    nm = surf.integrate(d, "normal").cpu().numpy()
    # FLUX of 37 vectors (f_r, f_{r+1}, f_{r+2}) with overlapping rows: row_stride = NDofs
    n = F.shape[1]
    fl = surf.integrate(d, "flux", row_stride=n, comp_stride=n).cpu().numpy()
    surf.close()
    op.close()
    assert sc.shape == (6, 37) and nm.shape == (6, 37, 3) and fl.shape == (6, 35)
    exact = np.array([[sfu.box_face_integral(*polys[k], p >> 1, p & 1) for k in range(37)] for p in range(6)])
    unit = np.zeros((6, 3))
    for p in range(6):
        unit[p, p >> 1] = 2 * (p & 1) - 1
    name = "test_thirty_seven_rows_take_several_passes"
    sfu.check(f"{name}: scalar", sc, sfu.integrate(mesh, order, 0, *faces, 6, F, sfu.SCALAR), exact=exact, log=_RATIOS)
    sfu.check(f"{name}: normal", nm, sfu.integrate(mesh, order, 0, *faces, 6, F, sfu.NORMAL),
              exact=exact[:, :, None] * unit[:, None, :], log=_RATIOS)
    Fv = np.stack([F[r:r + 3] for r in range(35)])
    exact_flux = np.array([[unit[p, p >> 1] * exact[p, r + (p >> 1)] for r in range(35)] for p in range(6)])
    sfu.check(f"{name}: flux", fl, sfu.integrate(mesh, order, 0, *faces, 6, Fv, sfu.FLUX), exact=exact_flux, log=_RATIOS)


# ---- 2. warped, closed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 3, 5])
@pytest.mark.parametrize("dim", [2, 3])
def test_warped_closed_surface(dim, order):
    """every boundary face of a warped box, as one patch and as 2 dim patches: the normals add up to zero, the flux of X is
    dim times the volume, the flux of a polynomial vector field is the volume integral of its divergence (both sides on the
    device: the two bounds add), SCALAR against the restatement"""
    mesh = (meshgen.box_hex(3, 2, 2, periodic=(False,) * 3, warp=0.08) if dim == 3 else
            meshgen.box_quad(3, 2, periodic=(False,) * 2, warp=0.08))
    op = _operator(_case(mesh, order))
    split = sfu.box_patches(mesh)
    whole = (split[0], split[1], np.zeros_like(split[2]))
    X = node_coordinates(mesh, order)
    ones = np.ones((1, X.shape[1]))
    polys = [sfu.polynomial_terms(dim, order, 70 * order + k) for k in range(dim)]
    F = np.stack([sfu.polynomial_eval(*polys[k], X) for k in range(dim)])
    div = sum(sfu.polynomial_eval(*sfu.polynomial_derivative(*polys[k], k), X) for k in range(dim)) + np.zeros(X.shape[1])
    vol, _ = op.integrate(_dev(op, np.stack([ones[0], div])))
    vol = vol.cpu().numpy()
    vref = iu.integrate(mesh, order, 0, np.stack([ones[0], div]))
    vbound = vref["K"] * EPS * vref["S1"]
    name = f"test_warped_closed_surface[{dim}d p{order}]"
    for label, faces, npatch in (("one patch", whole, 1), ("split", split, 2 * dim)):
        surf = op.createSurface(faces=faces + (npatch,))
        nm = surf.integrate(_dev(op, ones), "normal").cpu().numpy()      # (npatch, 1, dim)
        fx = surf.integrate(_dev(op, X), "flux").cpu().numpy()           # (npatch, 1)
        ff = surf.integrate(_dev(op, F), "flux").cpu().numpy()
        sc = surf.integrate(_dev(op, F), "scalar").cpu().numpy()
        surf.close()
        rn = sfu.integrate(mesh, order, 0, *faces, npatch, ones, sfu.NORMAL)
        rx = sfu.integrate(mesh, order, 0, *faces, npatch, X[None], sfu.FLUX)
        rf = sfu.integrate(mesh, order, 0, *faces, npatch, F[None], sfu.FLUX)
        sfu.check(f"{name}: {label} normal", nm, rn, log=_RATIOS)
        sfu.check(f"{name}: {label} flux of X", fx, rx, log=_RATIOS)
        sfu.check(f"{name}: {label} flux of F", ff, rf, log=_RATIOS)
        sfu.check(f"{name}: {label} scalar", sc, sfu.integrate(mesh, order, 0, *faces, npatch, F, sfu.SCALAR), log=_RATIOS)
        # the sums over the patches, added exactly
        for k in range(dim):
            total, bound = math.fsum(nm[:, 0, k]), float((rn["K"] * EPS * rn["S"][:, 0]).sum())
            _RATIOS.append((f"{name}: {label} closed normal", abs(total) / bound))
            assert abs(total) <= bound, (label, k, total, bound)
        for got, r, want, vb, what in ((fx, rx, dim * vol[0], dim * vbound[0], "dim V"), (ff, rf, vol[1], vbound[1], "div F")):
            total, bound = math.fsum(got[:, 0]), float((r["K"] * EPS * r["S"][:, 0]).sum()) + vb + 8 * EPS * abs(want)
            print(f"{name}: {label} {what}: surface {total!r}, volume {want!r}, bound {bound:.3e}")
            _RATIOS.append((f"{name}: {label} {what}", abs(total - want) / bound))
            assert abs(total - want) <= bound, (label, what, total, want, bound)
    op.close()


# ---- 3. partial batches and corner elements ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big_box():
    mesh = iu.perturbed_box(3, (7, 5, 3))
    faces = sfu.box_patches(mesh)
    assert faces[0].size == 142
    return mesh, faces


@pytest.mark.parametrize("order", [1, 2])
def test_partial_batches_and_corner_elements(order):
    """7 x 5 x 3 hexahedra, 142 boundary faces: at p = 1 four faces share a wave and the last batch of most patches is
    partial; corner elements carry three faces of three patches.  The six sides, one single face, the faces of one element,
    and an empty patch between two others, against the restatement; two calls and a surface made from the shuffled list
    are bit-equal."""
    mesh, faces = _big_box()
    op = _operator(_case(mesh, order))
    rng = np.random.default_rng(17 + order)
    F = rng.standard_normal((6, mesh.num_elements * (order + 1) ** 3))
    name = f"test_partial_batches_and_corner_elements[p{order}]"
    corner = faces[0] == 0
    assert sorted(faces[1][corner]) == [0, 2, 4] and len(set(faces[2][corner])) == 3
    one = tuple(a[77:78] for a in faces)
    gap = tuple(a[(faces[2] == 1) | (faces[2] == 4)] for a in faces)
    gap = (gap[0], gap[1], np.where(gap[2] == 1, 0, 2).astype(np.int32))  # patch 1 of 3 stays empty
    sets = (("six sides", faces, 6), ("one face", (one[0], one[1], np.zeros(1, np.int32)), 1),
            ("one element", tuple(a[corner] for a in faces[:2]) + (np.arange(3, dtype=np.int32),), 3), ("empty patch", gap, 3))
    for label, fs, npatch in sets:
        surf = op.createSurface(faces=fs + (npatch,))
        got = _all_forms(op, surf, F)
        again = _all_forms(op, surf, F)
        perm = rng.permutation(fs[0].size)
        shuffled = op.createSurface(faces=tuple(a[perm] for a in fs) + (npatch,))
        other = _all_forms(op, shuffled, F)
        info = surf.info()
        assert info[0] == npatch and info[1] == fs[0].size and np.array_equal(info[2], np.bincount(fs[2], minlength=npatch))
        shuffled.close()
        surf.close()
        for a, b, c in zip(got, again, other):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        if label == "empty patch":
            assert all((g[1] == 0.0).all() for g in got)
        for form, g, r in zip(("scalar", "flux", "normal"), got, _restate_all(mesh, order, 0, fs, npatch, F)):
            sfu.check(f"{name}: {label} {form}", g, r, log=_RATIOS)
    empty = op.createSurface(faces=(np.zeros(0, np.int32),) * 3 + (2,))  # no face at all: every integral is zero
    assert all((g == 0.0).all() for g in _all_forms(op, empty, F))
    op.close()


# ---- 4. areas in closed form -----------------------------------------------------------------------------------------------------
def test_areas_of_the_cylinder_and_the_ring_and_a_mass_flow_outlet():
    from tps_amd.rhs_operator import RHSoperator, TpsRhsError

    name = "test_areas_of_the_cylinder_and_the_ring_and_a_mass_flow_outlet"
    c = cases.cyl3d(3, 8, 3, 2)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    surf = op.createSurface(attributes=[1, 2, 3])
    area = surf.area().cpu().numpy()
    both = op.createSurface(faces=(lambda f: (f[0], f[1], np.where(f[2] == 2, 1, 0).astype(np.int32)))(capi.patch_faces(c.mesh, [1, 2, 3])))
    a2 = both.area().cpu().numpy()
    op.close()
    chord = 8 * 2 * math.sin(math.pi / 8) * 2.0  # ntheta chords of the unit circle times the span
    ones = np.ones((1, c.mesh.num_elements * 27))
    ref = sfu.integrate(c.mesh, 2, 0, *sfu.patch_faces_np(c.mesh, [1, 2, 3]), 3, ones)
    sfu.check(f"{name}: cylinder restatement", area[:, None], ref, log=_RATIOS)
    sfu.check(f"{name}: cylinder wall", area[2:, None], {k: v[2:] for k, v in ref.items()}, exact=[[0.5 * chord]], log=_RATIOS)
    f3 = sfu.patch_faces_np(c.mesh, [1, 2, 3])
    ref2 = sfu.integrate(c.mesh, 2, 0, f3[0], f3[1], np.where(f3[2] == 2, 1, 0), 2, ones)
    sfu.check(f"{name}: inlet + outlet", a2[:1, None], {k: v[:1] for k, v in ref2.items()}, exact=[[10.0 * chord]], log=_RATIOS)
    # the mass-flow outlet needs the area of its patch in data[7]: refused without, accepted with surface.area()
    data = [1.2 * 20.0 * float(area[1]), 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_MF_NR, data + [0.0])
    with pytest.raises(TpsRhsError):
        RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    c.bcs[1] = capi.make_bc(2, capi.OUTLET, capi.SUB_MF_NR, data + [float(area[1])])
    RHSoperator(c.mesh, c.disc, c.physics, c.bcs).close()
    # the 2-D chord sums
    ring = iu.ring_quad()
    op = _operator(_case(ring, 3))
    f = sfu.patch_faces_np(ring, [3, 1, 2])
    f = (f[0], f[1], np.minimum(f[2], 1).astype(np.int32))  # patch 0 the wall, patch 1 inlet and outlet: the outer circle
    a = op.createSurface(faces=f).area().cpu().numpy()
    op.close()
    ref = sfu.integrate(ring, 3, 0, *f, 2, np.ones((1, ring.num_elements * 16)))
    chord = 12 * 2 * math.sin(math.pi / 12)
    sfu.check(f"{name}: ring wall and outer circle", a[:, None], ref, exact=[[0.5 * chord], [10.0 * chord]], log=_RATIOS)


# ---- 5. axisymmetric -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
def test_axisymmetric_areas_carry_the_radial_weight(order):
    from tps_amd.rhs_operator import RHSoperator

    mesh = meshgen.annulus_quad(4, 5, r_in=0.2, r_out=1.0, length=2.0)  # 4 inner wall, 3 outer wall, 1 and 2 the ends
    c = cases.dry_air_axisym(4, 5, order)
    op = RHSoperator(mesh, c.disc, c.physics, c.bcs)
    surf = op.createSurface(attributes=[3, 1, 2, 4])
    weighted = surf.area().cpu().numpy()  # radial=None: the operator's axisymmetric flag
    plain = surf.area(radial=False).cpu().numpy()
    op.close()
    f = sfu.patch_faces_np(mesh, [3, 1, 2, 4])
    ones = np.ones((1, mesh.num_elements * (order + 1) ** 2))
    name = f"test_axisymmetric_areas_carry_the_radial_weight[p{order}]"
    ends = (1.0 - 0.2 ** 2) / 2
    sfu.check(f"{name}: radial", weighted[:, None], sfu.integrate(mesh, order, 0, *f, 4, ones, radial=True),
              exact=[[1.0 * 2.0], [ends], [ends], [0.2 * 2.0]], log=_RATIOS)
    sfu.check(f"{name}: plain", plain[:, None], sfu.integrate(mesh, order, 0, *f, 4, ones, radial=False),
              exact=[[2.0], [0.8], [0.8], [2.0]], log=_RATIOS)


# ---- 6. interior faces -----------------------------------------------------------------------------------------------------------
def test_a_station_plane_from_either_side():
    """the plane x = 1/3 of the unperturbed box, once as the faces (d = 0, s = 1) of the first column of elements and once
    as (d = 0, s = 0) of the second: a continuous polynomial has the same SCALAR and opposite FLUX"""
    order = 3
    mesh = meshgen.box_hex(3, 2, 2, periodic=(False,) * 3)
    op = _operator(_case(mesh, order))
    first, second = np.arange(0, 12, 3, dtype=np.int32), np.arange(1, 12, 3, dtype=np.int32)
    left = (first, np.full(4, 1, np.int32), np.zeros(4, np.int32))
    right = (second, np.zeros(4, np.int32), np.zeros(4, np.int32))
    X = node_coordinates(mesh, order)
    F = np.stack([iu.polynomial(3, order, 40 + k)[0](X) for k in range(3)])
    a, b = op.createSurface(faces=left), op.createSurface(faces=right)
    ga, gb = _all_forms(op, a, F), _all_forms(op, b, F)
    op.close()
    ra, rb = _restate_all(mesh, order, 0, left, 1, F), _restate_all(mesh, order, 0, right, 1, F)
    name = "test_a_station_plane_from_either_side"
    for form, sign in (("scalar", 1.0), ("flux", -1.0), ("normal", -1.0)):
        k = ("scalar", "flux", "normal").index(form)
        sfu.check(f"{name}: left {form}", ga[k], ra[k], log=_RATIOS)
        sfu.check(f"{name}: right {form}", gb[k], rb[k], log=_RATIOS)
        Sa = ra[k]["S"] if ga[k].ndim == 2 else ra[k]["S"][:, :, None]
        Sb = rb[k]["S"] if gb[k].ndim == 2 else rb[k]["S"][:, :, None]
        bound = EPS * (ra[k]["K"][0] * Sa + rb[k]["K"][0] * Sb)
        assert (np.abs(ga[k] - sign * gb[k]) <= bound).all(), form
    assert abs(ga[1][0, 0]) > 1e-3  # (the flux is not zero)


# ---- 7. strides ----------------------------------------------------------------------------------------------------------------
def test_gradients_go_in_as_they_are():
    """int grad u . n dS straight from tpsrhs_get_gradients ([d][eq][NDofs]: row_stride = NDofs, comp_stride = neq NDofs)
    and from a repacked contiguous [eq][d][NDofs] copy: bit-equal"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    c = cases.cyl3d(3, 8, 3, 2, capi.NS, capi.VISC_ISOTH)
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    x = _dev(op, c.state(seed=4))
    op.updateGradients(x)
    g = op.getGradients()
    n, neq = op.NDofs, op.num_equation
    assert g.numel() == 3 * neq * n
    surf = op.createSurface(attributes=[1, 2, 3])
    direct = surf.integrate(g, "flux", row_stride=n, comp_stride=neq * n)
    packed = surf.integrate(g.reshape(3, neq, n).permute(1, 0, 2).contiguous(), "flux")
    torch.cuda.synchronize()
    assert direct.shape == (3, neq) and torch.equal(direct, packed) and bool(torch.isfinite(direct).all())
    gn = g.cpu().numpy().reshape(3, neq, n).transpose(1, 0, 2)
    op.close()
    ref = sfu.integrate(c.mesh, 2, 0, *sfu.patch_faces_np(c.mesh, [1, 2, 3]), 3, gn, sfu.FLUX)
    sfu.check("test_gradients_go_in_as_they_are: flux", direct.cpu().numpy(), ref, log=_RATIOS)


# ---- 8. argument checks and lifecycle ------------------------------------------------------------------------------------------
def test_refusals_info_and_lifecycle():
    import torch
    from tps_amd.rhs_operator import TpsRhsError

    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    mesh = meshgen.box_hex(3, 2, 2, periodic=(False,) * 3)
    op, other = _operator(_case(mesh, 1)), _operator(_case(mesh, 1))
    i32 = lambda *v: np.array(v, dtype=np.int32)

    def create(npatch, e, f, p, h=op._h, out=True):
        s = C.c_void_p()
        st = lib.tpsrhs_surface_create(h, npatch, e.size, e.ctypes.data, f.ctypes.data, p.ctypes.data, C.byref(s) if out else None)
        return st, s

    for args in ((1, i32(0, 0), i32(1, 1), i32(0, 0)),      # a duplicate (element, face)
                 (2, i32(0, 0), i32(1, 1), i32(0, 1)),      # ... also in two patches
                 (1, i32(12), i32(0), i32(0)), (1, i32(-1), i32(0), i32(0)),  # an element outside 0 .. ne-1
                 (1, i32(0), i32(6), i32(0)), (1, i32(0), i32(-1), i32(0)),   # a face outside 0 .. 2 dim - 1
                 (1, i32(0), i32(0), i32(1)), (1, i32(0), i32(0), i32(-1)),   # a patch outside 0 .. num_patches-1
                 (0, i32(0), i32(0), i32(0))):                                # num_patches < 1
        st, s = create(*args)
        assert st == bad and not s.value and b"tpsrhs_surface_create" in lib.tpsrhs_last_error(), args
    assert create(1, i32(0), i32(0), i32(0), h=None)[0] == bad
    assert create(1, i32(0), i32(0), i32(0), out=False)[0] == bad
    surf = op.createSurface(attributes=[1, 2, 3, 4, 5, 6, 42])
    npatch, nf, per = surf.info()
    assert (npatch, nf) == (7, 32) and list(per) == [4, 4, 6, 6, 6, 6, 0]
    assert lib.tpsrhs_surface_info(surf._s, None, None, None) == 0 and lib.tpsrhs_surface_info(None, None, None, None) == bad
    field = torch.ones(op.NDofs, dtype=torch.float64, device=op.device)
    out = torch.zeros(7 * 3, dtype=torch.float64, device=op.device)
    fp, outp = C.c_void_p(field.data_ptr()), C.c_void_p(out.data_ptr())
    n = op.NDofs
    assert lib.tpsrhs_surface_integrate(None, 0, 1, fp, n, n, 0, outp) == bad
    assert lib.tpsrhs_surface_integrate(surf._s, 0, 1, None, n, n, 0, outp) == bad
    assert lib.tpsrhs_surface_integrate(surf._s, 0, 1, fp, n, n, 0, None) == bad
    assert lib.tpsrhs_surface_integrate(surf._s, 0, 0, fp, n, n, 0, outp) == bad
    for form in (-1, 3):
        assert lib.tpsrhs_surface_integrate(surf._s, form, 1, fp, n, n, 0, outp) == bad
    assert lib.tpsrhs_surface_integrate(surf._s, 2, 1, fp, n, n, 0, outp) == 0
    torch.cuda.synchronize()
    # a surface of another operator is refused by the history; negative interval, no capacity
    assert lib.tpsrhs_surface_monitor_configure(other._h, surf._s, 1, 4) == bad
    assert b"another operator" in lib.tpsrhs_last_error()
    for args in ((-1, 4), (1, -4), (1, 0)):
        assert lib.tpsrhs_surface_monitor_configure(op._h, surf._s, *args) == bad
    assert lib.tpsrhs_surface_monitor_configure(None, surf._s, 1, 4) == bad
    assert lib.tpsrhs_surface_monitor_read(op._h, None, None, None, None, None, None, 0) == bad  # not configured
    with pytest.raises(TpsRhsError):
        op.readSurfaceMonitor()
    with pytest.raises(ValueError):
        surf.integrate(field, "area")
    # close twice; destroy of NULL; an operator destroyed with surfaces alive frees them (the samplers' rule)
    surf_raw = surf._s.value
    surf.close()
    surf.close()
    assert lib.tpsrhs_surface_destroy(None) == 0
    alive = other.createSurface(attributes=[1])
    held = other.createSurface(attributes=[2])
    other.surfaceMonitor(held, 1, 2)
    dead = [C.c_void_p(alive._s.value), C.c_void_p(held._s.value)]
    other.close()
    assert alive._s is None and held._s is None
    alive.close()
    # the handles died with their operator: refused from the library's list of live surfaces, nothing of them is read
    for s in dead:
        assert lib.tpsrhs_surface_destroy(s) == bad and b"live operator" in lib.tpsrhs_last_error()
        assert lib.tpsrhs_surface_info(s, None, None, None) == bad
        assert lib.tpsrhs_surface_integrate(s, 0, 1, fp, n, n, 0, outp) == bad
        assert lib.tpsrhs_surface_monitor_configure(op._h, s, 1, 4) == bad
    gone = C.c_void_p(surf_raw)
    assert lib.tpsrhs_surface_destroy(gone) == bad  # destroyed twice through the C ABI
    op.close()
