"""tpsrhs_patch_faces through the C ABI on the CPU (host only: no device is touched) -- the faces, their order, the capacity
rules and the refusals -- the same selection in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/patch_faces_main.cpp: its own main, run as a child process, nothing loaded into Python), and the numpy restatement
of the surface rule (tests/surface_util.py) against closed forms, so that the GPU tests compare with something pinned."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import integrals_util as iu
import surface_util as sfu
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan"]  # the runtimes inside the program: nothing is preloaded


def _box():
    return meshgen.box_hex(3, 2, 2, periodic=(False,) * 3)


def _meshes():
    """(mesh, attributes): the box, the box with scrambled element frames, the ring"""
    return [(_box(), [1, 2, 3, 4, 5, 6]), (meshgen.scramble_orientations(_box(), 7), [1, 2, 3, 4, 5, 6]),
            (iu.ring_quad(), [3, 1, 2])]


def test_box_sides_hold_the_local_faces_of_their_elements():
    mesh = _box()
    elem, face, patch = capi.patch_faces(mesh, [1, 2, 3, 4, 5, 6])
    assert elem.dtype == face.dtype == patch.dtype == np.int32 and elem.size == 2 * (4 + 6 + 6)
    n = (3, 2, 2)
    cell = np.stack(np.unravel_index(np.arange(12), n, order="F"))  # element index: first direction fastest
    for d in range(3):
        for s in (0, 1):
            sel = patch == 2 * d + s
            want = np.where(cell[d] == (n[d] - 1 if s else 0))[0]
            assert np.array_equal(elem[sel], want)  # ascending
            assert (face[sel] == 2 * d + s).all()
    key = elem.astype(np.int64) * 6 + face
    assert (np.diff(key) > 0).all()
    for got, want in zip((elem, face, patch), sfu.patch_faces_np(mesh, [1, 2, 3, 4, 5, 6])):
        assert np.array_equal(got, want)


def test_scrambled_frames_give_the_same_physical_faces():
    mesh = _box()
    scr = meshgen.scramble_orientations(mesh, 7)
    a = capi.patch_faces(mesh, [1, 2, 3, 4, 5, 6])
    b = capi.patch_faces(scr, [1, 2, 3, 4, 5, 6])
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])  # the same elements, other local numbers
    ca, cb = sfu.face_centres(mesh, a[0], a[1]), sfu.face_centres(scr, b[0], b[1])
    for p in range(6):
        sa, sb = ca[a[2] == p], cb[b[2] == p]
        assert sa.shape == sb.shape
        assert np.allclose(sa[np.lexsort(sa.T)], sb[np.lexsort(sb.T)], rtol=0, atol=1e-14)
        assert np.allclose(sa[:, p >> 1], float(p & 1), rtol=0, atol=1e-14)
    for got, want in zip(b, sfu.patch_faces_np(scr, [1, 2, 3, 4, 5, 6])):
        assert np.array_equal(got, want)


def test_ring_wall_and_an_empty_patch():
    mesh = iu.ring_quad()
    elem, face, patch = capi.patch_faces(mesh, [3, 99, 1, 2])  # 99: no face carries it
    assert (patch == 0).sum() == 12 and (patch == 1).sum() == 0 and (patch == 2).sum() + (patch == 3).sum() == 12
    assert (face[patch == 0] == 0).all() and (face[patch >= 2] == 1).all()  # r = r_in is xi_0 = 0, the outer circle xi_0 = 1
    r = np.hypot(*sfu.face_centres(mesh, elem, face)[patch == 0].T)
    assert np.allclose(r, 0.5 * np.cos(np.pi / 12))
    e99 = capi.patch_faces(mesh, [99])
    assert all(a.size == 0 for a in e99)


def _raw(mesh, att, capacity, arrays=True, count=True):
    lib = capi.load()
    ma = capi.MeshArgs(mesh) if mesh is not None else None
    att = np.ascontiguousarray(att, dtype=np.int32)
    e, f, p = (np.full(max(capacity, 0) + 1, -7, dtype=np.int32) for _ in range(3))  # one guard entry each
    n = C.c_int64(-1)
    st = lib.tpsrhs_patch_faces(C.byref(ma.c) if ma is not None else None, int(att.size), att.ctypes.data if att.size else None,
                                capacity, *((a.ctypes.data if arrays else None) for a in (e, f, p)), C.byref(n) if count else None)
    return st, n.value, e, f, p


def test_capacity_count_and_null_rules():
    mesh = _box()
    full = capi.patch_faces(mesh, [2, 5])
    nf = full[0].size
    assert nf == 4 + 6
    st, n, *_ = _raw(mesh, [2, 5], 0, arrays=False)
    assert st == 0 and n == nf
    for cap in (1, nf - 1, nf, nf + 3):
        st, n, e, f, p = _raw(mesh, [2, 5], cap)
        w = min(cap, nf)
        assert st == 0 and n == nf
        for got, want in zip((e, f, p), full):
            assert np.array_equal(got[:w], want[:w]) and (got[w:] == -7).all()  # nothing behind min(count, capacity)


def test_refusals():
    lib = capi.load()
    mesh = _box()

    def refused(st):
        assert st == capi.ERR_INVALID_ARGUMENT
        assert b"tpsrhs_patch_faces" in lib.tpsrhs_last_error()

    refused(_raw(mesh, [1, 2, 1], 0, arrays=False)[0])   # an attribute listed twice
    refused(_raw(mesh, [], 0, arrays=False)[0])          # num_attributes < 1
    refused(_raw(None, [1], 0, arrays=False)[0])         # a NULL mesh
    refused(_raw(mesh, [1], -1, arrays=False)[0])        # negative capacity
    refused(_raw(mesh, [1], 2, arrays=False)[0])         # capacity without arrays
    refused(_raw(mesh, [1], 0, arrays=False, count=False)[0])
    import dataclasses

    bv = np.array(mesh.bdr_vertices)
    bv[0, :] = bv[0, 0]  # no element face has these vertices
    refused(_raw(dataclasses.replace(mesh, bdr_vertices=bv), [1], 0, arrays=False)[0])
    ma = capi.MeshArgs(mesh)
    ma.c.dim = 4
    n = C.c_int64(0)
    att = np.array([1], dtype=np.int32)
    refused(lib.tpsrhs_patch_faces(C.byref(ma.c), 1, att.ctypes.data, 0, None, None, None, C.byref(n)))


def _sanitizer_runtime_missing(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + FLAGS + [str(src), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    return r.returncode != 0


def test_selection_is_clean_under_asan_and_ubsan_and_agrees_with_the_library(tmp_path):
    # (skips, like the other *_sanitize tests, only where the toolchain cannot link the sanitizers' runtimes: a missing
    #  compiler feature decided before any work, not missing hardware; the comparison with the library is then
    #  test_box_sides_... and test_scrambled_..., which need no program)
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    exe = str(tmp_path / "patch_faces")
    b = subprocess.run(["g++"] + FLAGS + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "patch_faces_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    lines = []
    for mesh, att in _meshes():
        lines.append(f"{mesh.dim} {mesh.num_vertices} {mesh.num_elements} {len(mesh.bdr_attributes)} {len(att)}")
        lines.append(" ".join(str(a) for a in att))
        lines.append(" ".join(str(int(v)) for v in np.asarray(mesh.elem_vertices).ravel()))
        lines.append(" ".join(repr(float(v)) for v in np.asarray(mesh.elem_coords).ravel()))
        lines.append(" ".join(str(int(v)) for v in np.asarray(mesh.bdr_vertices).ravel()))
        lines.append(" ".join(str(int(v)) for v in np.asarray(mesh.bdr_attributes).ravel()))
    inp = tmp_path / "meshes.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PATCH FACES CLEAN" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = iter(r.stdout.split("\n"))
    for index, (mesh, att) in enumerate(_meshes()):
        want = capi.patch_faces(mesh, att)
        assert next(out) == f"mesh {index} {want[0].size}"
        got = np.array([[int(t) for t in next(out).split()] for _ in range(want[0].size)]).reshape(-1, 3)
        for k in range(3):
            assert np.array_equal(got[:, k], want[k])


# ---- the restatement against closed forms ---------------------------------------------------------------------------------
def test_polynomial_terms_are_those_of_integrals_util():
    for dim, p, seed in ((2, 3, 5), (3, 2, 9)):
        coef, terms = sfu.polynomial_terms(dim, p, seed)
        f, i1, _ = iu.polynomial(dim, p, seed)
        X = np.random.default_rng(1).uniform(size=(dim, 7))
        mine = sum(c * np.prod([X[d] ** e[d] for d in range(dim)], axis=0) for c, e in zip(coef, terms))
        assert np.allclose(mine, f(X), rtol=1e-14, atol=1e-15)
        assert np.isclose(sum(c * iu.monomial_integral_unit_box(e) for c, e in zip(coef, terms)), i1, rtol=1e-14)


@pytest.mark.parametrize("basis", [0, 1], ids=["legendre", "lobatto"])
@pytest.mark.parametrize("dim,order", [(2, 1), (2, 4), (3, 2), (3, 3)])
def test_restatement_integrates_polynomials_over_planar_box_faces(dim, order, basis):
    """planar, non-parallelogram boundary faces: SCALAR, NORMAL and FLUX of a polynomial of degree <= p are the closed
    forms over the faces of the unit box"""
    mesh = sfu.planar_box(dim, (3, 2, 2)[:dim])
    ex = np.asarray(mesh.elem_coords)
    assert ex.min() == 0.0 and ex.max() == 1.0 and not np.array_equal(ex, (meshgen.box_hex if dim == 3 else meshgen.box_quad)(
        *(3, 2, 2)[:dim], periodic=(False,) * dim).elem_coords)
    elem, face, patch = sfu.box_patches(mesh)
    X = node_coordinates(mesh, order, basis)
    polys = [sfu.polynomial_terms(dim, order, 100 + k) for k in range(dim)]
    F = np.stack([iu.polynomial(dim, order, 100 + k)[0](X) for k in range(dim)])  # (dim, NDofs)
    sc = sfu.integrate(mesh, order, basis, elem, face, patch, 2 * dim, F, sfu.SCALAR)
    nm = sfu.integrate(mesh, order, basis, elem, face, patch, 2 * dim, F, sfu.NORMAL)
    fl = sfu.integrate(mesh, order, basis, elem, face, patch, 2 * dim, F[None], sfu.FLUX)
    for d in range(dim):
        for s in (0, 1):
            p = 2 * d + s
            exact = np.array([sfu.box_face_integral(*polys[k], d, s) for k in range(dim)])
            tol = 64 * sfu.EPS * sc["S"][p]
            assert (np.abs(sc["val"][p] - exact) <= tol).all()
            unit = np.zeros(dim)
            unit[d] = 2 * s - 1
            assert (np.abs(nm["val"][p] - exact[:, None] * unit[None, :]) <= tol[:, None]).all()
            assert abs(fl["val"][p, 0] - (2 * s - 1) * exact[d]) <= 64 * sfu.EPS * fl["S"][p, 0]


def test_restatement_areas_of_the_ring_and_the_cylinder():
    ring = iu.ring_quad()
    e, f, p = sfu.patch_faces_np(ring, [3, 1, 2])
    ones = np.ones((1, ring.num_elements * 9))
    a = sfu.integrate(ring, 2, 0, e, f, p, 3, ones)["val"][:, 0]
    assert np.isclose(a[0], 12 * 2 * 0.5 * np.sin(np.pi / 12), rtol=1e-14)
    assert np.isclose(a[1] + a[2], 12 * 2 * 10.0 * np.sin(np.pi / 12), rtol=1e-14)
    c = cases.cyl3d(3, 8, 3, 1)
    e, f, p = sfu.patch_faces_np(c.mesh, [1, 2, 3])
    a = sfu.integrate(c.mesh, 1, 0, e, f, p, 3, np.ones((1, c.mesh.num_elements * 8)))["val"][:, 0]
    assert np.isclose(a[2], 8 * 2 * 0.5 * np.sin(np.pi / 8) * 2.0, rtol=1e-14)
    assert np.isclose(a[0] + a[1], 8 * 2 * 10.0 * np.sin(np.pi / 8) * 2.0, rtol=1e-14)
    # closed surfaces: the normals of the ring's whole boundary add up to zero
    e, f, p = sfu.patch_faces_np(ring, [1, 2, 3])
    nm = sfu.integrate(ring, 2, 0, e, f, np.zeros_like(p), 1, ones, sfu.NORMAL)
    assert (np.abs(nm["val"][0, 0]) <= 64 * sfu.EPS * nm["S"][0, 0]).all()
