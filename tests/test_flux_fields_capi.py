"""tpsrhs_get_flux / tpsrhs_surface_loads without a device: the symbols exist and the refusals come before any device work
(the way tests/test_capi_cpu.py calls the library)."""
import ctypes as C

from tps_amd import capi

INVALID = 1  # TPSRHS_ERR_INVALID_ARGUMENT


def test_symbols_exist_and_are_declared():
    lib = capi.load()
    for name in ("tpsrhs_get_flux", "tpsrhs_surface_loads"):
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS
    assert (capi.FLUX_TOTAL, capi.FLUX_CONVECTIVE, capi.FLUX_VISCOUS) == (0, 1, 2)
    assert [capi.flux_part(p) for p in ("total", "convective", "viscous")] == [0, 1, 2]


def test_header_declares_what_the_library_exports():
    import os

    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "tpsrhs.h")).read()
    assert "enum tpsrhs_flux_part { TPSRHS_FLUX_TOTAL = 0, TPSRHS_FLUX_CONVECTIVE = 1, TPSRHS_FLUX_VISCOUS = 2 };" in hdr
    assert "int tpsrhs_get_flux(tpsrhs_handle h, const double *x, int part, int gradients_current, double *out);" in hdr
    assert "int tpsrhs_surface_loads(tpsrhs_surface_handle s, const double *x, int part, int gradients_current, double *out);" in hdr


def test_get_flux_refuses_before_any_device_work():
    lib = capi.load()
    buf = (C.c_double * 8)()  # stands for a handle and for device arrays: none of them may be read
    p = C.cast(buf, C.c_void_p)
    assert lib.tpsrhs_get_flux(None, p, capi.FLUX_TOTAL, 0, p) == INVALID
    assert b"tpsrhs_get_flux" in lib.tpsrhs_last_error()
    assert lib.tpsrhs_get_flux(p, None, capi.FLUX_TOTAL, 0, p) == INVALID
    assert lib.tpsrhs_get_flux(p, p, capi.FLUX_TOTAL, 0, None) == INVALID
    for part in (-1, 3, 17):
        assert lib.tpsrhs_get_flux(p, p, part, 0, p) == INVALID
        assert b"part" in lib.tpsrhs_last_error()
    assert all(v == 0.0 for v in buf)


def test_surface_loads_refuses_a_dead_surface_and_null_arguments():
    lib = capi.load()
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.tpsrhs_surface_loads(None, p, capi.FLUX_TOTAL, 0, p) == INVALID
    assert lib.tpsrhs_surface_loads(p, None, capi.FLUX_TOTAL, 0, p) == INVALID
    assert lib.tpsrhs_surface_loads(p, p, capi.FLUX_TOTAL, 0, None) == INVALID
    # a pointer that is no live surface (never created, or its operator gone): nothing of it is read
    assert lib.tpsrhs_surface_loads(p, p, capi.FLUX_VISCOUS, 1, p) == INVALID
    assert b"not a surface of a live operator" in lib.tpsrhs_last_error()
    assert lib.tpsrhs_surface_loads(p, p, 5, 0, p) == INVALID
    assert all(v == 0.0 for v in buf)
