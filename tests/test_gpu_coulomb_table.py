"""The polynomial table of the Coulomb fits on the device, through the probe tpsrhs_coulomb_eval: route 1 (wave-uniform
coefficient loads, then lane by lane) and route 2 (lane by lane) against each other, against the host evaluation of
tests/coulomb_table_main.cpp (bit for bit) and against 40-digit arithmetic (4e-15, as tests/test_coulomb_table.py);
a wave whose lanes all fall into different intervals against the same arguments sorted; arguments off the table and NaN
against the formulas (route 0), bit for bit."""
import ctypes as C

import numpy as np
import pytest

from test_coulomb_table import RTOL, build_program, reference, run_program, table_info, worst_rel
from tps_amd import capi

pytestmark = pytest.mark.gpu
FORMULA, UNIFORM, PER_LANE = range(3)


def dev(route, x):
    import torch

    lib = capi.load()
    xd = torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")
    out = torch.empty((8, xd.numel()), dtype=torch.float64, device="cuda")
    assert lib.tpsrhs_coulomb_eval(route, xd.numel(), C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr())) == 0
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("coulomb_table_gpu"))


@pytest.fixture(scope="module")
def arguments(program):
    """on the table: random (neighbours in a wave mostly in different intervals), sorted runs (a wave in one or two
    intervals), every interval edge with its neighbours, the range ends; 4 099 arguments: no multiple of a wave or a block"""
    x0, h, ni, deg, fits = table_info(program)
    xend = x0 + ni * h
    rng = np.random.default_rng(7)
    edges = x0 + h * np.arange(ni + 1)
    x = np.concatenate([rng.uniform(x0, xend, 1500), np.sort(rng.uniform(1.0, 9.0, 2069)), edges[:-1], np.nextafter(edges[1:], -np.inf),
                        np.nextafter(edges[:-1], np.inf), [x0, np.nextafter(xend, -np.inf)]])
    assert len(x) == 4099
    return x


def test_routes_and_host_agree_bitwise(program, arguments):
    on, host = run_program(program, arguments)
    assert on.all()
    g1, g2 = dev(UNIFORM, arguments), dev(PER_LANE, arguments)
    assert np.array_equal(bits(g1), bits(g2))
    assert np.array_equal(bits(g1.T), bits(host))


def test_accuracy(program, arguments):
    x0, h, ni, deg, fits = table_info(program)
    ref = reference(fits, arguments)
    for route in (UNIFORM, PER_LANE):
        w = worst_rel(dev(route, arguments).T, ref)
        print(f"route {route}: worst relative error against 40 digits: {w:.3e}")
        assert w < RTOL


def test_every_lane_its_own_interval(program):
    """three waves whose 64 lanes hold 64 different intervals, against the same arguments sorted (neighbours then share
    intervals): a lane's value does not depend on what the other lanes of its wave hold"""
    x0, h, ni, deg, fits = table_info(program)
    rng = np.random.default_rng(11)
    x = np.concatenate([x0 + h * (rng.permutation(ni)[:64] + rng.uniform(0.0, 1.0, 64)) for _ in range(3)])
    order = np.argsort(x)
    for route in (UNIFORM, PER_LANE):
        scattered, srt = dev(route, x), dev(route, x[order])
        assert np.array_equal(bits(scattered[:, order]), bits(srt))


def test_off_the_table_is_the_formula(program):
    x0, h, ni, deg, fits = table_info(program)
    xend = x0 + ni * h
    rng = np.random.default_rng(13)
    off = np.array([np.nan, np.nextafter(x0, -np.inf), xend, -np.inf, np.inf, -50.0, -4.5, 41.0, 300.0, 1e300, -1e300, -0.0 - 700.0])
    # off-table lanes alone in their wave, and mixed with lanes on the table
    x = np.concatenate([np.tile(off, 6)[:64], rng.uniform(x0, xend, 64), np.tile(off, 6)[:64]])
    x[64:128:3] = off[np.arange(len(x[64:128:3])) % len(off)]
    is_off = ~((x >= x0) & (x < xend))
    with np.errstate(all="ignore"):
        g0 = dev(FORMULA, x)
        for route in (UNIFORM, PER_LANE):
            g = dev(route, x)
            assert np.array_equal(bits(g[:, is_off]), bits(g0[:, is_off]))
            assert np.all(np.isfinite(g[:, ~is_off]))
