"""The LDS window of the Coulomb-fit table (physics_plasma.hpp: coll::Window, the third route of the table next to the
wave-uniform and the per-lane one).  A lane's bits must not depend on its route, so everything here is compared bit for bit:
(a) the probe tpsrhs_coulomb_eval, route 3 (window) against route 2 (lane by lane; tests/test_gpu_coulomb_table.py pins that
    one to the host and to 40 digits), on argument sets built per 64-lane wave;
(b) one Mult of the case of tests/test_gpu_coulomb_paths.py, window on against TPSRHS_COULOMB_WINDOW=0: y, Up, gradUp;
(c) three RK4 steps through advance -- captured graph and launch loop -- window on against off: x."""
import ctypes as C

import numpy as np
import pytest

from parity_util import hip_mult
from test_gpu_coulomb_paths import _case
from tps_amd import capi, cases
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu

# tps_amd/csrc/coulomb_table.hpp (tests/test_coulomb_table.py::test_layout checks them)
X0, H, NI = -4.0, 0.25, 176
XEND = X0 + NI * H
# the probe's window: intervals it holds, blocks of the probe (include/tpsrhs.h: chunk c of 64 arguments goes to block c % BLOCKS)
W, BLOCKS = 2, 4
# the sweeps' windows (kernels.hpp: TPSRHS_COULOMB_WINDOW_GRAD, TPSRHS_COULOMB_WINDOW_FLUX)
W_SWEEPS = (4, 3)
PER_LANE, WINDOW = 2, 3
AMP = 0.01


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def dev(route, x):
    import torch

    lib = capi.load()
    xd = torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device="cuda")
    out = torch.empty((8, xd.numel()), dtype=torch.float64, device="cuda")
    assert lib.tpsrhs_coulomb_eval(route, xd.numel(), C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr())) == 0
    return out.cpu().numpy()


def _in(rng, i, n=None):
    """arguments inside interval(s) i, away from the edges by more than the rounding of (x - X0) / H"""
    i = np.asarray(i, dtype=np.float64)
    return X0 + H * (i + rng.uniform(0.05, 0.95, i.shape if n is None else n))


def _chunks():
    """(name, 64 arguments) per wave-sized chunk"""
    rng = np.random.default_rng(20)
    off = np.array([np.nan, X0 - 1.0, np.nextafter(X0, -np.inf), XEND, XEND + 3.0, -np.inf, np.inf, -50.0])
    out = []
    out.append(("one interval", _in(rng, np.full(64, 37))))
    two = np.full(64, 41)
    two[63] = 40  # the lowest interval only in the last lane: the wave's minimum is not its first lane's
    out.append(("lower interval in the last lane", _in(rng, two)))
    out.append(("descending intervals", _in(rng, 60 - np.arange(64) // 16)))  # one trip of the minimum search per interval
    out.append(("spread over W + 2 intervals", _in(rng, 50 + np.arange(64) % (W + 2))))
    out.append(("spread over 64 intervals", _in(rng, rng.permutation(NI)[:64])))
    mix = _in(rng, 70 + np.arange(64) % 2)
    mix[1::4] = X0 - 0.5 - np.arange(16)
    mix[2::4] = XEND + np.arange(16)
    mix[3::4] = np.nan
    out.append(("on the table / below / above / NaN alternating", mix))
    one = np.tile(off, 8)
    one[29] = _in(rng, np.array([90]))[0]
    out.append(("one lane on the table", one))
    out.append(("no lane on the table", np.tile(off, 8)))
    out.append(("top interval (the clamp)", _in(rng, np.full(64, NI - 1))))
    top = _in(rng, NI - 1 - np.arange(64) % 3)
    top[0] = np.nextafter(XEND, -np.inf)
    out.append(("top three intervals", top))
    out.append(("bottom interval", np.concatenate([[X0], _in(rng, np.zeros(63))])))
    return out


def test_probe_window_against_per_lane_per_wave():
    """every chunk alone (a fresh window), n = 64 and, cut short, n = 50 and n = 1 (ranks among 50 lanes and one)"""
    with np.errstate(all="ignore"):
        for name, x in _chunks():
            for n in (64, 50, 1):
                got, ref = dev(WINDOW, x[:n]), dev(PER_LANE, x[:n])
                assert np.array_equal(bits(got), bits(ref)), f"{name}, n = {n}"


def test_probe_window_carried_from_chunk_to_chunk():
    """A wave evaluates chunks b, b + BLOCKS, b + 2 BLOCKS, ... with ONE window: per wave a sequence in which a chunk fits the
    window its predecessor left (nothing is loaded), sits one interval above it (half of the lanes beyond the window), below
    it, far from it, follows a chunk without a lane on the table, and ends at the table's top; n is no multiple of 64."""
    rng = np.random.default_rng(21)
    named = dict(_chunks())
    seq = [
        _in(rng, np.full(64, 30)),                 # loads [30, 31]
        _in(rng, 30 + np.arange(64) % 2),          # fits
        _in(rng, 31 + np.arange(64) % 2),          # lowest interval 31 is held: 32 goes lane by lane
        _in(rng, 29 + np.arange(64) % 3),          # below: reload at 29, 31 beyond the window
        named["no lane on the table"],             # the window stays
        _in(rng, np.full(64, 30)),                 # ... and still serves
        named["on the table / below / above / NaN alternating"],
        _in(rng, 120 + np.arange(64) % (W + 2)),   # far away
        named["top interval (the clamp)"],
        _in(rng, NI - 2 - np.arange(64) % 2),      # held after the clamp (base NI - W), and one interval below it
        named["one lane on the table"],
        _in(rng, np.full(64, 90)),                 # the window that single lane loaded
    ]
    nseq = len(seq)
    x = np.empty((nseq, BLOCKS, 64))
    for b in range(BLOCKS):  # the waves run the sequence rotated against each other
        for k in range(nseq):
            x[k, b] = seq[(k + 3 * b) % nseq]
    x = x.reshape(-1)[: nseq * BLOCKS * 64 - 23]
    assert len(x) % 64 != 0
    with np.errstate(all="ignore"):
        got, ref = dev(WINDOW, x), dev(PER_LANE, x)
    assert np.array_equal(bits(got), bits(ref))
    on = (x >= X0) & (x < XEND)
    assert np.all(np.isfinite(got[:, on])) and 0.5 < on.mean() < 1.0


# ---- one Mult ------------------------------------------------------------------------------------------------------------
def _on_off(c, U, monkeypatch):
    monkeypatch.delenv("TPSRHS_COULOMB_TABLE", raising=False)
    monkeypatch.delenv("TPSRHS_COULOMB_WINDOW", raising=False)
    on = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U)
    monkeypatch.setenv("TPSRHS_COULOMB_WINDOW", "0")
    off = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U)
    monkeypatch.delenv("TPSRHS_COULOMB_WINDOW")
    return on, off


def _assert_identical(on, off):
    for k in ("y", "Up", "gradUp"):
        assert np.array_equal(bits(on[k]), bits(off[k])), k


def _ln_tp(ni, Th):
    """ln Tp of the nodes (PlasmaPhys::debye: the constants of physics_plasma.hpp), n_e = n_i, T_e = T_h -- as
    tests/test_gpu_coulomb_paths.py computes it"""
    NA, qe, eps0 = 6.0221409e+23, 1.60218e-19, 8.8541878128e-12
    dfac = (8.3144598 / NA) * eps0 / qe / qe
    return np.log(4.0 * np.pi * dfac * np.sqrt(dfac / NA / (2.0 * ni / Th)) * Th)


def _state(c, Th, alpha, w):
    """half-ionised-style state of tests/test_gpu_coulomb_paths.py: ionisation degree alpha at temperature Th, 1 atm"""
    ph = c.physics
    p = 101300.0 * (1.0 + 0.01 * w())
    nh = p / (capi.UNIVERSALGASCONSTANT * Th * (1.0 + alpha))
    ni = alpha * nh
    nsp = 3
    mw = [ph.mixture.gas_params[sp + capi.SPECIES_MW * nsp] for sp in range(nsp)]
    rho = ni * mw[0] + ni * mw[1] + (nh - ni) * mw[2]
    vel = [20.0 + 0.2 * w(), 0.2 * w(), 0.2 * w()]
    return cases.plasma_conserved(ph, 3, rho, vel, Th, [ni], None), ni


@pytest.mark.parametrize("ambipolar", [True, False])
@pytest.mark.parametrize("third_order", [True, False])
def test_mult_window_on_against_off(ambipolar, third_order, monkeypatch):
    c = _case(ambipolar, third_order)
    U = c.state(seed=21, amp=AMP)
    on, off = _on_off(c, U, monkeypatch)
    assert np.all(np.isfinite(on["y"]))
    _assert_identical(on, off)


def test_mult_cold_half_ionised(monkeypatch):
    """lanes of one wave split between the table (through the window) and the formulas"""
    c = _case(True, True)
    w = cases._waves(node_coordinates(c.mesh, 3), 21, kmax=1)
    Th = 600.0 + 300.0 * w()
    U, ni = _state(c, Th, 0.5 * np.ones_like(Th), w)
    below = float((_ln_tp(ni, Th) < X0).mean())
    assert 0.1 < below < 0.9
    on, off = _on_off(c, U, monkeypatch)
    assert np.all(np.isfinite(on["y"]))
    _assert_identical(on, off)


def _steep(c):
    """T_h = 3 000 K exp(1.5 s^3) along the normalised first coordinate s: ln Tp ~ 2 ln T_h is flat within the hexes at small
    s and crosses many intervals within those at large s"""
    X = node_coordinates(c.mesh, 3)
    w = cases._waves(X, 22, kmax=1)
    x = X[0]
    s =(x - x.min()) / (x.max() - x.min())
    Th = 3000.0 * np.exp(1.5 * s ** 3) * (1.0 + 0.002 * w())
    U, ni = _state(c, Th, 0.05 * np.ones_like(Th), w)
    return U, _ln_tp(ni, Th)


def test_mult_steep_state(monkeypatch):
    """hexes whose nodes the window holds altogether, and hexes that span W + 2 intervals or more (lanes beyond the window),
    for the window of either sweep"""
    c = _case(True, True)
    U, x = _steep(c)
    assert x.min() >= X0 and x.max() < XEND
    idx = np.floor((x - X0) / H).astype(int).reshape(-1, 64)  # nodes of a p = 3 hex are consecutive
    span = idx.max(axis=1) - idx.min(axis=1) + 1
    print(f"intervals per hex: {np.bincount(span)}")
    for w in W_SWEEPS:
        within, beyond = float((span <= w).mean()), float((span >= w + 2).mean())
        print(f"W = {w}: within the window {within:.2f}, W + 2 or more {beyond:.2f}")
        assert within >= 0.1 and beyond >= 0.1
    on, off = _on_off(c, U, monkeypatch)
    assert np.isfinite(on["y"]).mean() > 0.99
    _assert_identical(on, off)


def test_mult_one_nan_node(monkeypatch):
    c = _case(True, True)
    U = c.state(seed=21, amp=AMP)
    U[:, 64 * 40 + 21] = np.nan
    with np.errstate(all="ignore"):
        on, off = _on_off(c, U, monkeypatch)
    assert np.isnan(on["y"]).any() and np.isfinite(on["y"]).any()
    _assert_identical(on, off)


# ---- time loop: the window does not collide with the epilogue's use of the pool (RkDev::ta_out) ---------------------------
def _advance(monkeypatch, c, U, env, window, dt0):
    import torch
    from tps_amd.rhs_operator import RHSoperator

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TPSRHS_COULOMB_WINDOW", "1" if window else "0")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs, stream=side)
        x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
        t, dt, bad = op.advance(x, 0.0, dt0, 3, True, 0.0, 0.0)
        side.synchronize()
        out = x.cpu().numpy()
        op.close()
    assert bad == 0 and t > 0.0
    return out


def test_time_loop_window_on_against_off(monkeypatch):
    """three RK4 steps (advance takes the captured step graph from three steps on), fused traces + graph and the plain launch
    loop: x bit for bit"""
    c = _case(True, True)
    U = c.state(seed=21, amp=AMP)
    y0 = hip_mult(c.mesh, c.disc, c.physics, c.bcs, U, want_grad=False)["y"]
    # a tenth of the fastest local time scale of the residual (as tests/test_gpu_time_loop.py takes it)
    dt0 = 0.1 / (np.abs(y0) / np.maximum(np.abs(U), 1e-300 + 1e-6 * np.abs(U).max(axis=1, keepdims=True))).max()
    fused = {"TPSRHS_FUSE_TRACES": "1", "TPSRHS_GRAPH": "1", "TPSRHS_SWEEP_ALT": "1"}
    plain = {"TPSRHS_FUSE_TRACES": "0", "TPSRHS_GRAPH": "0", "TPSRHS_SWEEP_ALT": "0"}
    for env in (fused, plain):
        on = _advance(monkeypatch, c, U, env, True, dt0)
        off = _advance(monkeypatch, c, U, env, False, dt0)
        assert np.all(np.isfinite(on)) and not np.array_equal(on, np.ascontiguousarray(U).ravel())
        assert np.array_equal(bits(on), bits(off)), env
