"""The numpy restatement of the running statistics (tests/statistics_util.py) against closed forms: it is what the device
kernel is compared with (tests/test_gpu_statistics.py), so it is pinned here, without a GPU."""
import numpy as np
import pytest

import statistics_util as su

N = 7


def _sample(rng, nvel, neq):
    """(prim, pressure) with entries of order one; the temperature row is never what is averaged"""
    return rng.normal(size=(neq, N)), rng.normal(size=N)


@pytest.mark.parametrize("nvel", [2, 3])
def test_constant_samples(nvel):
    rng = np.random.default_rng(1)
    prim, p = _sample(rng, nvel, nvel + 3)
    mean, vari, nm, nv = su.run([(prim, p)] * 6, nvel)
    assert nm == nv == 6
    # (k s + s) / (k + 1) rounds, so the mean is the sample to a few ulp, and the covariances are products of such errors
    s = su.sample_of(prim, p, nvel)
    assert np.abs(mean - s).max() <= 8 * su.EPS * np.abs(s).max()
    assert np.abs(mean[1 + nvel] - p).max() <= 8 * su.EPS * np.abs(p).max()
    assert np.abs(vari).max() <= (8 * su.EPS) ** 2 * np.abs(s).max() ** 2
    # one sample: exact
    mean, vari, nm, nv = su.run([(prim, p)], nvel)
    assert np.array_equal(mean, su.sample_of(prim, p, nvel)) and not vari.any() and nm == nv == 1


@pytest.mark.parametrize("nvel", [2, 3])
def test_two_samples_closed_form(nvel):
    rng = np.random.default_rng(2)
    (pa, qa), (pb, qb) = _sample(rng, nvel, nvel + 2), _sample(rng, nvel, nvel + 2)
    mean, vari, nm, nv = su.run([(pa, qa), (pb, qb)], nvel)
    a, b = su.sample_of(pa, qa, nvel), su.sample_of(pb, qb, nvel)
    assert nm == nv == 2
    assert np.allclose(mean, (a + b) / 2, rtol=0, atol=4 * su.EPS * np.abs([a, b]).max())
    for row, (i, j) in enumerate(su.pairs(nvel)):
        want = (b[1 + i] - a[1 + i]) * (b[1 + j] - a[1 + j]) / 8  # NOT the textbook (b - a)^2 / 4
        assert np.allclose(vari[row], want, rtol=0, atol=16 * su.EPS * np.abs([a, b]).max() ** 2), (i, j)


def test_mean_is_the_arithmetic_mean():
    rng = np.random.default_rng(3)
    nvel, S = 3, 40
    samples = [_sample(rng, nvel, 6) for _ in range(S)]
    mean, _, nm, _ = su.run(samples, nvel)
    want = np.mean([su.sample_of(prim, p, nvel) for prim, p in samples], axis=0)
    assert nm == S
    assert np.abs(mean - want).max() <= 4 * S * su.EPS * max(np.abs(prim).max() for prim, _ in samples)


def test_restart_rms_restarts_only_the_covariances():
    rng = np.random.default_rng(4)
    nvel = 3
    samples = [_sample(rng, nvel, 5) for _ in range(5)]
    st = su.Statistics(5, N, nvel)
    for prim, p in samples[:3]:
        st.add(prim, p)
    assert st.vari.any()
    st.restart_rms()
    st.add(*samples[3])
    assert (st.ns_mean, st.ns_vari) == (4, 1)
    # the first sample after the restart: vari = d_i d_j with d against the mean of all FOUR samples
    mean4 = su.run(samples[:4], nvel)[0]
    assert np.array_equal(st.mean, mean4)
    d = su.sample_of(*samples[3], nvel)[1:4] - mean4[1:4]
    for row, (i, j) in enumerate(su.pairs(nvel)):
        assert np.array_equal(st.vari[row], d[i] * d[j] / 1.0)
    st.add(*samples[4])
    assert (st.ns_mean, st.ns_vari) == (5, 2)
    assert np.array_equal(st.mean, su.run(samples, nvel)[0])


def test_nan_fields_are_harmless_at_counter_zero():
    rng = np.random.default_rng(5)
    nvel = 2
    prim, p = _sample(rng, nvel, 4)
    nan_mean, nan_vari = np.full((4, N), np.nan), np.full((3, N), np.nan)
    st = su.Statistics(4, N, nvel, mean=nan_mean, vari=nan_vari).add(prim, p)
    assert np.array_equal(st.mean, su.sample_of(prim, p, nvel)) and not st.vari.any()
    # ... and only there: a counter above 0 keeps what the field holds
    st = su.Statistics(4, N, nvel, mean=nan_mean, vari=nan_vari, ns_mean=1, ns_vari=0).add(prim, p)
    assert np.isnan(st.mean).all() and np.isnan(st.vari).all()  # d = s - NaN


def test_row_order():
    assert su.pairs(3) == [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]  # uu vv ww uv uw vw
    assert su.pairs(2) == [(0, 0), (1, 1), (0, 1)]                          # uu vv uv
    assert su.num_variances(3) == 6 and su.num_variances(2) == 3
    # the rows really are those products: samples that differ in ONE velocity component move exactly the rows with it
    for nvel in (2, 3):
        neq = nvel + 2
        for comp in range(nvel):
            a, b = np.ones((neq, N)), np.ones((neq, N))
            b[1 + comp] = 3.0
            _, vari, _, _ = su.run([(a, np.ones(N)), (b, np.ones(N))], nvel)
            for row, (i, j) in enumerate(su.pairs(nvel)):
                want = (2.0 * 2.0 / 8) if i == j == comp else 0.0
                assert np.array_equal(vari[row], np.full(N, want)), (nvel, comp, i, j)
    # the pressure replaces row 1 + nvel and nothing else
    prim = np.arange(5 * N, dtype=float).reshape(5, N)
    s = su.sample_of(prim, -np.ones(N), 3)
    assert np.array_equal(s[4], -np.ones(N)) and np.array_equal(s[:4], prim[:4])
    s = su.sample_of(prim, -np.ones(N), 2)
    assert np.array_equal(s[3], -np.ones(N)) and np.array_equal(s[4], prim[4])
