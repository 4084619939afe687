"""The running statistics of the device time loop restated in numpy: what ``tpsrhs_stats_add_sample`` and the sampling
inside ``tpsrhs_advance`` are tested against.  ``tests/test_statistics_restatement.py`` pins it by closed forms.

The recurrence is the reference's ``Averaging::addSample`` / ``addSampleInternal`` (``src/averaging.cpp:198-234, 331-435``),
in its order of operations.  One sample ``s`` = the primitives with the temperature row ``1 + nvel`` replaced by the
pressure:

    mean = (ns_mean * mean + s) / (ns_mean + 1)                                   every row
    vari = (vari * ns_vari + d_i * d_j) / (ns_vari + 1),  d_i = s_i - mean_i      with the UPDATED mean, velocity rows

then both counters go up by one.  A field whose counter is 0 is set to zero first.  The covariance rows are the diagonal
first, then the pairs i < j in row-major order: uu vv ww uv uw vw for nvel = 3, uu vv uv for nvel = 2
(``src/M2ulPhyS.cpp:665-675``).  Not the textbook variance: two samples a, b give (b - a)^2 / 8.
"""
import numpy as np

EPS = 2.0 ** -52


def pairs(nvel):
    """(i, j) of every covariance row, velocity components counted from 0"""
    return [(i, i) for i in range(nvel)] + [(i, j) for i in range(nvel - 1) for j in range(i + 1, nvel)]


def num_variances(nvel):
    return nvel * (nvel + 1) // 2


def sample_of(prim, pressure, nvel):
    """what one sample contributes: the primitives with the pressure in the temperature row"""
    s = np.array(prim, dtype=np.float64)
    s[1 + nvel] = pressure
    return s


class Statistics:
    """mean (neq, n), vari (nvar, n), ns_mean, ns_vari.  `mean` / `vari` given: continuation; whatever they hold is dropped
    when the counter is 0."""

    def __init__(self, neq, n, nvel, mean=None, vari=None, ns_mean=0, ns_vari=0):
        self.nvel = nvel
        self.mean = np.zeros((neq, n)) if mean is None else np.array(mean, dtype=np.float64)
        self.vari = np.zeros((num_variances(nvel), n)) if vari is None else np.array(vari, dtype=np.float64)
        self.ns_mean, self.ns_vari = int(ns_mean), int(ns_vari)

    def restart_rms(self):
        self.ns_vari = 0

    def add(self, prim, pressure):
        s = sample_of(prim, pressure, self.nvel)
        if self.ns_mean == 0:
            self.mean[:] = 0.0
        if self.ns_vari == 0:
            self.vari[:] = 0.0
        nm, nv = float(self.ns_mean), float(self.ns_vari)
        self.mean = (nm * self.mean + s) / (nm + 1.0)
        d = s[1:1 + self.nvel] - self.mean[1:1 + self.nvel]
        for row, (i, j) in enumerate(pairs(self.nvel)):
            self.vari[row] = (self.vari[row] * nv + d[i] * d[j]) / (nv + 1.0)
        self.ns_mean += 1
        self.ns_vari += 1
        return self


def run(samples, nvel):
    """`samples`: a sequence of (prim, pressure) -> (mean, vari, ns_mean, ns_vari)"""
    st = None
    for prim, p in samples:
        if st is None:
            st = Statistics(prim.shape[0], prim.shape[1], nvel)
        st.add(prim, p)
    return st.mean, st.vari, st.ns_mean, st.ns_vari


def bounds(samples, nvel, extra_rel=0.0):
    """Per row, the largest |device - restatement| that rounding allows after the S samples given: each update rounds at
    most four times (product, sum, division; the difference d for the covariances), and the device may fuse the product
    into the sum where numpy rounds both -- 8 S eps of the row's scale covers both.  The scale of a mean row is the largest
    |s| of the row over the samples; of a covariance row (i, j), the largest max |s_i| max |s_j| of one sample.  `extra_rel`: a relative difference
    of the samples themselves (states from another run), on the same scales."""
    S = len(samples)
    rowmax = np.array([np.abs(sample_of(prim, p, nvel)).max(axis=1) for prim, p in samples])  # (S, neq)
    vel = rowmax[:, 1:1 + nvel]
    mean_b = (8 * S * EPS + extra_rel) * rowmax.max(axis=0)
    vari_b = (8 * S * EPS + extra_rel) * np.array([(vel[:, i] * vel[:, j]).max() for i, j in pairs(nvel)])
    return mean_b, vari_b
