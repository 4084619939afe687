"""Dump the two-dimensional local-thermodynamic-equilibrium tables of the reference's own unit test
(test/test_lte_mixture.cpp:16-30, `flow/lte/table_dim = 2`, the variant of test/inputs/plasma.lte2d.ini) into one fixture:
    test/inputs/argon_lte_thermo_table.dat       101 temperatures x 11 densities; the columns LteMixture reads
                                                 (src/lte_mixture.cpp:48-58): 0 T, 1 rho, 3 e, 6 R, 8 c
    test/inputs/argon_lte_e_rev_table.dat        101 energies x 11 densities -> T (:60-64), the first guess of the Newton iteration
    test/inputs/air_simple_transport_table.dat   200 temperatures x 150 densities, columns T, rho, mu, kappa, sigma
                                                 (src/lte_transport_properties.cpp:38-51)
Stored as the reference stores them (src/table.cpp:195-207): axes x[nx], y[ny] and values f[j, i] at (x[i], y[j]).
    thermo_T, thermo_rho, thermo_e, thermo_R, thermo_c     the full grid
    erev_e, erev_rho, erev_T                               the full grid
    trans_T, trans_rho, trans_mu, trans_kappa, trans_sigma all 200 temperatures, three of the 150 densities (first, middle, last)
The transport file does not depend on the density (asserted below), so every density line equals the first and bilinear
interpolation between three of them gives what it gives between all 150: the decimation is exact.
Run where a checkout of the reference exists (TPS_REFERENCE_DIR, default /root/reference):
    python tests/golden/tables/make_lte_tables_2d.py      -> lte_tables_2d.npz
The values are the decimal numbers of the files parsed by numpy (float64).  Data only.
"""
import os

import numpy as np

REF = os.path.join(os.environ.get("TPS_REFERENCE_DIR", "/root/reference"), "test", "inputs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lte_tables_2d.npz")


def read2d(path):
    """(x[nx], y[ny], columns[ncol, ny, nx]) of a file whose first line is `nx ny` and whose x runs fastest"""
    with open(path) as f:
        nx, ny = (int(v) for v in f.readline().split())
        data = np.loadtxt(f)
    assert data.shape[0] == nx * ny, (path, data.shape, nx, ny)
    g = data.reshape(ny, nx, -1)
    x, y = g[0, :, 0].copy(), g[:, 0, 1].copy()
    assert np.all(g[:, :, 0] == x[None, :]) and np.all(g[:, :, 1] == y[:, None]), path  # a tensor grid
    assert np.all(np.diff(x) > 0) and np.all(np.diff(y) > 0), path
    return x, y, np.ascontiguousarray(np.moveaxis(g, 2, 0))


def tables(ref=REF):
    out = {}
    T, rho, col = read2d(os.path.join(ref, "argon_lte_thermo_table.dat"))
    assert np.all(np.diff(col[3], axis=1) > 0)  # e increases with T on every density line
    out.update(thermo_T=T, thermo_rho=rho, thermo_e=col[3], thermo_R=col[6], thermo_c=col[8])
    e, rho, col = read2d(os.path.join(ref, "argon_lte_e_rev_table.dat"))
    out.update(erev_e=e, erev_rho=rho, erev_T=col[2])
    T, rho, col = read2d(os.path.join(ref, "air_simple_transport_table.dat"))
    assert np.all(col[2:] == col[2:, :1, :])  # no density dependence: the decimation below is exact
    keep = [0, len(rho) // 2, len(rho) - 1]
    out.update(trans_T=T, trans_rho=rho[keep].copy(), trans_mu=col[2][keep].copy(), trans_kappa=col[3][keep].copy(),
               trans_sigma=col[4][keep].copy())
    return out


if __name__ == "__main__":
    t = tables()
    for k, v in t.items():
        print(f"{k}: {v.shape} {v.min():.6g} .. {v.max():.6g}")
    np.savez_compressed(OUT, **t)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
