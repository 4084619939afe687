"""k_locate (tpsrhs_sampler_create_device) against the host locator tpsrhs_locate_points, which runs the same per-point text
(point_locate.hpp::locate_one) without FMA contraction: the element of every point identical, the reference coordinates
within 1e-12 -- Newton stops at a correction of 1e-13 and what remains is rounding times the conditioning of a mildly warped
element, so ten times the stop criterion is the bound -- and the found count taken on the device equal to the host's.

About 1 900 points per mesh (31 blocks of one wave, the last one partly filled): interior points, images of reference points
with coordinates exactly 0 or 1 (faces, edges, vertices, where the lowest element index must win on both sides), points
outside, one NaN.  The tolerance is 1e-6, not the default 1e-10: a point may differ in its element only where the host's
reference coordinate lies within rounding of -tol or 1 + tol, the test asserts that no input lies within 1e-9 of those two
values, and with the default tolerance every point ON a face (coordinate 0, which is 1e-10 from -tol) would fall under that
guard; with 1e-6 none does, so no point is left out of the comparison."""
import numpy as np
import pytest

import transfer_util as tu
from tps_amd import capi, cases
from tps_amd.rhs_operator import locate_points

pytestmark = pytest.mark.gpu

TOL = 1.0e-6
GUARD = 1.0e-9


def _case(name):
    if name == "ogrid":
        return cases.cyl3d(4, 12, 3, 2, capi.NS, capi.VISC_ISOTH)
    return tu.box_case(tu.LOCATE_MESHES[name](), 2)


@pytest.mark.parametrize("name", list(tu.LOCATE_MESHES))
def test_device_location_equals_the_host_locator(name):
    import torch

    from tps_amd.rhs_operator import RHSoperator

    c = _case(name)
    xyz = tu.point_set(c.mesh, 1200, 700, seed=31)
    npts = xyz.shape[1]
    assert npts % 64 != 0 and npts > 64 * 20
    e_host, r_host = locate_points(c.mesh, xyz, tol=TOL)
    found = e_host >= 0
    # the guard of the comparison, on the host result: no accepted coordinate near -tol or 1 + tol, so nothing is left out
    near = np.minimum(np.abs(r_host[:, found] + TOL), np.abs(r_host[:, found] - (1.0 + TOL)))
    assert near.min() > GUARD
    assert found.sum() == 1900 and (~found).sum() == npts - 1900
    op = RHSoperator(c.mesh, c.disc, c.physics, c.bcs)
    s = op.createSampler(torch.tensor(xyz, dtype=torch.float64, device=op.device), tol=TOL, fill=-3.0)
    e_dev, r_dev, nfound = s.info()
    # a device sampler samples like any other: the constant 1 at the found points, the fill value elsewhere
    ones = s.sample(torch.ones(op.NDofs, dtype=torch.float64, device=op.device)).cpu().numpy()[0]
    op.close()
    dref = np.abs(r_dev - r_host).max()
    print(f"{name}: {npts} points, {int(found.sum())} found, max |ref_dev - ref_host| = {dref:.2e}, "
          f"elements differing: {int((e_dev != e_host).sum())}")
    assert np.array_equal(e_dev, e_host)
    assert dref <= 1e-12
    assert not r_dev[:, ~found].any()  # zeros for a point that was not found, as on the host
    assert nfound == int(found.sum())
    assert np.abs(ones[found] - 1.0).max() <= 1e-13 and (ones[~found] == -3.0).all()
