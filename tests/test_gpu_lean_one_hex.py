"""The one-hex form of the lean 3-D face kernel (kernels.hpp::visc_phase_lean1): the single-temperature argon-minimal ternary
mixture at p = 3, where a block is one hex.  Its line stages take their LDS offsets from LeanLane instead of the item loops
of trace_lines / interp1_lines, the lanes beyond the 50 face points of a direction pair interpolate a duplicate point, and
the nodal gradient is re-read through scalar field addresses.  The cases compare one Mult with the CPU oracle at the bound
of tests/test_gpu_parity.py: both kernel families that take this path (ambipolar or not), a wall that makes the face kernel
run its second pass (viscous isothermal / adiabatic) and one that skips the viscous term on its faces (inviscid), scrambled
element orientations, and an element count that is not a multiple of anything the launch could round to."""
import pytest

from test_gpu_parity import _boost_transport, _compare, _tol
from tps_amd import capi, cases, meshgen

pytestmark = pytest.mark.gpu

AMP = 0.01


@pytest.mark.parametrize("ambipolar", [True, False])
@pytest.mark.parametrize("wall", [capi.VISC_ISOTH, capi.VISC_ADIAB, capi.INV])
def test_argon_minimal_p3_cylinder(ambipolar, wall):
    ph = capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL, "arrhenius", ambipolar=ambipolar)
    _boost_transport(ph)
    c = cases.argon_cyl3d(3, 11, 3, 3, wall_type=wall, physics=ph)
    c.mesh = meshgen.scramble_orientations(c.mesh, 5)
    _compare(c.mesh, c.disc, c.physics, c.bcs, c.state(seed=21, amp=AMP), tol=_tol(AMP))


@pytest.mark.parametrize("third_order", [False, True])
def test_argon_minimal_p3_periodic_box(third_order):
    """no boundary at all: every face interior, every orientation pair"""
    from tps_amd.rhs_operator import node_coordinates

    mesh = meshgen.scramble_orientations(meshgen.box_hex(3, 4, 3, lengths=(1.0, 0.8, 1.2), warp=0.1), 7)
    ph = capi.argon_ternary_physics(capi.NS, False, capi.ARGON_MINIMAL, "arrhenius", third_order_ke=third_order)
    _boost_transport(ph)
    U = cases.plasma_state(node_coordinates(mesh, 3), ph, nvel=3, seed=4, amp=AMP)
    _compare(mesh, capi.Disc(3, 0, 0, 0, 0), ph, [], U, tol=_tol(AMP))
