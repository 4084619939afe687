"""Statuses of the reactions with an external rate coefficient (model = bte) and of tpsrhs_boltzmann_fields: what
tpsrhs_create, tpsrhs_set_reaction_rates, tpsrhs_visualization_fields and tpsrhs_boltzmann_fields accept and refuse.  On the
GPU because tpsrhs_create needs a device; the rules themselves are host code (tests/test_external_rates_plan.py)."""
import numpy as np
import pytest

import external_rates_util as eu
from tps_amd import capi, cases

pytestmark = pytest.mark.gpu


def _case(physics=None):
    return cases.argon_axisym(2, 3, 1, physics=physics or capi.argon_ternary_physics(capi.NS, True, capi.CONSTANT, "arrhenius"))


def _create(c, physics):
    from tps_amd.rhs_operator import RHSoperator

    return RHSoperator(c.mesh, c.disc, physics, c.bcs)


def _status(fn):
    from tps_amd.rhs_operator import TpsRhsError

    with pytest.raises(TpsRhsError) as e:
        fn()
    return e.value.status


def _state(c, op):
    import torch

    return torch.tensor(np.ascontiguousarray(c.state()).ravel(), dtype=torch.float64, device=op.device)


def test_create_accepts_a_grid_function_reaction():
    c = _case()
    op = _create(c, eu.externalize(c.physics, {0: 0, 1: 3}))
    assert op.NDofs == 24
    op.close()


@pytest.mark.parametrize("component", [0.5, -1.0, -0.25, float("nan")])
def test_component_must_be_a_non_negative_integer(component):
    c = _case()
    ph = eu.externalize(c.physics, {1: 0})
    ph.chemistry.rate_params[0 + 1 * capi.MAXCHEMPARAMS] = component
    assert _status(lambda: _create(c, ph)) == capi.ERR_INVALID_ARGUMENT


def test_radiative_decay_stays_unsupported():
    c = _case()
    ph = eu.copy_physics(c.physics)
    ph.chemistry.reaction_models[1] = capi.RADIATIVE_DECAY
    assert _status(lambda: _create(c, ph)) == capi.ERR_UNSUPPORTED


def test_set_reaction_rates_checks_the_array():
    import torch

    c = _case()
    op = _create(c, eu.externalize(c.physics, {0: 0, 1: 3}))
    n = op.NDofs

    def rates(ncomp, size):
        return torch.zeros((ncomp, size), dtype=torch.float64, device=op.device)

    assert _status(lambda: op.setReactionRates(rates(4, n + 1))) == capi.ERR_INVALID_ARGUMENT  # size != NDofs
    assert _status(lambda: op.setReactionRates(rates(4, n - 1))) == capi.ERR_INVALID_ARGUMENT
    assert _status(lambda: op.setReactionRates(rates(3, n))) == capi.ERR_INVALID_ARGUMENT      # component 3 needs four
    op.setReactionRates(rates(4, n))
    op.setReactionRates(rates(5, n))
    op.setReactionRates(None)
    op.close()
    plain = _create(c, c.physics)  # no external reaction: NULL is accepted, an array is not
    plain.setReactionRates(None)
    assert _status(lambda: plain.setReactionRates(rates(4, n))) == capi.ERR_INVALID_ARGUMENT
    plain.close()


def test_visualization_fields_refuse_external_reactions():
    c = _case()
    op = _create(c, eu.externalize(c.physics, {1: 0}))
    x = _state(c, op)
    assert _status(lambda: op.visualizationFields(x)) == capi.ERR_UNSUPPORTED
    op.close()
    plain = _create(c, c.physics)
    assert len(plain.visualizationFields(x)) > 0  # the same mixture without external reactions is served
    plain.close()


def test_boltzmann_fields_statuses():
    import torch

    c = _case()
    op = _create(c, c.physics)
    x = _state(c, op)
    assert _status(lambda: op.boltzmannFields(x, 0)) == capi.ERR_INVALID_ARGUMENT
    assert _status(lambda: op.boltzmannFields(x, 4)) == capi.ERR_INVALID_ARGUMENT
    assert op.boltzmannFields(x, 3).shape == (5, op.NDofs)
    op.close()
    d = cases.dry_air_axisym(2, 3, 1)
    dry = _create(d, d.physics)
    xd = torch.tensor(np.ascontiguousarray(d.state()).ravel(), dtype=torch.float64, device=dry.device)
    assert _status(lambda: dry.boltzmannFields(xd, 1)) == capi.ERR_UNSUPPORTED
    dry.close()
