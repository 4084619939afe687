"""Shared by the tests of the reactions with an external rate coefficient (model = bte, capi.GRIDFUNCTION_RXN).

The oracle has no such reaction and needs none: an external reaction whose rate array holds the closed-form coefficient
must give the oracle's residual of the closed-form reaction.  `externalize` turns Arrhenius reactions of a physics block
into external ones; `arrhenius_rates` computes, on the host in numpy, what their array must hold:

    k_f(node) = A T^b exp(-E / (R T)),  T = max(T_e if the electron is a reactant else T_h, minimum_temperature)

with the node temperatures from tpsrhs_eval_pointwise(TPSRHS_POINT_PRIMITIVES) of the same state."""
import ctypes as C

import numpy as np

from tps_amd import capi


def avogadro_of_the_code():
    """kAvogadro as tps_amd/csrc/physics_plasma.hpp spells it (the reference's AVOGADRONUMBER)"""
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tps_amd", "csrc", "physics_plasma.hpp")
    with open(src) as f:
        m = re.search(r"constexpr double kAvogadro = ([0-9.eE+-]+);", f.read())
    return float(m.group(1))


def copy_physics(ph):
    """a Physics block of its own with the same contents; keeps `ph` (and the tables it points to) alive"""
    new = capi.Physics.from_buffer_copy(ph)
    new._keep = (ph, getattr(ph, "_keep", None))
    return new


def externalize(ph, components):
    """`ph` with the reactions {r: component} made external: model 3, the component in rate_params[0 + r * MAXCHEMPARAMS]"""
    new = copy_physics(ph)
    ch = new.chemistry
    for r, comp in components.items():
        assert 0 <= r < ch.num_reactions
        ch.reaction_models[r] = capi.GRIDFUNCTION_RXN
        ch.rate_params[0 + r * capi.MAXCHEMPARAMS] = float(comp)
        ch.rate_params[1 + r * capi.MAXCHEMPARAMS] = 0.0
        ch.rate_params[2 + r * capi.MAXCHEMPARAMS] = 0.0
    return new


def without_reactions(ph, gone):
    """`ph` with the reactions `gone` deleted from the list, the others in their order"""
    new = copy_physics(ph)
    src, ch = ph.chemistry, new.chemistry
    nsp = ph.mixture.num_species
    keep = [r for r in range(src.num_reactions) if r not in gone]
    ch.num_reactions = len(keep)
    for q, r in enumerate(keep):
        ch.reaction_energies[q] = src.reaction_energies[r]
        ch.detailed_balance[q] = src.detailed_balance[r]
        ch.reaction_models[q] = src.reaction_models[r]
        ch.rate_tables[q] = src.rate_tables[r]
        for k in range(capi.MAXCHEMPARAMS):
            ch.rate_params[k + q * capi.MAXCHEMPARAMS] = src.rate_params[k + r * capi.MAXCHEMPARAMS]
            ch.equilibrium_constant_params[k + q * capi.MAXCHEMPARAMS] = src.equilibrium_constant_params[k + r * capi.MAXCHEMPARAMS]
        for sp in range(nsp):
            ch.reactant_stoich[sp + q * nsp] = src.reactant_stoich[sp + r * nsp]
            ch.product_stoich[sp + q * nsp] = src.product_stoich[sp + r * nsp]
    return new


def primitives(op, x):
    """[neq, n] primitives of the device state x (tpsrhs_eval_pointwise, quantity 0)"""
    import torch

    n = op.NDofs
    out = torch.empty(op.num_equation * n, dtype=torch.float64, device=op.device)
    st = capi.load().tpsrhs_eval_pointwise(op._h, 0, n, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))
    assert st == 0
    return out.cpu().numpy().reshape(op.num_equation, n)


def arrhenius_rates(ph_closed, components, prim, nvel, num_components, fill=0.0):
    """[num_components, n]: row `component` holds the Arrhenius coefficient of reaction r of `ph_closed` (the physics with
    every reaction in its closed form) for {r: component}; the other rows hold `fill`"""
    ch, mx = ph_closed.chemistry, ph_closed.mixture
    nsp = mx.num_species
    Th = prim[nvel + 1]
    Te = prim[-1] if mx.two_temperature else Th
    rates = np.full((num_components, prim.shape[1]), fill, dtype=np.float64)
    for r, comp in components.items():
        assert ch.reaction_models[r] == capi.ARRHENIUS
        A, b, E = (ch.rate_params[k + r * capi.MAXCHEMPARAMS] for k in range(3))
        electron = ch.reactant_stoich[ch.electron_index + r * nsp] != 0
        T = np.maximum(Te if electron else Th, ch.minimum_temperature)
        rates[comp] = A * T ** b * np.exp(-E / (capi.UNIVERSALGASCONSTANT * T))
    return rates


def device_mult(c, physics, U, rates_of=None):
    """one Mult of an operator of `physics` on the case's mesh; rates_of(op, primitives) -> the [ncomp, n] array to set first (or
    None: no array).  -> (y [neq, n], primitives [neq, n] of U)"""
    import torch
    from tps_amd.rhs_operator import RHSoperator

    op = RHSoperator(c.mesh, c.disc, physics, c.bcs)
    x = torch.tensor(np.ascontiguousarray(U).ravel(), dtype=torch.float64, device=op.device)
    y = torch.empty_like(x)
    prim = primitives(op, x)
    if rates_of is not None:
        rates = rates_of(op, prim)
        if rates is not None:
            op.setReactionRates(torch.tensor(rates, dtype=torch.float64, device=op.device))
    op.Mult(x, y)
    torch.cuda.synchronize()
    out = y.cpu().numpy().reshape(U.shape)
    op.close()
    return out, prim
