"""plan_operator of tps_amd/csrc/operator_plan.hpp -- everything tpsrhs_create decides before it touches a device or the mesh
connectivity -- and the host geometry of element_geometry.hpp, in a stand-alone program (tests/operator_plan_main.cpp, its
own main) that includes the two headers alone and is built with plain g++.  The program walks a table of configurations and
prints the plan or the refusal of each; the expected lines below are written out by hand from the rules of include/tpsrhs.h
and the messages of the library:

    nvel = 3 for the axisymmetric formulation, else dim;  neq = nvel + 2 for dry air and the table gas
    mixtures: neq = nvel + 2 + (species - 2 if ambipolar else species - 1) + (1 if two temperatures)
    sp: the species rows [first, last) of the state that the time loop clamps at zero (Check_Undershoot): they follow the
        nvel + 2 flow rows, species - 2 of them if ambipolar else species - 1; empty (first = last) for dry air and the table gas
    kernel family of a mixture: plasma_<3d | 2d | axi>_n<species>[a if ambipolar][_hi for orders 4 and 5 of the Gauss-Legendre pair]
    heavy2d: the 2-D kernels of mixtures and of the axisymmetric formulation;  les: dry air with a model or a sponge
    sponge plane: normal / |normal| over the first dim components, the others 0; width = ratio = 1 without a sponge
    sgs_const: the caller's, or 0.12 (Smagorinsky) / 0.135 (sigma)

Every refusal has accepted neighbours in the table, so none of them is vacuous.  element_sizes is checked on an axis-aligned
box (the smallest edge), inverse_mass_matrices by M M^-1 = I with a mass matrix the program integrates itself on a warped
element.  The second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child
process; nothing is loaded into Python."""
import os
import subprocess

import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))

U, I = "unsupported", "invalid"
PAIRS = "basisType / integrationRule: built pairs are (0, 0) Gauss-Legendre and (1, 1) Gauss-Lobatto"
GLL = "the Gauss-Lobatto pair is built for the planar 2-D and the 3-D formulation"
LTE = "WorkingFluid::LTE_FLUID (one-dimensional tables): built for the axisymmetric formulation, Gauss-Legendre pair"
ROE = "flow/useRoe: Eval_Roe of the reference is 2-D, single-species, not axisymmetric (src/riemann_solver.cpp:117-206)"
NR = ("non-reflecting inlet/outlet types: perfect gas (dry air), not axisymmetric -- the reference's characteristic algebra "
      "(src/outletBC.cpp:573-1027)")
SCOPE = "boundary condition type outside the hot-path scope (attribute %d)"
SPECIES = "USER_DEFINED fluids: 3 to 8 species (electron, background and 1 to 6 others)"
SGS_DRY = "sub-grid scale models: built for dry air in 3-D"
LES = "sub-grid scale model / viscous sponge: built for dry air, planar 2-D and 3-D, Gauss-Legendre pair, reflecting boundary types"
SPONGE_MIX = "viscous sponge for mixtures: built for the planar 2-D and the axisymmetric formulation, Gauss-Legendre pair"
WIDTH, NORMAL = "visc_sponge.width must be positive", "visc_sponge.normal is zero"
ORDER = "polynomial order %d is not built (1..5)"
P2 = (0.25, -0.5, 0.0)  # the sponge point of the program, first two components (2-D)

# name -> (class, message) of a refusal, or the plan's fields that differ from a plain dry-air plan of that dim and order
# (nc 0, nvel = dim, neq = dim + 2, sp = (nvel + 2, nvel + 2), every flag 0, no sponge: n = p = 0, width = ratio = 1, sgs_const 0, transport 0, no unit)
ROWS = [
    ("dry3d_gl", dict(dim=3, order=2)),
    ("dry2d_gl", dict(dim=2, order=5)),
    ("dry3d_gll", dict(dim=3, order=3, nc=1)),
    ("dry2d_gll", dict(dim=2, order=1, nc=1)),
    ("basis_gl_rule_gll", (U, PAIRS)),
    ("basis_gll_rule_gl", (U, PAIRS)),
    ("dry_axi", dict(dim=2, order=2, nvel=3, neq=5, heavy2d=1)),
    ("gll_axi", (U, GLL)),
    ("axi_on_3d_mesh", (I, "the axisymmetric formulation needs a 2-D mesh")),
    ("unknown_fluid", (I, "unknown working_fluid")),
    ("lte_axi", dict(dim=2, order=2, nvel=3, neq=5, heavy2d=1, lte=1)),
    ("lte_planar", (U, LTE)),
    ("lte_3d", (U, LTE)),
    ("roe_2d", dict(dim=2, order=2)),
    ("roe_3d", (U, ROE)),
    ("roe_axi", (U, ROE)),
    ("roe_mixture", (U, ROE)),
    ("ns_passive", (U, "NS_PASSIVE is out of scope")),
    ("order_0", (U, ORDER % 0)),
    ("order_1", dict(dim=3, order=1)),
    ("order_5", dict(dim=3, order=5)),
    ("order_6", (U, ORDER % 6)),
    ("order_6_mixture", (U, ORDER % 6)),
    ("dry_16_bcs", dict(dim=3, order=2)),
    ("dry_17_bcs", (U, "too many boundary conditions")),
    ("mixture_8_bcs", dict(dim=3, order=2, plasma=1, neq=6, sp=(5, 6), transport=1, unit="plasma_3d_n3a")),
    ("mixture_9_bcs", (U, "too many boundary conditions")),
    ("reflecting_set", dict(dim=3, order=2)),
    ("nr_outlet", dict(dim=3, order=2, any_nr=1)),
    ("nr_inlet_2d", dict(dim=2, order=2, any_nr=1)),
    ("nr_outlet_mixture", (U, NR)),
    ("nr_outlet_axi", (U, NR)),
    ("nr_outlet_lte", (U, NR)),
    ("massflow_with_area", dict(dim=3, order=2, any_nr=1)),
    ("massflow_without_area", (I, "mass-flow outlet: data[7] must hold the total patch area")),
    ("face_inlet_3d", dict(dim=3, order=2)),
    ("face_inlet_2d", (U, "face-relative inlets (subsonicFaceBasedX/Y/Z): 3-D (the reference's face frame has three components)")),
    ("uniform_inlet", (U, SCOPE % 5)),
    ("general_wall_dry_air", (U, SCOPE % 3)),
]


def _general_wall_rows():
    """WallData of a viscous_general wall (include/tpsrhs.h, src/M2ulPhyS.cpp:3515-3582): the heavy species are isothermal (1)
    or adiabatic (0); the electrons of a two-temperature plasma take either or the sheath condition (2), those of a
    single-temperature plasma the sheath condition only; the sheath condition needs an ambipolar plasma.  Planar 2-D ternary
    mixture, constant transport (index 0)."""
    rows = []
    for two_t in (0, 1):
        for ambi in (0, 1):
            for hc in (0, 1, 2, 3):
                for ec in (0, 1, 2, 3):
                    name = f"general_wall_t{two_t}_a{ambi}_h{hc}_e{ec}"
                    if hc not in (0, 1):
                        want = (I, "viscous_general wall: heavy thermal condition must be isothermal or adiabatic")
                    elif (ec not in (0, 1, 2)) if two_t else (ec != 2):
                        want = (I, "viscous_general wall: electron thermal condition not understood "
                                   "(single-temperature plasmas accept the sheath condition only)")
                    elif ec == 2 and not ambi:
                        want = (I, "viscous_general wall: plasma must be ambipolar for the sheath condition")
                    else:
                        want = dict(dim=2, order=2, plasma=1, heavy2d=1, neq=2 + 2 + (1 if ambi else 2) + two_t,
                                    sp=(4, 5 if ambi else 6),
                                    unit="plasma_2d_n3a" if ambi else "plasma_2d_n3")
                    rows.append((name, want))
    return rows


ROWS += _general_wall_rows()
ROWS += [
    ("ternary_3d_p3", dict(dim=3, order=3, plasma=1, neq=6, sp=(5, 6), transport=1, unit="plasma_3d_n3a")),
    ("ternary_3d_p4", dict(dim=3, order=4, plasma=1, neq=6, sp=(5, 6), transport=1, unit="plasma_3d_n3a_hi")),
    ("ternary_3d_gll_p3", dict(dim=3, order=3, nc=1, plasma=1, neq=6, sp=(5, 6), transport=1, unit="plasma_3d_n3a")),
    ("ternary_2d_not_ambipolar_2t", dict(dim=2, order=2, plasma=1, heavy2d=1, neq=7, sp=(4, 6), unit="plasma_2d_n3")),
    ("seven_axi_p3", dict(dim=2, order=3, nvel=3, plasma=1, heavy2d=1, neq=11, sp=(5, 10), transport=2, unit="plasma_axi_n7a")),
    ("seven_axi_p4", dict(dim=2, order=4, nvel=3, plasma=1, heavy2d=1, neq=11, sp=(5, 10), transport=2, unit="plasma_axi_n7a_hi")),
    ("seven_3d_not_ambipolar_p5", dict(dim=3, order=5, plasma=1, neq=11, sp=(5, 11), transport=2, unit="plasma_3d_n7_hi")),
    ("eight_constant", dict(dim=3, order=2, plasma=1, neq=11, sp=(5, 11), unit="plasma_3d_n8a")),
    ("eight_argon_mixture", (U, "argon_mixture transport supports at most 7 species (Ar, Ar.+1, Ar_m, Ar_r, Ar_p, Ar_h, E)")),
    ("four_argon_minimal", (U, "argon_minimal transport is the ternary (Ar, Ar.+1, E) model")),
    ("four_argon_mixture", dict(dim=2, order=1, plasma=1, heavy2d=1, neq=6, sp=(4, 6), transport=2, unit="plasma_2d_n4a")),
    ("two_species", (U, SPECIES)),
    ("nine_species", (U, SPECIES)),
    ("lte_transport_for_a_mixture", (U, "transport model outside the built scope (constant, argon_minimal, argon_mixture)")),
    ("no_electrons", (U, "USER_DEFINED fluids without electrons are not built")),
    ("smagorinsky_3d", dict(dim=3, order=2, les=1, sgs_const=0.12)),
    ("sigma_3d", dict(dim=3, order=2, les=1, sgs_const=0.135)),
    ("sigma_3d_own_constant", dict(dim=3, order=2, les=1, sgs_const=0.2)),
    ("smagorinsky_2d", (U, "sub-grid scale models need dim == 3 (the reference's strain tensor indexes three directions)")),
    ("smagorinsky_gll", (U, LES)),
    ("smagorinsky_nr_outlet", (U, LES)),
    ("unknown_sgs_model", (I, "unknown sgs.model_type")),
    ("smagorinsky_mixture", (U, SGS_DRY)),
    ("smagorinsky_axi", (U, SGS_DRY)),
    ("smagorinsky_lte", (U, SGS_DRY)),
    ("sponge_dry_2d", dict(dim=2, order=2, les=1, sponge=1, n=(3.0 / 5.0, 4.0 / 5.0, 0.0), p=P2, width=0.3, ratio=25.0)),
    ("sponge_dry_3d_sigma", dict(dim=3, order=2, les=1, sponge=1, n=(1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0), p=(0.25, -0.5, 2.0), width=1.5,
                                 ratio=8.0, sgs_const=0.135)),
    ("sponge_dry_zero_width", (I, WIDTH)),
    ("sponge_dry_2d_normal_in_z_only", (I, NORMAL)),
    ("sponge_mixture_2d", dict(dim=2, order=2, plasma=1, heavy2d=1, neq=5, sp=(4, 5), transport=1, unit="plasma_2d_n3a", sponge=1,
                               n=(0.0, 1.0, 0.0), p=P2, width=0.2, ratio=11.0)),
    ("sponge_dry_axi", dict(dim=2, order=2, nvel=3, neq=5, heavy2d=1, sponge=1, n=(4.0 / 5.0, 3.0 / 5.0, 0.0), p=P2, width=0.5, ratio=2.0)),
    ("sponge_lte", dict(dim=2, order=2, nvel=3, neq=5, heavy2d=1, lte=1, sponge=1, n=(1.0, 0.0, 0.0), p=P2, width=0.5, ratio=2.0)),
    ("sponge_mixture_3d", (U, SPONGE_MIX)),
    ("sponge_mixture_2d_negative_width", (I, WIDTH)),
    ("sponge_mixture_2d_zero_normal", (I, NORMAL)),
    ("lte_log_scale", (I, "lte tables: linear scales only (x_log_scale = f_log_scale = 0)")),
    ("lte_energy_not_increasing", (I, "lte.energy_table: e(T) must increase (the inverse table T(e) is its transpose)")),
]


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(HERE, "operator_plan_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _plan_fields(line):
    f = line.split()
    assert f[0] == "plan", line
    v, k = {}, 1
    while k < len(f):
        width = 3 if f[k] in ("n", "p") else (2 if f[k] == "sp" else 1)
        v[f[k]] = tuple(f[k + 1:k + 1 + width]) if width > 1 else f[k + 1]
        k += 1 + width
    return v


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(ROWS) + 7 and got[-1] == "OPERATOR_PLAN DONE"
    refused = accepted = 0
    for line, (name, want) in zip(got, ROWS):
        head, _, rest = line.partition(": ")
        assert head == name, line
        if isinstance(want, tuple):
            assert rest == f"{want[0]} {want[1]}", line
            refused += 1
            continue
        accepted += 1
        v = _plan_fields(rest)
        dim = want["dim"]
        rows = want.get("nvel", dim) + 2
        assert ("sp" in want) == bool(want.get("plasma")), name  # every mixture's species rows are written out above
        full = dict(nc=0, nvel=dim, neq=rows, sp=(rows, rows), plasma=0, lte=0, heavy2d=0, les=0, any_nr=0, sponge=0,
                    n=(0.0, 0.0, 0.0), p=(0.0, 0.0, 0.0), width=1.0, ratio=1.0, sgs_const=0.0, transport=0, unit="-")
        full.update(want)
        assert set(v) == set(full), line
        for key, w in full.items():
            if isinstance(w, tuple):
                assert tuple(float(x) for x in v[key]) == w, (line, key)
            elif isinstance(w, float):
                assert float(v[key]) == w, (line, key)
            else:
                assert v[key] == str(w), (line, key)
    assert refused > 40 and accepted > 40
    # an axis-aligned box: the smallest singular value of the Jacobian is the smallest edge (0.5 x 0.2 x 0.3, 0.7 x 0.4)
    for line, name, edge in ((got[-7], "hex", 0.2), (got[-6], "quad", 0.4)):
        f = line.split()
        assert f[:2] == ["element_size", name] and abs(float(f[2]) - edge) <= 1e-14 * edge, line
    cases = []
    for line in got[-5:-1]:
        f = line.split()
        assert f[0] == "mass_inverse_defect" and float(f[5]) < 1e-12, line
        cases.append((int(f[2]), int(f[4])))
    assert cases == [(2, 1), (2, 2), (3, 1), (3, 2)]


def test_plan_and_element_geometry_follow_their_rules(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "operator_plan"))


def test_plan_and_element_geometry_are_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "operator_plan_sanitize"))
