"""The oracle's point closures against the REFERENCE's own compiled code (oracle/_ref/libtpsref_point.so, built by
oracle/ref.mk from a checkout of the reference; driver oracle/ref_point.cpp, loader tests/ref_point_lib.py).

Per configuration of tests/host_physics/run_cases.py (and dry air): 96 random admissible states with primitive
gradients and non-unit normals, plus the edge states of ref_point_lib.edge_states; every quantity the driver exposes,
oracle against reference, per output row relative to that row's max norm over the sample.

BOUND = 1e-12 for every quantity: both sides evaluate the same formulas in IEEE double and nothing is differenced.
(Measured: every row of every configuration agrees BIT FOR BIT, profiles/r19_reference_point.txt -- the oracle follows
the reference operation by operation and both are compiled without contraction into FMAs for the baseline x86-64.)
No bound is widened.  One exclusion: with CONSTANT transport the reference's own transport class ends the run (assert) on
the edge state without charged particles, so that state is compared there for everything outside the transport class
only (ref_point_lib.edge_states).

The same library also checks the DEVICE text: test_device_text_against_the_reference builds and runs
tests/reference_point_main.cpp (bound 1e-11), and test_fixtures_regenerate_bit_for_bit keeps the recorded values that
tests/test_gpu_reference_point.py reads on the GPU equal to the live library's.

Not covered here, because no compiled reference code exists for them without the finite-element library: the assembly of
SourceTerm::updateTerms (its pieces ARE covered), the boundary-condition classes (the mixture's state modifiers they are
built from ARE covered), the non-reflecting patches.

`python tests/test_reference_point.py` rewrites profiles/r19_reference_point.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ref_point_lib as R  # noqa: E402
from tps_amd import capi  # noqa: E402

BOUND = 1.0e-12
N_STATES = 96

pytestmark = pytest.mark.skipif(not R.have_reference() and not os.path.exists(R.REF_SO),
                                reason="no checkout of the reference and no built oracle/_ref/libtpsref_point.so")


def test_library_builds_from_the_checkout():
    """with a checkout present the library must build (a failure, not a skip) and must leave no symbol unresolved"""
    L = R.lib()
    for f in ("tpsref_create", "tpsref_prim", "tpsref_flux_transport", "tpsref_source_transport", "tpsref_viscous_flux",
              "tpsref_bdr_viscous_flux", "tpsref_lf", "tpsref_roe", "tpsref_chemistry", "tpsref_energy_sink",
              "tpsref_sheath_bdr_flux", "tpsref_modify_state_from_primitive"):
        assert hasattr(L, f), f


def compare(key, oracle_physics=None, reference_physics=None):
    """-> {quantity: per-row errors} over the random sample, the same over the edge states (which reuse the first
    gradients, normals and positions of the sample; evaluated on their own, so that the Lax-Friedrichs partner of an
    admissible state is an admissible state)"""
    X, U, G, N = R.sample(key, N_STATES)
    parts = [(X, U, G, N, True)]
    if R.is_plasma(key):
        names, E = R.edge_states(key)
        m = len(names)
        keep = np.ones(m, dtype=bool)
        if R.CONFIGS[key]["tr"] == capi.CONSTANT and R.NO_TRANSPORT_EDGE in names:
            keep[names.index(R.NO_TRANSPORT_EDGE)] = False  # the reference's transport ends the run on it: see edge_states
            parts.append((X[:m][~keep], E[~keep], G[:m][~keep], N[:m][~keep], False))
        parts.insert(1, (X[:m][keep], E[keep], G[:m][keep], N[:m][keep], True))
    out = []
    for Xp, Up, Gp, Np, transport in parts:
        Xp, Up, Gp, Np = (np.ascontiguousarray(a) for a in (Xp, Up, Gp, Np))
        ref = R.evaluate_reference(key, Up, Gp, Np, Xp, reference_physics, transport=transport)
        got = R.evaluate_oracle(key, Up, Gp, Np, Xp, ref, oracle_physics)
        assert set(ref) == set(got)
        if not out:  # the random sample is admissible: everything finite there
            assert all(np.all(np.isfinite(v)) for v in ref.values()), key
        out.append({k: R.row_errors(got[k], ref[k]) for k in got})
    edge = dict(out[1]) if len(out) > 1 else {}
    for k, e in (out[2].items() if len(out) > 2 else ()):  # the transport-free state: the worse of the two per row
        edge[k] = np.maximum(edge[k], e)
    return out[0], edge


@pytest.mark.parametrize("key", list(R.CONFIGS))
def test_oracle_matches_reference(key):
    body, edge = compare(key)
    for part, errs in (("sample", body), ("edges", edge)):
        for k, e in errs.items():
            print(f"{key:28s} {part:6s} {k:32s} {e.max():.3e}")
    bad = [(part, k, float(e.max())) for part, errs in (("sample", body), ("edges", edge)) for k, e in errs.items()
           if not e.max() <= BOUND]
    assert not bad, bad


def red(errs):
    return {k for k, e in errs.items() if not e.max() <= BOUND}


# ---- negative controls: each must turn red what one expects and leave the rest green ---------------------------
def test_control_swapped_molar_masses():
    """ion and electron molar masses swapped on the oracle side only.  Every closure that reads a molar mass turns red;
    what is a function of the temperatures and number densities HANDED IN alone stays green: the rate coefficients, the
    equilibrium constants, the progress rates (mass action on the given densities) and the radiation sink."""
    key = "3d_n3_2T_minimal_ke3"
    ph = R.make_physics(key)
    nsp = ph.mixture.num_species
    a, b = 0 + capi.SPECIES_MW * nsp, 1 + capi.SPECIES_MW * nsp
    ph.mixture.gas_params[a], ph.mixture.gas_params[b] = ph.mixture.gas_params[b], ph.mixture.gas_params[a]
    body, _ = compare(key, oracle_physics=ph)
    green = {"forward_rate_coeffs", "equilibrium_constants", "progress_rates", "energy_sink"}
    assert red(body) & green == set(), red(body) & green
    for k in ("prim", "pressure", "number_densities", "species_enthalpies", "max_char_speed", "flux_transport",
              "flux_diffusion_velocity", "convective_flux", "viscous_flux", "lf", "sheath_bdr_flux", "electric_conductivity",
              "mt_frequency", "creation_rates"):
        assert k in red(body), k


def test_control_third_order_electron_conductivity():
    """thirdOrderkElectron on in the reference, off in the oracle.  Red: the electron thermal conductivity (row 3 of the
    flux transport buffer) and the fluxes that conduct electron heat with it -- the interior viscous flux and the boundary
    flux with nothing prescribed, in their two energy rows only.  Green: everything else, among it the boundary flux
    of an adiabatic wall (both heat fluxes prescribed) and of the sheath (electron heat flux prescribed): k_e never
    enters them."""
    key = "3d_n3_2T_minimal_ke3"
    ph = R.make_physics(key)
    ph.gas_transport.third_order_k_electron = 0
    body, _ = compare(key, oracle_physics=ph)
    assert red(body) == {"flux_transport", "viscous_flux", "bdr_viscous_flux_none"}, red(body)
    assert np.all(body["flux_transport"][:3] <= BOUND) and body["flux_transport"][3] > 1e-3
    dim, nvel = R.dims(key)
    neq = len(body["bdr_viscous_flux_none"])
    other_rows = [k for k in range(neq) if k not in (1 + nvel, neq - 1)]
    assert np.all(body["bdr_viscous_flux_none"][other_rows] <= BOUND)
    assert np.all(body["bdr_viscous_flux_none"][[1 + nvel, neq - 1]] > BOUND)


def test_control_detailed_balance():
    """detailed balance of the ionisation off on the oracle side: equilibrium constants, progress and creation rates turn
    red; the forward rate coefficients and everything outside the chemistry stay green"""
    key = "3d_n3_2T_minimal_ke3"
    ph = R.make_physics(key)
    assert ph.chemistry.detailed_balance[0] == 1
    ph.chemistry.detailed_balance[0] = 0
    body, _ = compare(key, oracle_physics=ph)
    assert red(body) == {"equilibrium_constants", "progress_rates", "creation_rates"}, red(body)


@pytest.mark.parametrize("key", list(R.FIXTURE_KEYS))
def test_fixtures_regenerate_bit_for_bit(key):
    """tests/golden/reference_point/<key>.npz (what the GPU leg reads) against the live library: same compiler, same
    flags, so anything but bit equality means the fixture or the recipe drifted (tests/golden/make_reference_point.py)"""
    if not R.have_reference():
        pytest.skip("regeneration needs the checkout the library is built from")
    live, stored = R.fixture_arrays(key), R.load_fixture(key)
    assert set(live) == set(stored)
    assert str(stored["key"]) == key
    assert stored["U"].shape[0] <= 64 and os.path.getsize(R.fixture_path(key)) < 200_000
    for k in live:
        if k != "key":
            assert live[k].shape == stored[k].shape and live[k].tobytes() == stored[k].tobytes(), k


def test_device_text_against_the_reference(tmp_path):
    """tests/reference_point_main.cpp: the product's device headers compiled for the host (plain g++, no sanitizer) and
    linked with libtpsref_point.so, on the states written here; 1e-11 per row, asserted by the program's exit status"""
    R.lib()
    cases_file = str(tmp_path / "device_text_cases.bin")
    R.write_device_cases(cases_file, N_STATES)
    exe = str(tmp_path / "reference_point_main")
    here = os.path.dirname(os.path.abspath(__file__))
    refdir = os.path.dirname(R.REF_SO)
    # the product's headers with ONE line dropped, as tests/host_physics/Makefile does: the empty AMDGPU-only asm of
    # PlasmaPhys::relaunder (a scalar-register constraint no host compiler knows)
    csrc, src = os.path.join(R.ROOT, "tps_amd", "csrc"), tmp_path / "src"
    src.mkdir()
    for name in os.listdir(csrc):
        if name.endswith(".hpp"):
            text = open(os.path.join(csrc, name)).read().splitlines(keepends=True)
            (src / name).write_text("".join(ln for ln in text if 'asm volatile("" : "+s"(lo), "+s"(hi));' not in ln))
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-attributes",
           "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-I" + os.path.join(here, "host_physics"),
           "-I" + str(src), "-I" + os.path.join(R.ROOT, "include"),
           os.path.join(here, "reference_point_main.cpp"), "-o", exe, "-L" + refdir, "-ltpsref_point", "-Wl,-rpath," + refdir]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, cases_file], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert f"{len(R.DEVICE_TEXT_KEYS)} cases, 0 quantities beyond" in r.stdout


def write_profile(path):
    lines = ["# oracle (oracle/_build/libtpsoracle.so) against the reference's compiled point physics (oracle/_ref/libtpsref_point.so)",
             "# max over the rows of a quantity of: max |oracle - reference| over the sample / max |reference| over the sample",
             f"# sample: {N_STATES} random admissible states per configuration; edges: tests/ref_point_lib.py::edge_states",
             f"# bound asserted by tests/test_reference_point.py: {BOUND:g} for every quantity",
             f"{'configuration':28s} {'quantity':32s} {'sample':>10s} {'edges':>10s}"]
    for key in R.CONFIGS:
        body, edge = compare(key)
        for k in body:
            e = f"{edge[k].max():10.3e}" if edge else f"{'-':>10s}"
            lines.append(f"{key:28s} {k:32s} {body[k].max():10.3e} {e}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    write_profile(os.path.join(R.ROOT, "profiles", "r19_reference_point.txt"))
