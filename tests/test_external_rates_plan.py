"""split_chemistry of tps_amd/csrc/plasma_params_host.hpp -- the chemistry of a mixture in two blocks: the reactions with a
closed form for the sweeps, the reactions with an external rate coefficient (TPSRHS_GRIDFUNCTION_RXN, the reference's
model = bte) for a pass of their own -- in a stand-alone program (tests/external_rates_plan_main.cpp, its own main) built
with plain g++.  The expected blocks below are written out by hand from the rules:

    a reaction goes to the external block iff its model is 3; both blocks keep the caller's order
    every field of a reaction travels with it (energy, detailed balance, keq, stoichiometry)
    external: rate[0] = the component (rate_params[0], an integer >= 0, else INVALID_ARGUMENT), the other rate slots 0
    table_share counts in the block's own numbering: the first reaction OF THE BLOCK on the same abscissae
    components_needed = 1 + the largest component; only tabulated reactions place a table
    radiative decay (4) and unknown models: UNSUPPORTED

The second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process;
nothing is loaded into Python."""
import os
import subprocess

import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ION, REC = "0>1 1>2 1>0", "1>0 2>1 0>1"  # the stoichiometry (reactant>product per species) of the program's two reactions
COMPONENT = "grid-function reaction: rate_params[0] must hold the component index (an integer >= 0)"
SCOPE = "reaction model outside the built scope (Arrhenius, Hoffert-Lien, tabulated, grid function)"


def rx(model, p0, energy, keq0, share, stoich, balance=0, table_n=0):
    """one printed reaction; p1 = 1.5 as the program sets it, 0 for an external reaction"""
    return dict(model=model, p0=p0, p1=0.0 if model == 3 else 1.5, energy=energy, balance=balance, keq0=keq0, share=share,
                table_n=table_n, stoich=stoich)


# name -> (sweep block, external block, components_needed, tables_placed) or (class, message) of a refusal.
# keq0 = 10 + the reaction's number in the CALLER's list: it shows where a reaction came from.
EXPECT = {
    "no_external": ([rx(0, 74072, 1, 10, 0, ION), rx(0, 34126, 2, 11, 1, REC)], [], 0, 0),
    "both_external": ([], [rx(3, 0, 1, 10, 0, ION), rx(3, 1, 2, 11, 1, REC)], 2, 0),
    "second_external": ([rx(0, 74072, 1, 10, 0, ION)], [rx(3, 1, 2, 11, 0, REC)], 2, 0),
    "first_external_component_5": ([rx(0, 34126, 2, 11, 0, REC)], [rx(3, 5, 1, 10, 0, ION)], 6, 0),
    "balance_external": ([], [rx(3, 0, 1, 10, 0, ION, balance=1)], 1, 0),
    # caller: 0 external(2) | 1 table A | 2 table B | 3 table A | 4 Arrhenius | 5 external(0) | 6 table B
    "table_moves": ([rx(2, 0, 2, 11, 0, REC, table_n=4), rx(2, 0, 1, 12, 1, ION, table_n=4), rx(2, 0, 2, 13, 0, REC, table_n=4),
                     rx(0, 7, 1, 14, 3, ION), rx(2, 0, 1, 16, 1, ION, table_n=4)],
                    [rx(3, 2, 1, 10, 0, ION), rx(3, 0, 2, 15, 1, REC)], 3, 4),
    "hoffert_lien_stays": ([rx(1, 0.01, 1, 10, 0, ION)], [rx(3, 3, 2, 11, 0, REC)], 4, 0),
    "fractional_component": ("invalid", COMPONENT),
    "negative_component": ("invalid", COMPONENT),
    "nan_component": ("invalid", COMPONENT),
    "radiative_decay": ("unsupported", SCOPE),
    "unknown_model": ("unsupported", SCOPE),
    # TPSRHS_MAXREACTIONS = 34 reactions, tabulated (one grid) and external in turn
    "every_slot": ([rx(2, 0, 2, 10 + 2 * k, 0, REC, table_n=4) for k in range(17)],
                   [rx(3, 1, 1, 11 + 2 * k, k, ION) for k in range(17)], 2, 17),
}


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    cmd = ["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-Wno-attributes", "-Wno-unused-variable",
                             "-Wno-unused-but-set-variable", "-Wno-unused-parameter", "-I" + os.path.join(HERE, "host_physics"),
                             "-I" + os.path.join(ROOT, "tps_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                             os.path.join(HERE, "external_rates_plan_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _parse(lines):
    """{case: refusal tuple or (sweep, external, needed, placed)} of the program's output"""
    out, k = {}, 0
    while k < len(lines) and lines[k] != "EXTERNAL_RATES_PLAN DONE":
        assert lines[k].endswith(":") and not lines[k].startswith(" "), lines[k]
        name = lines[k][:-1]
        k += 1
        first = lines[k].split()
        if first[0] in ("invalid", "unsupported"):
            out[name] = (first[0], lines[k].strip().partition(" ")[2])
            k += 1
            continue
        blocks = []
        for label in ("sweep:", "external:"):
            f = lines[k].split()
            assert f[0] == label and f[1] == "reactions" and f[3:] == ["electron", "1", "min_temperature", "2000"], lines[k]
            n = int(f[2])
            k += 1
            rows = []
            for r in range(n):
                f = lines[k].split()
                assert f[0] == f"{r}:", lines[k]
                v = {f[i]: f[i + 1] for i in range(1, 17, 2)}
                rows.append(dict(model=int(v["model"]), p0=float(v["p0"]), p1=float(v["p1"]), energy=float(v["energy"]),
                                 balance=int(v["balance"]), keq0=float(v["keq0"]), share=int(v["share"]),
                                 table_n=int(v["table_n"]), stoich=" ".join(f[18:])))
                assert f[17] == "stoich"
                k += 1
            blocks.append(rows)
        f = lines[k].split()
        assert f[0] == "components_needed" and f[2] == "tables_placed", lines[k]
        out[name] = (blocks[0], blocks[1], int(f[1]), int(f[3]))
        k += 1
    assert lines[k] == "EXTERNAL_RATES_PLAN DONE" and k == len(lines) - 1
    return out


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = _parse(r.stdout.splitlines())
    assert list(got) == list(EXPECT)
    for name, want in EXPECT.items():
        assert got[name] == want, (name, got[name], want)


def test_chemistry_splits_into_the_two_blocks(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "external_rates_plan"))


def test_the_split_is_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "external_rates_plan_sanitize"))
