"""Every refusal of tpsrhs_limit / tpsrhs_limiter_configure (include/tpsrhs.h), with its status and message, and the rows a
valid limiter resolves to: plan_limiter of tps_amd/csrc/limiter.hpp through status.hpp's `guarded`, in a small host program
(tests/limiter_plan_main.cpp) -- the refusals come before any device work, so no device is needed to see them."""
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OK, INVALID, UNSUPPORTED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def _cases():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "limiter_plan")
        b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "limiter_plan_main.cpp"),
                            "-o", exe], capture_output=True, text=True)
        assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "LIMITER PLAN DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        if "|" in line:
            name, status, rows, covers, msg = line.split("|", 4)
            out[name] = (int(status), [int(x) for x in rows.split(",")] if rows else [], int(covers), msg)
    return out


def _refused(name, status, *fragments):
    st, rows, _, msg = _cases()[name]
    assert st == status, (name, st, msg)
    for f in fragments:
        assert f in msg, (name, msg)


def test_valid_limiters_resolve_their_rows():
    c = _cases()
    assert c["ok_rows"][:3] == (OK, [0, 3], 0)
    assert c["ok_pressure"][:3] == (OK, [0], 0)
    # num_rows = -1 without species rows: a valid, empty limiter
    assert c["default_dry_air_is_empty"][:3] == (OK, [], 0)
    assert c["default_table_gas_is_empty"][:3] == (OK, [], 0)
    # ... and with them exactly [sp_first, sp_last): the limiter takes the clamp's place
    assert c["default_ternary"][:3] == (OK, [4], 1)
    assert c["default_six_species"][:3] == (OK, [4, 5, 6, 7, 8], 1)  # row 9, the electron energy, is not listed
    assert c["no_species_row_in_the_loop"][:3] == (OK, [0], 0)        # the clamp stays
    assert c["some_species_rows_in_one_application"][:3] == (OK, [4, 6], 0)


def test_rows_outside_the_state_or_listed_twice_are_invalid():
    _refused("row_negative", INVALID, "tpsrhs_limit", "row -1", "outside")
    _refused("row_too_large", INVALID, "row 4", "outside")
    _refused("row_twice", INVALID, "row 1", "twice")


def test_num_rows_out_of_range_is_invalid():
    _refused("num_rows_below_minus_one", INVALID, "num_rows")
    _refused("num_rows_above_neq", INVALID, "num_rows")


def test_nan_floors_and_bad_pressure_floors_are_invalid():
    _refused("floor_nan", INVALID, "floor of row 0", "NaN")
    _refused("pressure_floor_negative", INVALID, "pressure_floor")
    _refused("pressure_floor_nan", INVALID, "pressure_floor")
    _refused("pressure_without_row_0", INVALID, "row 0", "floor > 0")
    _refused("pressure_with_row_0_at_floor_0", INVALID, "row 0", "floor > 0")


def test_pressure_floor_is_unsupported_off_dry_air():
    _refused("pressure_on_a_mixture", UNSUPPORTED, "pressure_floor", "dry air")
    _refused("pressure_on_the_table_gas", UNSUPPORTED, "pressure_floor", "dry air")


def test_the_loop_refuses_a_part_of_the_species_rows():
    _refused("some_species_rows_in_the_loop", INVALID, "tpsrhs_limiter_configure", "2 of the 5 species rows")
