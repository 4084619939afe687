"""StepCadence and RecordIndex of tps_amd/csrc/record_log.hpp -- the bookkeeping that the statistics, the probes and the
monitor of the device time loop share -- in a stand-alone program (tests/record_log_main.cpp, its own main) that includes
the header alone and is built with plain g++.  The program takes 40 steps for every (interval, start, capacity), restarts the
log after step 17 and assigns the step counter after step 29; this file recomputes every line it prints from the rules:

    tick():            count += 1;  due = count % interval == 0 and count >= start
    due_after_next():  the same question of count + 1
    claim(count):      the log is full: ndropped += 1, row -1;  else iters.append(count), row = nrecords, nrecords += 1
    reset():           nrecords = ndropped = 0, iters = [];  count goes on

The second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process;
nothing is loaded into Python."""
import itertools
import os
import subprocess

import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, RESET_AFTER, SET_AFTER, SET_COUNT = 40, 17, 29, 8
CASES = list(itertools.product((1, 2, 3, 5), (0, 4), (1, 3)))  # interval, start, capacity


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "record_log_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


def _expected():
    lines = []
    for interval, start, capacity in CASES:
        lines.append(f"case interval {interval} start {start} capacity {capacity}")
        count = nrecords = ndropped = 0
        iters = []
        summary = lambda what: f"{what} nrecords {nrecords} ndropped {ndropped} iters" + "".join(f" {c}" for c in iters)
        for step in range(1, STEPS + 1):
            due_next = (count + 1) % interval == 0 and count + 1 >= start
            count += 1
            due = count % interval == 0 and count >= start
            row = "."
            if due and nrecords >= capacity:
                ndropped += 1
                row = "-1"
            elif due:
                iters.append(count)
                row = str(nrecords)
                nrecords += 1
            lines.append(f"step {step} count {count} due_next {int(due_next)} tick {int(due)} row {row} "
                         f"nrecords {nrecords} ndropped {ndropped}")
            if step == RESET_AFTER:
                lines.append(summary("reset"))
                nrecords = ndropped = 0
                iters = []
            if step == SET_AFTER:
                count = SET_COUNT
        lines.append(summary("end"))
    lines.append("RECORD_LOG DONE")
    return lines


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), _expected()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {k + 1}: got {g!r}, expected {w!r}"
    assert len(got) == len(want) == len(CASES) * (STEPS + 3) + 1
    # ... and two properties read from the program's own lines, whatever the model above says
    due_since_reset, start, held_back = 0, 0, 0
    for line in got:
        f = line.split()
        if f[0] == "case":
            due_since_reset, start = 0, int(f[4])
        elif f[0] == "step":
            v = dict(zip(f[2::2], f[3::2]))
            assert v["due_next"] == v["tick"], line  # due_after_next() before a step is what tick() says after it
            due_since_reset += int(v["tick"])
            assert int(v["nrecords"]) + int(v["ndropped"]) == due_since_reset, line
            assert (v["row"] == ".") == (v["tick"] == "0"), line
            assert v["tick"] == "0" or int(v["count"]) >= start, line
            held_back += int(v["count"]) < start
            if int(f[1]) == RESET_AFTER:
                due_since_reset = 0
    # the cases are not vacuous: records, drops and a start that holds records back all occur
    assert any(" row 2 " in g for g in got) and any(" row -1 " in g for g in got) and held_back > 0


def test_cadence_and_record_index_follow_their_rules(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "record_log"))


def test_record_log_is_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "record_log_sanitize"))
