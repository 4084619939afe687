"""TraceChain, steps_per_graph and ScopeExit of tps_amd/csrc/trace_chain.hpp -- the host state of the device time loop that
can go stale without producing a NaN -- in a stand-alone program (tests/trace_chain_main.cpp, its own main) that includes
the header alone and is built with plain g++.  For every combination of fusing on / off, eligible / ineligible kernel and
single rank / partitioned mesh the program makes the calls of a driver's time loop and prints what every Mult is told; this
file recomputes every line from the rules:

    mult(stage):  reuse  = eligible and valid and (stage >= 2 or (stage == 1 and chained)):  read the buffer handed over,
                           no k_traces sweep;  otherwise sweep into buffer 0
                  valid  = False
                  write  = eligible and fusing and not gradients_only and single rank and stage >= 1 and (stage <= 3 or
                           chained):  k_flux writes the other buffer, valid = True
    begin / end of a step:      valid = False unless chained
    begin / end of an advance:  valid = False;  chained = (RK4 without forcing) / False
    a failed launch:            valid = False, the stage's RkDev is gone (ScopeExit)
    steps_per_graph:            2 with non-reflecting faces and an odd number of Mults per step, else 1

and then checks the six properties the time loop relies on from the program's own lines, whatever the model says.  The
second case builds the same program with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process;
nothing is loaded into Python."""
import itertools
import os
import subprocess

import pytest

from test_locate_sanitize import FLAGS as SANITIZE_FLAGS, _sanitizer_runtime_missing

HERE = os.path.dirname(os.path.abspath(__file__))
INTEGRATORS = (1, 2, 3, 4)  # tpsrhs_integrator: forward Euler, RK2, RK3-SSP, RK4 -- the stage count of each
CASES = list(itertools.product((0, 1), (0, 1), (0, 1)))  # fuse, eligible, partitioned


def _build(tmp_path, flags, name):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", os.path.join(HERE, "trace_chain_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    return exe


class _Model:
    def __init__(self, fuse, eligible, partitioned, lines):
        self.fuse, self.eligible, self.partitioned, self.lines = fuse, eligible, partitioned, lines
        self.valid = self.chained = False
        self.next = 0

    def mult(self, stage=0, gradients_only=False):
        read, have, write = 0, 0, -1
        if self.eligible and self.valid and (stage >= 2 or (stage == 1 and self.chained)):
            read, have = self.next, 1
        self.valid = False
        if self.eligible and self.fuse and not gradients_only and not self.partitioned and stage >= 1 and (stage <= 3 or self.chained):
            write = self.next = 1 - read
            self.valid = True
        self.lines.append(f"mult stage {stage} gradients_only {int(gradients_only)} read {read} have_traces {have} write {write} "
                          f"valid {int(self.valid)}")

    def step_edge(self):
        if not self.chained:
            self.valid = False

    def rk4_step(self, between=0):
        self.step_edge()
        for stage in (1, 2, 3, 4):
            if stage == 3 and between == 1:
                self.mult()
            if stage == 3 and between == 2:
                self.mult(gradients_only=True)
            self.mult(stage)
            if stage == 3 and between == 3:  # that launch failed: abandoned, and taken again
                self.valid = False
                self.lines.append("failed valid 0 rk_mode 0")
                self.mult(stage)
        self.step_edge()

    def plain_step(self, mults):
        self.step_edge()
        for _ in range(mults):
            self.mult()
        self.step_edge()

    def advance(self, chained):
        self.valid, self.chained = False, chained

    def state(self, what):
        self.lines.append(f"{what} valid {int(self.valid)} chained {int(self.chained)}")


def _expected():
    lines = []
    for fuse, eligible, partitioned in CASES:
        lines.append(f"case fuse {fuse} eligible {eligible} partitioned {partitioned}")
        m = _Model(fuse, eligible, partitioned, lines)
        lines.append("lone_rk4")
        m.rk4_step()
        m.state("end")
        lines.append("advance_rk4")
        m.advance(True)
        for _ in range(3):
            m.rk4_step()
        m.state("inside")
        m.advance(False)
        m.state("end")
        for between in (1, 2, 3):
            lines.append(f"interrupted {between}")
            m.rk4_step(between)
            m.state("end")
        lines.append("advance_interrupted")
        m.advance(True)
        m.rk4_step()
        m.mult(1)
        m.advance(False)
        m.state("failed")
        m.rk4_step()
        m.state("end")
        for integrator in INTEGRATORS:
            lines.append(f"advance_plain {integrator}")
            m.advance(False)
            for _ in range(2):
                m.plain_step(integrator)
            m.state("inside")
            m.advance(False)
        m.state("end")
    for integrator in INTEGRATORS:
        for nr in (0, 1):
            lines.append(f"steps_per_graph integrator {integrator} nr_faces {nr} mults {integrator} "
                         f"steps {2 if nr and integrator % 2 else 1}")
    lines += ["step_key same 1 other_integrator 0", "TRACE_CHAIN DONE"]
    return lines


def _sections(got):
    """{(fuse, eligible, partitioned): {section name: [its lines as dicts, in order]}} of the program's output"""
    out, case, sec = {}, None, None
    for line in got:
        f = line.split()
        if f[0] == "case":
            case = out.setdefault((int(f[2]), int(f[4]), int(f[6])), {})
        elif len(f) <= 2 and f[0] not in ("TRACE_CHAIN",):
            sec = case.setdefault(line, [])
        elif f[0] in ("mult", "end", "inside", "failed") and case is not None:
            d = {k: int(v) for k, v in zip(f[1::2], f[2::2])}
            d["kind"] = f[0]
            sec.append(d)
    return out


def _check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got, want = r.stdout.splitlines(), _expected()
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {k + 1}: got {g!r}, expected {w!r}"
    assert len(got) == len(want)
    # ... and the properties the time loop relies on, read from the program's own lines
    for (fuse, eligible, partitioned), sec in _sections(got).items():
        fusing = bool(fuse and eligible and not partitioned)
        mults = lambda name: [d for d in sec[name] if d["kind"] == "mult"]
        # 1. a lone RK4 step sweeps its own traces at stage 1, reuses them at stages 2-4 and leaves nothing valid
        lone = mults("lone_rk4")
        assert [d["stage"] for d in lone] == [1, 2, 3, 4]
        assert [d["have_traces"] for d in lone] == [0] + [int(fusing)] * 3
        assert lone[3]["write"] == -1 and sec["lone_rk4"][-1] == dict(kind="end", valid=0, chained=0)
        # 2. inside an advance every step after the first reuses stage 4's traces; every step starts by reading buffer 0 and
        #    ends by writing buffer 0: four swaps
        adv = mults("advance_rk4")
        assert len(adv) == 12
        for s in range(3):
            step = adv[4 * s:4 * s + 4]
            assert step[0]["have_traces"] == int(fusing and s > 0) and step[0]["read"] == 0
            assert [d["write"] for d in step] == ([1, 0, 1, 0] if fusing else [-1] * 4)
            assert all(b["read"] == a["write"] for a, b in zip(step, step[1:])) or not fusing
        assert sec["advance_rk4"][-2] == dict(kind="inside", valid=int(fusing), chained=1)
        assert sec["advance_rk4"][-1] == dict(kind="end", valid=0, chained=0)
        # 3. a plain Mult, gradients only or a failed launch between two stages: the next Mult sweeps (into buffer 0)
        for between in (1, 2, 3):
            rows = sec[f"interrupted {between}"]
            k = next(i for i, d in enumerate(rows) if d["kind"] == "failed" or (d["kind"] == "mult" and d["stage"] == 0))
            assert rows[k - 1]["valid"] == int(fusing)  # (stage 2, or the failed stage 3, had promised a hand-over)
            after = rows[k + 1]
            assert after["kind"] == "mult" and after["stage"] == 3 and after["have_traces"] == 0 and after["read"] == 0
            assert rows[k]["valid"] == 0 and rows[k].get("write", -1) == -1
            assert rows[-2]["have_traces"] == int(fusing)  # stage 4 reuses what the repeated stage 3 left
        rows = sec["advance_interrupted"]
        k = next(i for i, d in enumerate(rows) if d["kind"] == "failed")
        assert rows[k] == dict(kind="failed", valid=0, chained=0) and rows[k - 1]["valid"] == int(fusing)
        assert rows[k + 1]["stage"] == 1 and rows[k + 1]["have_traces"] == 0
        # 4. the Euler / RK2 / RK3 sequences (and RK4 with forcing terms) never reuse or write a hand-over
        for integrator in INTEGRATORS:
            plain = mults(f"advance_plain {integrator}")
            assert len(plain) == 2 * integrator
            assert all(d["have_traces"] == 0 and d["write"] == -1 and d["read"] == 0 and d["valid"] == 0 for d in plain)
        # 5. with fusing off, an ineligible kernel or a partitioned mesh every Mult sweeps
        if not fusing:
            every = [d for rows in sec.values() for d in rows if d["kind"] == "mult"]
            assert len(every) > 50 and all(d["have_traces"] == 0 and d["write"] == -1 and d["read"] == 0 for d in every)
    # 6. two steps per graph exactly for (non-reflecting faces, odd Mults per step), for all four schemes
    spg = [dict(zip(l.split()[1::2], map(int, l.split()[2::2]))) for l in got if l.startswith("steps_per_graph")]
    assert [(d["integrator"], d["nr_faces"]) for d in spg] == list(itertools.product(INTEGRATORS, (0, 1)))
    assert all(d["steps"] == (2 if d["nr_faces"] and d["mults"] % 2 else 1) for d in spg)
    assert [d["mults"] for d in spg[::2]] == [1, 2, 3, 4]


def test_trace_chain_follows_its_rules(tmp_path):
    _check(_build(tmp_path, ["-std=c++17", "-O2"], "trace_chain"))


def test_trace_chain_is_clean_under_asan_and_ubsan(tmp_path):
    if _sanitizer_runtime_missing(tmp_path):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    _check(_build(tmp_path, SANITIZE_FLAGS, "trace_chain_sanitize"))
