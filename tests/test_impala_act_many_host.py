"""Host logic of vectorised impala acting (no GPU): ``idqn_act_host_many_impala`` is declared, bound and (once built) exported;
the case table of tests/impala_act_shapes.py against its coverage conditions -- every branch of the Dense_0 plan hit at both
ends, every row, n, head assignment and parameter set the device test needs; csrc/imp_act_many_args.h through
tools/probes/imp_act_many_args_probe.cpp -- its own checks, the plan against the table's restatement, and its table check
against numpy's grouped order for every case's head list (permuted ones included) and against broken copies of them;
``DeviceAgent._best_actions`` asks the new entry third, for impala agents and the sizes in ``act_many_imp_sizes`` only.
The device is a stub.  On the parent commit the symbol, the args header, the probe and the flag do not exist."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import impala_act_shapes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_act_host_many_impala"
CSRC = os.path.join(ROOT, "i-dqn_amd", "csrc")


def _cxx():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    assert NAME in _hip.SYMBOLS, f"{NAME} is not bound in slimdqn/_hip.py"
    assert _hip.SYMBOLS[NAME] == _hip.SYMBOLS["idqn_act_host_many_fc"]  # its signature and contract
    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), f"{NAME} is not declared in include/idqn_hip.h"
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if os.path.exists(_hip.LIB_PATH):
        nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
        exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                                  capture_output=True, text=True).stdout
        assert re.search(r"\sT\s+" + NAME + r"$", exported, re.M), f"{NAME} is not exported by the library"
        lib = _hip.lib()
        assert getattr(lib, NAME).argtypes == _hip.SYMBOLS[NAME][1]
        assert lib.idqn_abi_version() == 4  # an entry added only


def test_constants_of_the_args_header_are_the_tables_and_the_bindings():
    from slimdqn import _hip

    text = open(os.path.join(CSRC, "imp_act_many_args.h")).read()
    got = {k: int(v) for k, v in re.findall(r"^#define (IMP_ACT_\w+) (\d+)", text, re.M)}
    assert got == {"IMP_ACT_MAX": T.MAX, "IMP_ACT_SC": T.SC, "IMP_ACT_PASS": T.PASS, "IMP_ACT_OC": T.OC, "IMP_ACT_PPW": T.PPW}
    assert (_hip.ACT_MANY_MAX, _hip.IMP_ACT_SC, _hip.IMP_ACT_PASS, _hip.IMP_ACT_OC, _hip.IMP_ACT_PPW) == (T.MAX, T.SC, T.PASS, T.OC, T.PPW)
    kernels = open(os.path.join(CSRC, "impala_kernels.h")).read()
    assert re.search(r"^#define IMP_D0_IC 64\b", kernels, re.M), "a pass of the acting Dense_0 is a pass of k_imp_d0_fwd"


def test_table_meets_its_coverage_conditions():
    assert len(set(T.CASES)) == len(T.CASES)
    for row, n, assign, which in T.CASES:
        obs, feats, A, K, B = T.shape(row)
        h = T.heads(assign, n, K)
        assert 1 <= n <= T.MAX and assign in T.ASSIGNMENTS and which in (0, 1) and len(h) == n and min(h) >= 0 and max(h) < K
        assert len(T.states(row, n)) == n
    by_row = {}
    for row, n, assign, which in T.CASES:
        by_row.setdefault(row, []).append((n, assign, which))
    # the rows the device test must run, at the n the issue names
    need = {"odd_even", "no_hidden", "tile_plus", "tile_minus", "u8_tail", "d0_blocks", "mid", "tie", "one_row", "workload", "reference_test"}
    assert need <= set(by_row)
    assert (3, "rot", 0) in by_row["workload"] and any(n == 2 for n, _, _ in by_row["reference_test"])
    assert {n for n, _, _ in by_row["odd_even"]} >= {1, 2, T.SC, T.SC + 1, 31, 32}
    assert {a for _, _, a, _ in T.CASES} == set(T.ASSIGNMENTS) and {w for _, _, _, w in T.CASES} == {0, 1}
    # shapes: with and without a hidden layer, A above 32, K = 1 and K > 2
    assert any(T.geometry(r)[1] is None for r in by_row) and any(T.geometry(r)[1] is not None for r in by_row)
    assert any(T.shape(r)[2] > 32 for r in by_row) and any(T.shape(r)[3] == 1 for r in by_row) and any(T.shape(r)[3] >= 5 for r in by_row)
    # the Dense_0 plan: every branch at both ends
    plans = {r: T.d0_plan(*T.geometry(r)) for r in by_row if T.geometry(r)[1] is not None}
    lpf = {p["last_pass_features"] for p in plans.values()}
    assert T.PASS in lpf and any(v < T.PASS for v in lpf), "a full and a ragged last pass"
    lrp = {p["last_range_passes"] for p in plans.values()}
    assert 1 in lrp and T.PPW in lrp and any(1 < v < T.PPW for v in lrp), "last range: one pass, all four, in between"
    assert any(p["ranges"] == 1 for p in plans.values()) and any(p["ranges"] > 2 for p in plans.values())
    assert any(p["n_pass"] == 1 for p in plans.values()) and any(p["n_pass"] > 100 for p in plans.values())
    lbu = {(p["col_blocks"], p["last_block_units"]) for p in plans.values()}
    assert (1, T.OC) in lbu and (2, 1) in lbu and any(c == 1 and u < T.OC for c, u in lbu) and any(c > 2 for c, _ in lbu), \
        "exactly one column block, a second block of one unit, a partial single block, many blocks"
    assert plans["workload"] == dict(n_pass=121, ranges=31, col_blocks=8, last_pass_features=64, last_range_passes=1, last_block_units=64,
                                     part_floats=32 * 121 * 512)
    assert plans["workload"]["part_floats"] * 4 < 8 << 20, "under 8 MB at n = 32"
    # groups and register chunks over the cases that have a Dense_0 launch
    groups, last_chunks, n_chunks, permuted, unused = set(), set(), set(), False, False
    for row, n, assign, which in T.CASES:
        if T.geometry(row)[1] is None:
            continue
        K = T.shape(row)[3]
        h = T.heads(assign, n, K)
        ng, order, g_head, g_start, g_count = T.grouped(h, K)
        groups.add((ng, min(n, K)))
        permuted |= order != sorted(order)
        unused |= ng < min(n, K)
        for c in g_count:
            k, last = T.chunks(c)
            n_chunks.add(k)
            last_chunks.add(last)
    assert any(g == 1 for g, _ in groups) and any(g == m and g >= 5 for g, m in groups), "one group, and as many as the grid has"
    assert permuted and unused
    assert {1, 2, 4} <= n_chunks and {1, T.SC} <= last_chunks and any(1 < v < T.SC for v in last_chunks)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("probe") / "imp_act_many_args_probe"
    subprocess.run([cc, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tools", "probes", "imp_act_many_args_probe.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def test_probe_builds_and_reports_no_failures(probe):
    out = subprocess.run([probe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    m = re.search(r"^ok: (\d+) checks, 0 failures$", out.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) > 1000, out.stdout[-500:]


def test_plan_of_the_header_is_the_tables(tmp_path):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    shapes = sorted({T.geometry(r) for r, _, _, _ in T.CASES if T.geometry(r)[1] is not None})
    src = tmp_path / "plan.cpp"
    src.write_text('#include <stdio.h>\n#include "imp_act_many_args.h"\nint main() {\n' + "".join(
        f'  {{ imp_act_many_d0_plan_t p = imp_act_many_d0_plan({F}, {D}); printf("%d %d %d %d %d %d %ld\\n", p.n_pass, p.ranges, p.col_blocks, '
        "p.last_pass_features, p.last_range_passes, p.last_block_units, (long)p.part_floats); }\n" for F, D in shapes) + "  return 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.run([cc, "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(lines) == len(shapes)
    for line, (F, D) in zip(lines, shapes):
        p = T.d0_plan(F, D)
        assert [int(x) for x in line.split()] == [p["n_pass"], p["ranges"], p["col_blocks"], p["last_pass_features"], p["last_range_passes"],
                                                  p["last_block_units"], p["part_floats"]], (F, D)


def _line(n, K, heads, table):
    ng, order, g_head, g_start, g_count = table
    j = lambda v: " ".join(str(int(x)) for x in v)
    return f"{n} {K} | {j(heads)} | {ng} | {j(order)} | {j(g_head)} | {j(g_start)} | {j(g_count)}\n"


def test_table_check_against_numpy_tables_and_broken_copies(probe, tmp_path):
    lines, want = [], []
    rng = np.random.default_rng(5)
    lists = [(T.shape(r)[3], T.heads(a, n, T.shape(r)[3])) for r, n, a, _ in T.CASES]
    lists += [(5, rng.permutation([e % 5 for e in range(n)]).tolist()) for n in (2, 9, 17, 32)]  # permuted head lists
    for K, h in lists:
        n = len(h)
        ng, order, g_head, g_start, g_count = T.grouped(h, K)
        assert sorted(order) == list(range(n)) and sum(g_count) == n and g_head == sorted(set(h))
        for g in range(ng):
            members = order[g_start[g] : g_start[g] + g_count[g]]
            assert members == [e for e in range(n) if h[e] == g_head[g]], "call order within a head"
        lines.append(_line(n, K, h, (ng, order, g_head, g_start, g_count)))
        want.append("ok")
        if n >= 2:
            rev = order[::-1]
            if rev != order:  # a reversed order breaks the call order or the groups
                lines.append(_line(n, K, h, (ng, rev, g_head, g_start, g_count)))
                want.append(None)
            dup = list(order)
            dup[-1] = dup[0]
            lines.append(_line(n, K, h, (ng, dup, g_head, g_start, g_count)))
            want.append("a state appears twice in the order")
        if ng >= 2:
            lines.append(_line(n, K, h, (ng - 1, order, g_head, g_start, g_count)))
            want.append("the groups do not cover the n states")
            shifted = list(g_start)
            shifted[1] += 1
            lines.append(_line(n, K, h, (ng, order, g_head, shifted, g_count)))
            want.append("a group does not start where the one before it ends")
        lines.append(_line(n, K, h, (ng, order, [g_head[0] + K] + g_head[1:], g_start, g_count)))
        want.append("a group's head is outside [0, n_heads)")
    path = tmp_path / "tables.txt"
    path.write_text("".join(lines))
    out = subprocess.run([probe, str(path)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(want)
    for i, (got, w) in enumerate(zip(out, want)):
        assert (got != "ok") if w is None else (got == w), (lines[i], got, w)


# ---- DeviceAgent._best_actions on a stub ------------------------------------------------------------------------------
K, A, OBS = 3, 4, (2, 2, 2)


class _StubLib:
    def __init__(self, agent, rc):
        self.agent, self.rc, self.calls = agent, rc, []

    def _entry(self, name, handle, which, heads_ptr, states_ptr, n, q_ptr, acts_ptr, stream):
        heads = np.ctypeslib.as_array(C.cast(heads_ptr, C.POINTER(C.c_int32)), (n,)).copy()
        self.calls.append((name, which, heads.tolist(), self.agent._acts_pin_np[:n].copy()))
        if self.rc[name] == 0:
            self.agent._acts_out_np[:n] = (heads + np.arange(n)) % A
        return self.rc[name]

    def idqn_act_host_many(self, *a):
        return self._entry("idqn_act_host_many", *a)

    def idqn_act_host_many_fc(self, *a):
        return self._entry("idqn_act_host_many_fc", *a)

    def idqn_act_host_many_impala(self, *a):
        return self._entry(NAME, *a)

    def idqn_last_error(self):
        return b"stub error"


def _stub_agent(monkeypatch, rc_imp, arch="impala", sizes=(2, 6)):
    import torch

    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent, _HostAction

    agent = DeviceAgent.__new__(DeviceAgent)
    agent._K, agent._obs, agent._arch, agent._handle, agent._pixels = K, OBS, arch, None, True
    agent.act_many_imp_sizes = frozenset(sizes)
    agent._ensure_handle = lambda batch: None
    agent._q_out = torch.zeros((32, A), dtype=torch.float32)
    agent._acts_pin = torch.zeros((32, int(np.prod(OBS))), dtype=torch.uint8)
    agent._acts_pin_np = agent._acts_pin.numpy()
    agent._acts_out = torch.zeros(32, dtype=torch.int32)
    agent._acts_out_np = agent._acts_out.numpy()
    agent.loop_calls = []

    def best_action(which, head, state):
        i = len(agent.loop_calls)
        agent.loop_calls.append((which, head))
        return _HostAction((head + i) % A)

    agent._best_action = best_action
    stub = _StubLib(agent, {"idqn_act_host_many": _hip.E_INVALID, "idqn_act_host_many_fc": _hip.E_INVALID, NAME: rc_imp})
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    return agent, stub


def _inputs(n):
    rng = np.random.default_rng(2)
    return [int(h) for h in rng.integers(0, K, n)], list(rng.integers(0, 256, (n,) + OBS, dtype=np.uint8))


def test_default_sizes_are_a_set_of_call_sizes():
    from slimdqn.networks._agent import DeviceAgent

    assert isinstance(DeviceAgent.act_many_imp_sizes, frozenset) and all(1 <= s <= 32 for s in DeviceAgent.act_many_imp_sizes)


def test_impala_agent_asks_the_new_entry_third(monkeypatch):
    agent, stub = _stub_agent(monkeypatch, 0)
    heads, states = _inputs(6)
    got = agent._best_actions(1, heads, states)
    assert [c[0] for c in stub.calls] == ["idqn_act_host_many", "idqn_act_host_many_fc", NAME]
    assert agent._act_many_ok is False and agent._act_many_fc_ok is False and agent._act_many_imp_ok is True and not agent.loop_calls
    assert got.dtype == np.int64 and got.tolist() == [(h + e) % A for e, h in enumerate(heads)]
    name, which, staged_heads, staged = stub.calls[-1]
    assert which == 1 and staged_heads == heads and all(staged[e].tobytes() == states[e].tobytes() for e in range(6))
    stub.calls.clear()
    agent._best_actions(0, heads[:2], states[:2])
    assert [c[0] for c in stub.calls] == [NAME], "from now on: one call"
    # a size outside the set stays on the loop and leaves the flag alone
    stub.calls.clear()
    got = agent._best_actions(0, heads[:3], states[:3])
    assert not stub.calls and agent.loop_calls == [(0, h) for h in heads[:3]] and agent._act_many_imp_ok is True
    assert got.tolist() == [(h + e) % A for e, h in enumerate(heads[:3])]


def test_a_first_refusal_switches_it_off_and_a_later_one_raises(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, _hip.E_INVALID)
    heads, states = _inputs(6)
    got = agent._best_actions(0, heads, states)
    assert agent._act_many_imp_ok is False and agent.loop_calls == [(0, h) for h in heads]
    assert got.tolist() == [(h + e) % A for e, h in enumerate(heads)]
    stub.calls.clear()
    agent._best_actions(0, heads, states)
    assert not stub.calls, "no entry is asked again"
    agent, stub = _stub_agent(monkeypatch, _hip.E_HIP)
    with pytest.raises(_hip.HipExtensionError, match=NAME):
        agent._best_actions(0, heads, states)
    assert agent.__dict__.get("_act_many_imp_ok") is None and not agent.loop_calls
    agent, stub = _stub_agent(monkeypatch, 0)
    agent._best_actions(0, heads, states)
    stub.rc[NAME] = _hip.E_INVALID
    with pytest.raises(_hip.HipExtensionError):
        agent._best_actions(0, heads, states)


def test_other_architectures_never_ask_it(monkeypatch):
    for arch in ("fc", "cnn"):
        agent, stub = _stub_agent(monkeypatch, 0, arch=arch)
        heads, states = _inputs(6)
        agent._best_actions(0, heads, states)
        assert [c[0] for c in stub.calls] == ["idqn_act_host_many", "idqn_act_host_many_fc"] and len(agent.loop_calls) == 6
        assert agent.__dict__.get("_act_many_imp_ok") is None
