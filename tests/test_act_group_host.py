"""Host logic of the acting groups (no GPU): the three entries are declared, exported and bound; what the header and
csrc/act_group_args.h fix agrees with the binding; the table builder's order and groups against a numpy restatement for random
assignments (through tools/probes/act_group_args_probe.cpp, which also runs its own checks); ``AgentGroup.best_actions`` routes cnn
members under ``_group_act_cnn_ok`` (unset: not tried; a first refusal sticks; a later one raises); ``SeedVectorTrainer`` sends the
S x E greedy states of such a group through chunks of at most 32; the Atari seeds entry script takes the flags of the LunarLander
one.  The device is a stub.  On the parent commit the symbols, the flag and the script do not exist."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("idqn_act_group_create", "idqn_act_group_destroy", "idqn_act_group_host")


def _cxx():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)


def test_entries_are_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    for name in NAMES:
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
    assert "typedef struct idqn_act_group_s* idqn_act_group_t;" in header
    # the contract and signature pattern of the fc group's entries
    assert _hip.SYMBOLS["idqn_act_group_host"] == _hip.SYMBOLS["idqn_group_act_host_fc"]
    assert _hip.SYMBOLS["idqn_act_group_create"] == _hip.SYMBOLS["idqn_group_create"]
    assert _hip.SYMBOLS["idqn_act_group_destroy"] == _hip.SYMBOLS["idqn_group_destroy"]
    if os.path.exists(_hip.LIB_PATH):
        nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
        exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                                  capture_output=True, text=True).stdout
        for name in NAMES:
            assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        lib = _hip.lib()
        for name in NAMES:
            assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
        assert lib.idqn_abi_version() == 4  # entries added only


def test_header_and_args_header_against_the_binding(tmp_path):
    """The new entries add no record: the group is an opaque pointer, and the limits of csrc/act_group_args.h are the binding's.
    The records the group entries of the header share with the binding keep their layout."""
    from slimdqn import _hip

    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idqn_hip.h"\n#include "act_group_args.h"\n'
                   'int main() { printf("%zu %zu %d %zu %zu\\n", sizeof(idqn_act_group_t), sizeof(idqn_group_t), ACT_GROUP_MAX, '
                   "sizeof(idqn_group_ring_t), offsetof(idqn_group_ring_t, stack)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "i-dqn_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(C.c_void_p), C.sizeof(C.c_void_p), _hip.ACT_MANY_MAX, C.sizeof(_hip.GroupRing), _hip.GroupRing.stack.offset]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("probe") / "act_group_args_probe"
    subprocess.run([cc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "i-dqn_amd", "csrc"),
                    os.path.join(ROOT, "tools", "probes", "act_group_args_probe.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_probe_builds_and_reports_no_failures(probe):
    out = subprocess.run([probe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    m = re.search(r"^ok: (\d+) checks, 0 failures$", out.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) > 1000, out.stdout[-500:]


def _numpy_table(members, heads, K):
    members, heads = np.asarray(members), np.asarray(heads)
    order = np.argsort(members * K + heads, kind="stable")
    pairs = np.stack([members[order], heads[order]], axis=1)
    starts = [0] + [i for i in range(1, len(order)) if (pairs[i] != pairs[i - 1]).any()]
    counts = np.diff(starts + [len(order)]).tolist()
    return [len(starts), order.tolist(), pairs[starts, 0].tolist(), pairs[starts, 1].tolist(), starts, counts]


def test_table_builder_against_numpy(probe, tmp_path):
    rng = np.random.default_rng(3)
    cases = []
    for n in range(1, 33):
        for S, K in ((1, 1), (2, 2), (3, 5), (8, 5), (32, 5), (32, 1)):
            cases.append((K, rng.integers(0, S, n).tolist(), rng.integers(0, K, n).tolist()))
    cases.append((5, [1] * 32, [4] * 32))
    cases.append((5, list(range(31, -1, -1)), [e % 5 for e in range(32)]))
    path = tmp_path / "cases.txt"
    path.write_text("".join(" ".join(str(x) for x in [len(m)] + m + h) + "\n" for _, m, h in cases))
    out = subprocess.run([probe, str(path)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(cases)
    for line, (K, m, h) in zip(out, cases):
        got = [[int(x) for x in part.split()] for part in line.split("|")]
        want = _numpy_table(m, h, K)
        assert got[0] == [want[0]] and got[1:] == want[1:], (m, h, line)
        assert want[0] <= min(len(m), 32) and sum(want[5]) == len(m)


# ---- AgentGroup.best_actions on stubs ---------------------------------------------------------------------------------
class _Lib:
    def __init__(self, refuse_create=(), refuse_host=()):
        self.calls, self.refuse_create, self.refuse_host, self.created = [], set(refuse_create), set(refuse_host), 0

    def idqn_act_group_create(self, arr, n, out):
        self.created += 1
        self.calls.append(("create", [arr[i] for i in range(n)]))
        if self.created in self.refuse_create:
            return -1
        out._obj.value = 900 + self.created
        return 0

    def idqn_act_group_destroy(self, g):
        self.calls.append(("destroy", g.value))
        return 0

    def idqn_group_destroy(self, g):
        return 0

    def idqn_act_group_host(self, g, which, members, heads, pin, n, q_out, acts, stream):
        m = np.ctypeslib.as_array(C.cast(members, C.POINTER(C.c_int32)), (n,)).copy()
        h = np.ctypeslib.as_array(C.cast(heads, C.POINTER(C.c_int32)), (n,)).copy()
        states = np.ctypeslib.as_array(C.cast(pin, C.POINTER(C.c_uint8)), (n, 16)).copy()
        k = sum(1 for c in self.calls if c[0] == "host") + 1
        self.calls.append(("host", g.value, which, m.tolist(), h.tolist(), n))
        if k in self.refuse_host:
            return -1
        out = np.ctypeslib.as_array(C.cast(acts, C.POINTER(C.c_int32)), (n,))
        out[:] = [_greedy(mi, hi, s) for mi, hi, s in zip(m, h, states)]
        return 0

    def idqn_last_error(self):
        return b"stub refusal"


def _greedy(member, head, state):
    return (int(np.asarray(state).reshape(-1)[0]) + 3 * int(member) + int(head)) % 5


def _stub_group(monkeypatch, S, lib, arch="cnn"):
    import torch

    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent, _HostAction
    from slimdqn.networks.group import AgentGroup

    loop = []
    agents = []
    for g in range(S):
        a = DeviceAgent.__new__(DeviceAgent)
        a._K, a._arch, a._obs, a._handle = 3, arch, (2, 2, 4), C.c_void_p(500 + g)
        a.network = types.SimpleNamespace(n_actions=5, features=[32, 32, 32, 128])
        a._ensure_handle = lambda batch: None
        a._best_action = lambda which, head, state, g=g: loop.append((g, which, head)) or _HostAction(_greedy(g, head, state))
        agents.append(a)
    group = AgentGroup(agents)
    group.act_group_sizes = frozenset({S})
    # (no device: ordinary host tensors stand in for the pinned staging buffers)
    group._pin_u8 = torch.zeros((32, 16), dtype=torch.uint8)
    group._pin_u8_np = group._pin_u8.numpy()
    group._out = torch.zeros(32, dtype=torch.int32)
    group._out_np = group._out.numpy()
    group.q_out = torch.zeros((32, 5), dtype=torch.float32)
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    return group, loop


def _states(n, seed=0):
    return list(np.random.default_rng(seed).integers(0, 256, (n, 2, 2, 4), dtype=np.uint8))


def test_best_actions_takes_the_group_call(monkeypatch):
    lib = _Lib()
    group, loop = _stub_group(monkeypatch, 3, lib)
    members, heads, states = [2, 0, 0, 1], [1, 2, 0, 1], _states(4)
    got = group.best_actions(0, heads, states, members)
    assert got.tolist() == [_greedy(m, h, s) for m, h, s in zip(members, heads, states)] and got.dtype == np.int64
    assert group._group_act_cnn_ok is True and not loop
    assert [c[0] for c in lib.calls] == ["create", "host"] and lib.calls[0][1] == [500, 501, 502]
    assert lib.calls[1][1:] == (901, 0, members, heads, 4)
    group.best_actions(1, [0, 0, 0], _states(3))  # default members: one state per member; the same C object
    assert [c[0] for c in lib.calls] == ["create", "host", "host"] and lib.calls[2][3] == [0, 1, 2] and lib.calls[2][2] == 1
    # a member re-creates its handle: the group is destroyed and created again over the new handles
    group.agents[1]._handle = C.c_void_p(777)
    group.best_actions(0, heads, states, members)
    assert [c[0] for c in lib.calls][3:] == ["destroy", "create", "host"] and lib.calls[3][1] == 901 and lib.calls[4][1] == [500, 777, 502]
    group.close()
    assert lib.calls[-1] == ("destroy", 902)


@pytest.mark.parametrize("where", ["create", "host"])
def test_a_first_refusal_sticks_and_the_loop_runs(monkeypatch, where):
    lib = _Lib(refuse_create={1} if where == "create" else (), refuse_host={1} if where == "host" else ())
    group, loop = _stub_group(monkeypatch, 2, lib)
    members, heads, states = [1, 0, 1], [0, 2, 1], _states(3)
    want = [_greedy(m, h, s) for m, h, s in zip(members, heads, states)]
    assert group.best_actions(0, heads, states, members).tolist() == want
    assert group._group_act_cnn_ok is False and loop == [(1, 0, 0), (0, 0, 2), (1, 0, 1)]
    n_calls = len(lib.calls)
    assert group.best_actions(0, heads, states, members).tolist() == want
    assert len(lib.calls) == n_calls and len(loop) == 6, "the loop, and the library is not asked again"


@pytest.mark.parametrize("where", ["create", "host"])
def test_a_later_refusal_raises(monkeypatch, where):
    from slimdqn import _hip

    lib = _Lib(refuse_create={2} if where == "create" else (), refuse_host={2} if where == "host" else ())
    group, loop = _stub_group(monkeypatch, 2, lib)
    group.best_actions(0, [0, 1], _states(2))
    assert group._group_act_cnn_ok is True
    if where == "create":
        group.agents[0]._handle = C.c_void_p(321)
    with pytest.raises(_hip.HipExtensionError):
        group.best_actions(0, [0, 1], _states(2))
    assert not loop


def test_the_route_is_off_for_other_sizes_members_and_overrides(monkeypatch):
    from slimdqn.networks._agent import DeviceAgent
    from slimdqn.networks.group import AgentGroup

    assert isinstance(AgentGroup.act_group_sizes, frozenset) and all(1 <= s <= 32 for s in AgentGroup.act_group_sizes)
    lib = _Lib()
    group, loop = _stub_group(monkeypatch, 2, lib)
    assert group._stock_act_cnn() and not group._stock(), "the learner routes keep their own rule"
    group.act_group_sizes = frozenset({3})
    assert not group._stock_act_cnn()
    group.best_actions(0, [0, 1], _states(2))
    assert len(loop) == 2 and not lib.calls and group.__dict__.get("_group_act_cnn_ok") is None
    group.act_group_sizes = frozenset({2})
    group.agents[1].network.n_actions = 6
    assert not group._stock_act_cnn(), "members of different shapes"
    group.agents[1].network.n_actions = 5
    group.agents[1]._n_quantiles = 8
    assert not group._stock_act_cnn(), "quantile heads"
    del group.agents[1]._n_quantiles

    class Own(DeviceAgent):
        def _best_actions(self, which, heads, states):
            raise AssertionError

    group.agents[0].__class__ = Own
    assert not group._stock_act_cnn(), "an acting rule of its own"
    fc_group, _ = _stub_group(monkeypatch, 2, lib, arch="fc")
    assert not fc_group._stock_act_cnn()


# ---- SeedVectorTrainer: chunks of 32 ---------------------------------------------------------------------------------------
def test_seed_vector_trainer_sends_chunks_of_at_most_32(monkeypatch):
    from experiments.base.seeds import SeedVectorTrainer
    from slimdqn import prng

    lib = _Lib()
    S, E = 5, 8
    group, loop = _stub_group(monkeypatch, S, lib)
    for a in group.agents:
        a.n_networks, a.params = 3, None

    class Env:
        n_actions = 5

        def __init__(self, v):
            self.state = np.full((2, 2, 4), v, np.uint8)

    p = dict(epsilon_end=0.0, epsilon_duration=1, n_epochs=1)
    envs = [[Env(8 * g + e) for e in range(E)] for g in range(S)]
    trainer = SeedVectorTrainer([prng.PRNGKey(g) for g in range(S)], p, group.agents, envs, [None] * S, group=group, collector=object())
    for s in trainer.seeds:
        s.total_steps = 10  # epsilon has reached 0: every state is greedy
    out = trainer._select_actions(list(range(S)))
    hosts = [c for c in lib.calls if c[0] == "host"]
    assert [c[5] for c in hosts] == [32, 8] and not loop
    assert hosts[0][3] == [g for g in range(4) for _ in range(E)] and hosts[1][3] == [4] * 8, "in (seed, environment) order"
    for g in range(S):
        idx, actions = out[g]
        assert idx == list(range(E)) and all(0 <= a < 5 for a in actions)
    flat_heads = hosts[0][4] + hosts[1][4]
    want = [_greedy(g, flat_heads[g * E + e], envs[g][e].state) for g in range(S) for e in range(E)]
    assert [a for g in range(S) for a in out[g][1]] == want


def test_atari_seeds_entry_script_takes_the_flags():
    from experiments.atari import idqn_seeds

    for argv in (["--first_seed", "3", "--last_seed", "2"], ["--first_seed", "0", "--last_seed", "32"],
                 ["--first_seed", "0", "--last_seed", "1", "--n_envs", "0"]):
        with pytest.raises(SystemExit):
            idqn_seeds.run(argv)
    with pytest.raises(SystemExit):
        idqn_seeds.run(["--last_seed", "2"])  # --first_seed is required
