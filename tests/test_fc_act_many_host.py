"""Host-side checks of vectorised acting on MLP / general-shape cnn handles: ``idqn_act_host_many_fc`` is declared in the
header, exported by the built library and bound in ``_hip`` (the ABI version stays 4: an entry was added, none changed), and
``DeviceAgent._best_actions`` dispatches between ``idqn_act_host_many``, ``idqn_act_host_many_fc`` and the loop of
``_best_action`` as the two entries' answers say -- on a stub library and an agent that never touched a device.  No GPU
needed; the device side is ``tests/test_gpu_fc_act_many.py``."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_act_host_many_fc"


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    assert NAME in _hip.SYMBOLS, f"{NAME} is not bound in slimdqn/_hip.py"
    assert _hip.SYMBOLS[NAME] == _hip.SYMBOLS["idqn_act_host_many"]  # signature and contract of idqn_act_host_many
    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), f"{NAME} is not declared in include/idqn_hip.h"
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+" + NAME + r"$", exported, re.M), f"{NAME} is not exported by the library"
    assert getattr(lib, NAME).argtypes == _hip.SYMBOLS[NAME][1]
    assert lib.idqn_abi_version() == 4


K, A, OBS = 3, 4, (8, 1, 1)


class _StubLib:
    """The two vectorised entries with scripted return codes; an accepted call answers action e = (head e + e) % A and
    Q row e = e.  Every call is recorded."""

    def __init__(self, agent, rc_many, rc_fc):
        self.agent, self.rc, self.calls = agent, {"idqn_act_host_many": rc_many, "idqn_act_host_many_fc": rc_fc}, []

    def _entry(self, name, handle, which, heads_ptr, states_ptr, n, q_ptr, acts_ptr, stream):
        import ctypes as C

        heads = np.ctypeslib.as_array(C.cast(heads_ptr, C.POINTER(C.c_int32)), (n,)).copy()
        self.calls.append((name, which, heads.tolist(), self.agent._acts_pin_np[:n].copy()))
        if self.rc[name] == 0:
            self.agent._acts_out_np[:n] = (heads + np.arange(n)) % A
            self.agent._q_out[:n] = self.agent._q_out.new_tensor(np.arange(n, dtype=np.float32))[:, None]
        return self.rc[name]

    def idqn_act_host_many(self, *a):
        return self._entry("idqn_act_host_many", *a)

    def idqn_act_host_many_fc(self, *a):
        return self._entry("idqn_act_host_many_fc", *a)

    def idqn_last_error(self):
        return b"stub error"


def _stub_agent(monkeypatch, rc_many, rc_fc):
    """A DeviceAgent that never touched a device: the attributes ``_best_actions`` reads, ordinary host tensors for the staging
    block and the Q rows, a recording ``_best_action`` for the loop, and the stub library behind ``_hip.lib``."""
    import torch

    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent, _HostAction

    agent = DeviceAgent.__new__(DeviceAgent)
    agent._K, agent._obs, agent._arch, agent._handle = K, OBS, "fc", None
    agent._ensure_handle = lambda batch: None
    agent._q_out = torch.zeros((32, A), dtype=torch.float32)
    agent._acts_pin = torch.zeros((32, int(np.prod(OBS))), dtype=torch.float32)
    agent._acts_pin_np = agent._acts_pin.numpy()
    agent._acts_out = torch.zeros(32, dtype=torch.int32)
    agent._acts_out_np = agent._acts_out.numpy()
    agent.loop_calls = []

    def best_action(which, head, state):
        i = len(agent.loop_calls)
        agent.loop_calls.append((which, head, np.asarray(state).copy()))
        agent._q_out[0] = float(i)
        return _HostAction((head + i) % A)  # what the stub entries answer for position i of a call

    agent._best_action = best_action
    stub = _StubLib(agent, rc_many, rc_fc)
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    return agent, stub


def _inputs(n=6):
    rng = np.random.default_rng(2)
    return [int(h) for h in rng.integers(0, K, n)], [rng.standard_normal(OBS[0]).astype(np.float32) for _ in range(n)]


def test_first_entry_refuses_second_serves(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, _hip.E_INVALID, 0)
    heads, states = _inputs()
    got = agent._best_actions(1, heads, states)
    assert [c[0] for c in stub.calls] == ["idqn_act_host_many", "idqn_act_host_many_fc"]
    assert agent._act_many_ok is False and agent._act_many_fc_ok is True and not agent.loop_calls
    assert got.dtype == np.int64 and got.tolist() == [(h + e) % A for e, h in enumerate(heads)]
    name, which, staged_heads, staged = stub.calls[-1]
    assert which == 1 and staged_heads == heads and staged.dtype == np.float32
    assert all(staged[e].tobytes() == states[e].tobytes() for e in range(len(heads)))
    assert agent._q_out[: len(heads), 0].tolist() == list(range(len(heads)))
    # from now on: ONE call per best_actions, to the second entry
    stub.calls.clear()
    again = agent._best_actions(1, heads, states)
    assert [c[0] for c in stub.calls] == ["idqn_act_host_many_fc"] and again.tolist() == got.tolist()


def test_both_refuse_then_it_is_the_loop_with_the_same_actions(monkeypatch):
    from slimdqn import _hip

    heads, states = _inputs()
    served, _ = _stub_agent(monkeypatch, _hip.E_INVALID, 0)
    want = served._best_actions(0, heads, states)
    want_rows = served._q_out[: len(heads)].clone()
    agent, stub = _stub_agent(monkeypatch, _hip.E_INVALID, _hip.E_INVALID)
    got = agent._best_actions(0, heads, states)
    assert [c[0] for c in stub.calls] == ["idqn_act_host_many", "idqn_act_host_many_fc"]
    assert agent._act_many_ok is False and agent._act_many_fc_ok is False
    assert [(w, h) for w, h, _ in agent.loop_calls] == [(0, h) for h in heads]
    assert all(s.tobytes() == states[e].tobytes() for e, (_, _, s) in enumerate(agent.loop_calls))
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    assert agent._q_out[: len(heads)].numpy().tobytes() == want_rows.numpy().tobytes()
    # neither entry is asked again
    stub.calls.clear()
    agent.loop_calls.clear()
    assert agent._best_actions(0, heads, states).tolist() == want.tolist() and not stub.calls


def test_another_error_from_the_second_entry_raises(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, _hip.E_INVALID, _hip.E_HIP)
    heads, states = _inputs()
    with pytest.raises(_hip.HipExtensionError, match="idqn_act_host_many_fc"):
        agent._best_actions(0, heads, states)
    assert not agent.loop_calls and agent.__dict__.get("_act_many_fc_ok") is None


def test_a_refusal_after_the_entry_has_served_raises(monkeypatch):
    """E_INVALID is a domain answer only on the first call: later it is a caller's error and is reported."""
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, _hip.E_INVALID, 0)
    heads, states = _inputs()
    agent._best_actions(0, heads, states)
    stub.rc["idqn_act_host_many_fc"] = _hip.E_INVALID
    with pytest.raises(_hip.HipExtensionError):
        agent._best_actions(0, heads, states)
    assert not agent.loop_calls
