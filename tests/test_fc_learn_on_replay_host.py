"""Host-side checks of the replay-sourced learner step on MLP / general-shape cnn handles: ``idqn_learn_on_replay_fc`` and
``idqn_learn_on_replay_fc_dev`` are declared in the header, exported by the built library and bound in ``_hip`` with the
signature of ``idqn_learn_on_replay`` (the ABI version stays 4: entries were added, none changed), and
``DeviceAgent._sample_and_learn`` dispatches between ``idqn_learn_on_replay``, ``idqn_learn_on_replay_fc`` and gather-then-learn
as the entries' answers and the switches say -- on a stub library, a stub buffer and an agent that never touched a device.  No
GPU needed; the device side is ``tests/test_gpu_fc_learn_on_replay.py``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("idqn_learn_on_replay_fc", "idqn_learn_on_replay_fc_dev")


def test_entries_are_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    for name, twin in zip(NAMES, ("idqn_learn_on_replay", "idqn_learn_on_replay_dev")):
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        assert _hip.SYMBOLS[name] == _hip.SYMBOLS[twin]  # signature and contract of the plane entry
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
    assert lib.idqn_abi_version() == 4


B = 6
SLOT_DRAWS = [np.array([5, 1, 9, 9, 0, 3], np.int64) + 10 * i for i in range(8)]


class _StubBuffer:
    """``sample_slots`` hands out scripted draws; ``_gather`` / ``sample`` record what they were asked for."""

    _batch_size = B

    def __init__(self, arch):
        self.arch, self.draws, self.gathered, self.sampled = arch, 0, [], 0

    def sample_slots(self):
        self.draws += 1
        return SLOT_DRAWS[self.draws - 1].astype(np.int32)

    def ring_view(self):
        if self.arch == "fc":
            return "frames", 50, 16, "rows", 2, (4,), np.float32  # 4 float32 elements x stack 2 = obs dim 8
        return "frames", 50, 400, "rows", 4, (20, 20), np.uint8

    def _gather(self, slots):
        self.gathered.append(np.asarray(slots).copy())
        return ("batch", len(self.gathered))

    def sample(self):
        self.sampled += 1
        return ("sampled", self.sampled)


class _StubLib:
    def __init__(self, rc_plane, rc_fc):
        self.rc, self.calls = {"idqn_learn_on_replay": rc_plane, "idqn_learn_on_replay_fc": rc_fc}, []

    def _entry(self, name, handle, ring, n_frames, frame_bytes, rows, slots_ptr, batch, stack, divisor, flags, stream):
        slots = np.ctypeslib.as_array(C.cast(slots_ptr, C.POINTER(C.c_int32)), (batch,)).copy()
        self.calls.append((name, ring, n_frames, frame_bytes, rows, slots.tolist(), batch, stack, divisor, flags))
        return self.rc[name]

    def idqn_learn_on_replay(self, *a):
        return self._entry("idqn_learn_on_replay", *a)

    def idqn_learn_on_replay_fc(self, *a):
        return self._entry("idqn_learn_on_replay_fc", *a)

    def idqn_last_error(self):
        return b"stub error"


def _stub_agent(monkeypatch, arch, rc_plane=0, rc_fc=0):
    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent

    agent = DeviceAgent.__new__(DeviceAgent)
    agent._K, agent._arch, agent._handle = 3, arch, None
    agent._obs = (8, 1, 1) if arch == "fc" else (20, 20, 4)
    agent._ensure_handle = lambda batch: None
    agent._losses = "losses"
    agent.learned = []
    agent._learn = lambda batch: agent.learned.append(batch) or "losses of the two-call form"
    stub = _StubLib(rc_plane, rc_fc)
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.setattr(_hip, "ptr", lambda t: t)
    monkeypatch.delenv("IDQN_LEARN_ON_REPLAY", raising=False)
    return agent, stub


def test_fc_agent_goes_to_the_new_entry_with_the_drawn_slots(monkeypatch):
    agent, stub = _stub_agent(monkeypatch, "fc")
    rb = _StubBuffer("fc")
    for i in range(3):
        assert agent._sample_and_learn(rb) == "losses"
    assert agent._replay_fc_ok is True and agent.__dict__.get("_replay_fused_ok") is None
    assert not rb.gathered and not rb.sampled and not agent.learned and rb.draws == 3
    assert stub.calls == [("idqn_learn_on_replay_fc", "frames", 50, 16, "rows", SLOT_DRAWS[i].tolist(), B, 2, B, 0) for i in range(3)]


def test_a_first_refusal_falls_back_with_the_same_slots_and_is_never_retried(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, "fc", rc_fc=_hip.E_INVALID)
    rb = _StubBuffer("fc")
    assert agent._sample_and_learn(rb) == "losses of the two-call form"
    assert [c[0] for c in stub.calls] == ["idqn_learn_on_replay_fc"] and agent._replay_fc_ok is False
    assert len(rb.gathered) == 1 and rb.gathered[0].tolist() == SLOT_DRAWS[0].tolist() == stub.calls[0][5]
    assert agent.learned == [("batch", 1)] and rb.draws == 1 and not rb.sampled
    # from now on: sample() + learn, the entry is not asked again
    stub.calls.clear()
    agent._sample_and_learn(rb)
    assert not stub.calls and rb.sampled == 1 and agent.learned[-1] == ("sampled", 1)


def test_a_ring_outside_the_domain_is_not_offered(monkeypatch):
    agent, stub = _stub_agent(monkeypatch, "fc")
    rb = _StubBuffer("fc")
    rb.ring_view = lambda: ("frames", 50, 32, "rows", 2, (4,), np.float64)  # float64 frames: the gather casts, the entry cannot
    assert agent._sample_and_learn(rb) == "losses of the two-call form"
    assert not stub.calls and agent._replay_fc_ok is False and rb.gathered[0].tolist() == SLOT_DRAWS[0].tolist()


def test_a_later_refusal_raises(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, "fc")
    rb = _StubBuffer("fc")
    agent._sample_and_learn(rb)
    stub.rc["idqn_learn_on_replay_fc"] = _hip.E_INVALID
    with pytest.raises(_hip.HipExtensionError, match="idqn_learn_on_replay_fc"):
        agent._sample_and_learn(rb)
    assert not agent.learned and agent._replay_fc_ok is True


def test_a_hip_error_raises(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, "fc", rc_fc=_hip.E_HIP)
    with pytest.raises(_hip.HipExtensionError, match="idqn_learn_on_replay_fc"):
        agent._sample_and_learn(_StubBuffer("fc"))
    assert not agent.learned and agent.__dict__.get("_replay_fc_ok") is None


@pytest.mark.parametrize("arch", ["fc", "cnn"])
@pytest.mark.parametrize("switch", ["attribute", "environment"])
def test_the_switches_turn_the_new_route_off_too(monkeypatch, arch, switch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, arch, rc_plane=_hip.E_INVALID)
    if switch == "attribute":
        agent.fuse_replay_sampling = False
    else:
        monkeypatch.setenv("IDQN_LEARN_ON_REPLAY", "0")
    rb = _StubBuffer(arch)
    for _ in range(2):
        agent._sample_and_learn(rb)
    assert not stub.calls and rb.sampled == 2 and not rb.draws
    assert agent.__dict__.get("_replay_fc_ok") is None and agent.__dict__.get("_replay_fused_ok") is None


def test_plane_path_agents_never_call_it(monkeypatch):
    agent, stub = _stub_agent(monkeypatch, "cnn")
    rb = _StubBuffer("cnn")
    for _ in range(3):
        assert agent._sample_and_learn(rb) == "losses"
    assert [c[0] for c in stub.calls] == ["idqn_learn_on_replay"] * 3
    assert agent._replay_fused_ok is True and agent.__dict__.get("_replay_fc_ok") is None and not agent.learned


def test_a_cnn_handle_the_plane_entry_refuses_takes_the_new_entry_with_the_same_slots(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, "cnn", rc_plane=_hip.E_INVALID)
    rb = _StubBuffer("cnn")
    for _ in range(2):
        assert agent._sample_and_learn(rb) == "losses"
    assert [c[0] for c in stub.calls] == ["idqn_learn_on_replay", "idqn_learn_on_replay_fc", "idqn_learn_on_replay_fc"]
    assert stub.calls[0][5] == stub.calls[1][5] == SLOT_DRAWS[0].tolist() and stub.calls[2][5] == SLOT_DRAWS[1].tolist()
    assert agent._replay_fused_ok is False and agent._replay_fc_ok is True and not agent.learned and rb.draws == 2


def test_a_cnn_handle_both_entries_refuse_gathers_the_same_slots(monkeypatch):
    from slimdqn import _hip

    agent, stub = _stub_agent(monkeypatch, "cnn", rc_plane=_hip.E_INVALID, rc_fc=_hip.E_INVALID)
    rb = _StubBuffer("cnn")
    assert agent._sample_and_learn(rb) == "losses of the two-call form"
    assert [c[0] for c in stub.calls] == ["idqn_learn_on_replay", "idqn_learn_on_replay_fc"]
    assert agent._replay_fused_ok is False and agent._replay_fc_ok is False
    assert rb.draws == 1 and rb.gathered[0].tolist() == SLOT_DRAWS[0].tolist() and agent.learned == [("batch", 1)]
    stub.calls.clear()
    agent._sample_and_learn(rb)
    assert not stub.calls and rb.sampled == 1
