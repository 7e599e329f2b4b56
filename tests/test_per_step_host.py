"""Host-side checks of the one-call prioritized step: the three entries are declared, exported and bound, and
``PrioritizedLearner.step`` picks between ``idqn_per_learn_on_replay`` and the chain of calls as the agent kind, the switches and
the entry's first answer say -- on a stub library, stub buffers and agents that never touched a device.  No GPU needed; the
device side is ``tests/test_gpu_per_step_fused.py``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("per_draw", "per_write_back", "idqn_per_learn_on_replay")
B = 6


def test_entries_are_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    for name in NAMES:
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
    assert lib.idqn_abi_version() == 4
    # idqn_per_step_t as the header lays it out (naturally aligned: depth is padded to 8 bytes, stratified / reduce_max share 8)
    assert C.sizeof(_hip.PerStep) == 120 and _hip.PerStep.tau_dev.offset == 112 and _hip.PerStep.beta.offset == 40


class _T:
    """Stands in for a device tensor."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def numel(self):
        return B


class _StubBuffer:
    _batch_size, add_count = B, 100

    def __init__(self, arch):
        self.arch, self.gathered = arch, 0

    def sample_slots(self):
        raise AssertionError("a prioritized step draws no slots on the host")

    def ring_view(self):
        if self.arch == "fc":
            return "frames", 50, 16, "rows", 2, (4,), np.float32
        return "frames", 50, 400, "rows", 4, (20, 20), np.uint8

    def _gather_device(self, leaves):
        self.gathered += 1


class _StubLib:
    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def idqn_per_learn_on_replay(self, handle, per, ring, n_frames, frame_bytes, rows, batch, stack, divisor, flags, stream):
        p = per._obj
        u = np.ctypeslib.as_array(C.cast(p.uniforms_host, C.POINTER(C.c_double)), (batch,)).copy()
        self.calls.append(dict(u=u, ring=ring, n_frames=n_frames, frame_bytes=frame_bytes, rows=rows, batch=batch, stack=stack,
                               divisor=divisor, flags=flags, n_items=p.n_items, depth=p.depth, tau=p.tau_dev, leaves=p.leaves_dev,
                               beta=p.beta, eps=p.eps, alpha=p.alpha, stratified=p.stratified, reduce_max=p.reduce_max))
        return self.rc

    def idqn_last_error(self):
        return b"stub refusal"


def _learner(monkeypatch, kind, rc=0, agent_cls=None):
    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent
    from slimdqn.networks.iiqn import iIQN
    from slimdqn.sample_collection.per import PrioritizedLearner

    cls = agent_cls or (iIQN if kind == "iqn" else DeviceAgent)
    agent = cls.__new__(cls)
    agent._K, agent._arch, agent._handle, agent._losses = 3, "fc" if kind == "fc" else "cnn", None, "fused losses"
    agent._obs = (8, 1, 1) if kind == "fc" else (20, 20, 4)
    agent._ensure_handle = lambda batch: None
    if kind == "iqn":
        agent._n_quantiles, agent._tau_rng, agent._tau_dev, agent.uploaded = 2, np.random.default_rng(5), _T(900), []
        agent._upload_fractions = lambda batch, taus=None: agent.uploaded.append(taus)
    learner = PrioritizedLearner.__new__(PrioritizedLearner)
    learner.agent, learner.rb = agent, _StubBuffer("fc" if kind == "fc" else "cnn")
    sampler = type("S", (), {"__len__": lambda self: 40})()
    sampler._rng_key, sampler._alpha, sampler._max_priority_dev = np.random.default_rng(11), 0.6, _T(500)
    sampler._sum_tree = type("Tree", (), {})()
    sampler._sum_tree._nodes_dev, sampler._sum_tree._depth, sampler._sum_tree._scratch = _T(100), 7, _T(200)
    learner.sampler = sampler
    learner.beta, learner.eps, learner.reduce_max, learner.stratified = 0.4, 1e-6, 0, 1
    learner._leaves, learner._weights, learner._td_abs, learner._priorities = _T(1), _T(2), _T(3), _T(4)
    learner.fuse_per_family = dict.fromkeys(PrioritizedLearner.fuse_per_family, True)  # the routes, whatever the measured defaults
    learner.chain = []
    learner._step_chain = lambda u, taus=None: learner.chain.append((u.copy(), taus)) or "chain losses"
    stub = _StubLib(rc)
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.setattr(_hip, "ptr", lambda t: t)
    monkeypatch.delenv("IDQN_LEARN_ON_REPLAY", raising=False)
    monkeypatch.delenv("IDQN_PER_FUSED", raising=False)
    return learner, stub


@pytest.mark.parametrize("kind", ["fc", "plane", "iqn"])
def test_every_agent_kind_takes_the_one_call_step(monkeypatch, kind):
    learner, stub = _learner(monkeypatch, kind)
    want = np.random.default_rng(11).random((3, B))
    for i in range(3):
        assert learner.step() == "fused losses"
    assert not learner.chain and not learner.rb.gathered and learner._fused_ok is True and len(stub.calls) == 3
    for i, c in enumerate(stub.calls):
        assert c["u"].tobytes() == want[i].tobytes()  # the sampler's generator, one draw of B per step
        assert (c["ring"], c["rows"], c["batch"], c["divisor"], c["flags"]) == ("frames", "rows", B, B, 0)
        assert (c["n_items"], c["depth"], c["leaves"], c["beta"], c["alpha"], c["stratified"]) == (40, 7, 1, 0.4, 0.6, 1)
        assert (c["stack"], c["frame_bytes"]) == ((2, 16) if kind == "fc" else (4, 400))
        assert c["tau"] == (900 if kind == "iqn" else None)
    agent = learner.agent
    if kind == "iqn":
        taus = np.random.default_rng(5).random((3, 3, 2, B)).astype(np.float32)
        assert len(agent.uploaded) == 3 and agent.uploaded[0].tobytes() == taus.tobytes()
        assert agent._replay_fused_ok is True
    elif kind == "fc":
        assert agent._replay_fc_ok is True
    else:
        assert agent.__dict__.get("_replay_fused_ok") is None and agent.__dict__.get("_replay_fc_ok") is None


@pytest.mark.parametrize("kind", ["fc", "plane", "iqn"])
@pytest.mark.parametrize("switch", ["attribute", "environment", "agent attribute", "agent environment", "family"])
def test_the_switches_keep_the_chain(monkeypatch, kind, switch):
    learner, stub = _learner(monkeypatch, kind)
    if switch == "attribute":
        learner.fuse_per_step = False
    elif switch == "environment":
        monkeypatch.setenv("IDQN_PER_FUSED", "0")
    elif switch == "agent attribute":
        learner.agent.fuse_replay_sampling = False
    elif switch == "agent environment":
        monkeypatch.setenv("IDQN_LEARN_ON_REPLAY", "0")
    else:
        learner.fuse_per_family = dict(learner.fuse_per_family, **{kind: False})
    want = np.random.default_rng(11).random((2, B))
    for i in range(2):
        assert learner.step() == "chain losses"
    assert not stub.calls and learner.__dict__.get("_fused_ok") is None
    assert [u.tobytes() for u, _ in learner.chain] == [want[0].tobytes(), want[1].tobytes()]
    assert all(t is None for _, t in learner.chain)  # (the chain draws an i-IQN agent's fractions itself)


@pytest.mark.parametrize("kind", ["fc", "iqn"])
def test_a_first_refusal_runs_the_chain_on_the_same_draws_and_is_never_retried(monkeypatch, kind):
    from slimdqn import _hip

    learner, stub = _learner(monkeypatch, kind, rc=_hip.E_INVALID)
    want = np.random.default_rng(11).random((2, B))
    assert learner.step() == "chain losses"
    assert len(stub.calls) == 1 and learner._fused_ok is False and learner.fused_refusal == "stub refusal"
    u, taus = learner.chain[0]
    assert u.tobytes() == want[0].tobytes() == stub.calls[0]["u"].tobytes()  # the same uniforms, nothing more drawn
    if kind == "iqn":
        assert taus.tobytes() == np.random.default_rng(5).random((3, 3, 2, B)).astype(np.float32).tobytes()
    assert learner.step() == "chain losses"
    assert len(stub.calls) == 1 and learner.chain[1][0].tobytes() == want[1].tobytes()  # the generator went on from where it was


def test_family_defaults_and_the_general_shape_rule(monkeypatch):
    from slimdqn.sample_collection.per import PrioritizedLearner

    assert PrioritizedLearner.fuse_per_step is True and set(PrioritizedLearner.fuse_per_family) == {"plane", "fc", "gcnn", "iqn"}
    learner, stub = _learner(monkeypatch, "plane")
    net = type("Net", (), {"features": [32, 64, 64, 512], "n_actions": 6})()
    learner.agent.network = net
    assert not learner._general_shape(learner.agent)
    net.features = [2, 3, 1, 15]
    assert learner._general_shape(learner.agent)
    learner.fuse_per_family = dict(learner.fuse_per_family, gcnn=False)
    assert learner.step() == "chain losses" and not stub.calls  # a family switched off keeps the chain
    net.features = [32, 64, 64, 512]
    learner.agent._replay_fused_ok = False  # the plane entry refused this handle: general shape, whatever the rule says
    assert learner._general_shape(learner.agent)


def test_a_later_refusal_and_a_hip_error_raise(monkeypatch):
    from slimdqn import _hip

    learner, stub = _learner(monkeypatch, "fc")
    learner.step()
    stub.rc = _hip.E_INVALID
    with pytest.raises(_hip.HipExtensionError, match="idqn_per_learn_on_replay"):
        learner.step()
    learner2, _ = _learner(monkeypatch, "fc", rc=_hip.E_HIP)
    with pytest.raises(_hip.HipExtensionError, match="idqn_per_learn_on_replay"):
        learner2.step()
    assert not learner.chain and not learner2.chain


def test_a_subclass_with_its_own_learn_keeps_the_chain(monkeypatch):
    from slimdqn.networks._agent import DeviceAgent
    from slimdqn.networks.iiqn import iIQN

    class OwnLearn(DeviceAgent):
        def _learn(self, batch, flags=0, mean_divisor=None):
            return "own"

    class OwnQuantileLearn(iIQN):
        def _learn(self, batch, flags=0, mean_divisor=None, taus=None):
            return "own"

    for kind, cls in (("fc", OwnLearn), ("plane", OwnLearn), ("iqn", OwnQuantileLearn)):
        learner, stub = _learner(monkeypatch, kind, agent_cls=cls)
        assert learner.step() == "chain losses" and not stub.calls and len(learner.chain) == 1


def test_a_ring_outside_the_domain_or_a_large_batch_keeps_the_chain(monkeypatch):
    learner, stub = _learner(monkeypatch, "fc")
    learner.rb.ring_view = lambda: ("frames", 50, 32, "rows", 2, (4,), np.float64)
    assert learner.step() == "chain losses" and not stub.calls
    learner, stub = _learner(monkeypatch, "plane")
    learner.rb._batch_size = 257
    assert learner.step() == "chain losses" and not stub.calls
