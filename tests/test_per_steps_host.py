"""Host-side checks of the n-step prioritized call: ``per_turn`` and ``idqn_per_learn_steps_on_replay`` are declared, exported and
bound, ``PrioritizedLearner.steps`` draws the sampler's generator as n ``step()`` calls do, every row of uniforms goes through
exactly one route in order (``per_steps_min``, ``_steps_ok``, ``MAX_STEPS_PER_CALL``), and ``update_params_many`` puts the target
operations where ``plan_step_runs`` does -- on a stub library, stub buffers and agents that never touched a device.  No GPU
needed; the device side is ``tests/test_gpu_per_turn.py`` and ``tests/test_gpu_per_steps.py``."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("per_turn", "idqn_per_learn_steps_on_replay")
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
    assert "idqn_per_steps_t" in header
    # idqn_per_steps_t: idqn_per_step_t without its last field, tau_dev
    assert C.sizeof(_hip.PerSteps) == 112 and _hip.PerSteps.tree_scratch_dev.offset == 104 and _hip.PerSteps.beta.offset == 40
    assert [f[0] for f in _hip.PerSteps._fields_] == [f[0] for f in _hip.PerStep._fields_ if f[0] != "tau_dev"]
    assert _hip.MAX_STEPS_PER_CALL == int(re.search(r"#define IDQN_MAX_STEPS_PER_CALL (\d+)", header).group(1))


class _T:
    """Stands in for a device tensor; ``t[i]`` is row i."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def numel(self):
        return B

    def __getitem__(self, i):
        return _T(self.address + 1000 * (i + 1))


class _StubBuffer:
    _batch_size, add_count = B, 100

    def sample_slots(self):
        raise AssertionError("a prioritized step draws no slots on the host")

    def ring_view(self):
        return "frames", 50, 16, "rows", 2, (4,), np.float32

    def _gather_device(self, leaves):
        raise AssertionError("a replay-sourced step gathers nothing")


class _StubLib:
    """Records, in call order, the rows of uniforms every entry received."""

    def __init__(self, rc_steps=0):
        self.rc_steps, self.log = rc_steps, []

    def idqn_per_learn_steps_on_replay(self, handle, per, ring, n_frames, frame_bytes, rows, n_steps, batch, stack, divisor, flags, stream):
        p = per._obj
        U = np.ctypeslib.as_array(C.cast(p.uniforms_host, C.POINTER(C.c_double)), (n_steps, batch)).copy()
        self.log.append(("steps", U, dict(ring=ring, rows=rows, n_frames=n_frames, frame_bytes=frame_bytes, stack=stack, divisor=divisor,
                                          flags=flags, leaves=p.leaves_dev, td=p.td_abs_dev, n_items=p.n_items, depth=p.depth)))
        return self.rc_steps

    def idqn_per_learn_on_replay(self, handle, per, ring, n_frames, frame_bytes, rows, batch, stack, divisor, flags, stream):
        u = np.ctypeslib.as_array(C.cast(per._obj.uniforms_host, C.POINTER(C.c_double)), (batch,)).copy()
        self.log.append(("step", u[None], None))
        return 0

    def idqn_last_error(self):
        return b"stub refusal"

    def rows(self):
        return np.concatenate([U for _, U, _ in self.log])

    def shape(self):
        return [(kind, len(U)) for kind, U, _ in self.log]


def _learner(monkeypatch, rc_steps=0):
    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent
    from slimdqn.sample_collection.per import PrioritizedLearner

    agent = DeviceAgent.__new__(DeviceAgent)
    agent._K, agent._arch, agent._handle, agent._losses, agent._obs = 3, "fc", None, "losses", (8, 1, 1)
    agent._ensure_handle = lambda batch: None
    learner = PrioritizedLearner.__new__(PrioritizedLearner)
    learner.agent, learner.rb = agent, _StubBuffer()
    sampler = type("S", (), {"__len__": lambda self: 40})()
    sampler._rng_key, sampler._alpha, sampler._max_priority_dev = np.random.default_rng(11), 0.6, _T(500)
    sampler._sum_tree = type("Tree", (), {})()
    sampler._sum_tree._nodes_dev, sampler._sum_tree._depth, sampler._sum_tree._scratch = _T(100), 7, _T(200)
    learner.sampler = sampler
    learner.beta, learner.eps, learner.reduce_max, learner.stratified = 0.4, 1e-6, 0, 1
    learner._leaves, learner._weights, learner._td_abs, learner._priorities = _T(1), _T(2), _T(3), _T(4)
    learner._steps_rows = (_T(11), _T(12), _T(13), _T(14))
    # the routes, whatever the measured defaults
    learner.fuse_per_family = dict.fromkeys(PrioritizedLearner.fuse_per_family, True)
    learner.fuse_per_steps_family = dict.fromkeys(PrioritizedLearner.fuse_per_steps_family, True)
    learner.per_steps_min = 2
    learner._step_chain = lambda u, taus=None: pytest.fail("the chain ran")
    stub = _StubLib(rc_steps)
    monkeypatch.setattr(_hip, "lib", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.setattr(_hip, "ptr", lambda t: t)
    for name in ("IDQN_LEARN_ON_REPLAY", "IDQN_PER_FUSED", "IDQN_PER_STEPS"):
        monkeypatch.delenv(name, raising=False)
    return learner, stub


@pytest.mark.parametrize("n", [1, 2, 7, 33])
def test_steps_draws_the_generator_as_n_step_calls_do(monkeypatch, n):
    from slimdqn import _hip

    one, stub_one = _learner(monkeypatch)
    for _ in range(n):
        assert one.step() == "losses"
    many, stub_many = _learner(monkeypatch)
    assert many.steps(n) == "losses"
    assert many.sampler._rng_key.bit_generator.state == one.sampler._rng_key.bit_generator.state
    want = np.random.default_rng(11).random((n, B))
    assert stub_one.rows().tobytes() == want.tobytes() == stub_many.rows().tobytes()
    assert stub_one.shape() == [("step", 1)] * n
    M = _hip.MAX_STEPS_PER_CALL
    assert stub_many.shape() == ([("step", 1)] if n == 1 else [("steps", M)] * (n // M) + ([("steps", n % M)] if n % M else []))
    if n >= 2:
        _, _, c = stub_many.log[0]
        assert (c["ring"], c["rows"], c["n_frames"], c["frame_bytes"], c["stack"], c["divisor"], c["flags"]) == ("frames", "rows", 50, 16, 2, B, 0)
        assert (c["leaves"], c["td"], c["n_items"], c["depth"]) == (11, 13, 40, 7)
        last = stub_many.log[-1][1].shape[0] - 1  # the learner's own buffers are the last step's rows
        assert (many._leaves.address, many._td_abs.address) == (11 + 1000 * (last + 1), 13 + 1000 * (last + 1))
    issued = len(stub_many.log)
    assert many.steps(0) == "losses" and len(stub_many.log) == issued  # nothing drawn, nothing issued
    assert many.sampler._rng_key.bit_generator.state == one.sampler._rng_key.bit_generator.state


def test_every_row_goes_through_exactly_one_route_in_order(monkeypatch):
    from slimdqn import _hip
    from slimdqn.sample_collection.per import PrioritizedLearner

    M = _hip.MAX_STEPS_PER_CALL
    U = np.random.default_rng(3).random((2 * M + 6, B))
    # long runs split into calls of at most MAX_STEPS_PER_CALL rows
    learner, stub = _learner(monkeypatch)
    learner.steps_with_uniforms(U)
    assert stub.shape() == [("steps", M), ("steps", M), ("steps", 6)] and stub.rows().tobytes() == U.tobytes()
    assert learner._steps_ok is True and learner.agent._replay_fc_ok is True
    # runs shorter than per_steps_min go step by step
    learner, stub = _learner(monkeypatch)
    learner.per_steps_min = 5
    learner.steps_with_uniforms(U[:4])
    learner.steps_with_uniforms(U[4:9])
    assert stub.shape() == [("step", 1)] * 4 + [("steps", 5)] and stub.rows().tobytes() == U[:9].tobytes()
    # a first refusal: the same rows one by one, and the entry is never tried again
    learner, stub = _learner(monkeypatch, rc_steps=_hip.E_INVALID)
    learner.steps_with_uniforms(U[:M + 3])
    assert stub.shape() == [("steps", M)] + [("step", 1)] * (M + 3)
    assert np.concatenate([u for k, u, _ in stub.log if k == "step"]).tobytes() == U[:M + 3].tobytes()
    assert learner._steps_ok is False and learner.steps_refusal == "stub refusal"
    learner.steps_with_uniforms(U[:3])
    assert stub.shape()[M + 4:] == [("step", 1)] * 3
    # a refusal after the entry has served, and any other error, raise
    learner, stub = _learner(monkeypatch)
    learner.steps_with_uniforms(U[:2])
    stub.rc_steps = _hip.E_INVALID
    with pytest.raises(_hip.HipExtensionError, match="idqn_per_learn_steps_on_replay"):
        learner.steps_with_uniforms(U[:2])
    learner, stub = _learner(monkeypatch, rc_steps=_hip.E_HIP)
    with pytest.raises(_hip.HipExtensionError, match="idqn_per_learn_steps_on_replay"):
        learner.steps_with_uniforms(U[:2])
    # the switches: environment, family default, the one-call step's own refusal
    for switch in ("environment", "family", "fused refused", "batch"):
        learner, stub = _learner(monkeypatch)
        if switch == "environment":
            monkeypatch.setenv("IDQN_PER_STEPS", "0")
        elif switch == "family":
            learner.fuse_per_steps_family = dict(learner.fuse_per_steps_family, fc=False)
        elif switch == "batch":
            learner.per_steps_max_batch = B - 1
        else:
            learner._fused_ok = False
            learner._step_chain = lambda u, taus=None: stub.log.append(("step", u[None].copy(), None))
        learner.steps_with_uniforms(U[:3])
        assert stub.shape() == [("step", 1)] * 3 and stub.rows().tobytes() == U[:3].tobytes(), switch
        monkeypatch.delenv("IDQN_PER_STEPS", raising=False)
    assert set(PrioritizedLearner.fuse_per_steps_family) == {"plane", "fc", "gcnn"} and PrioritizedLearner.per_steps_min >= 1
    assert 1 <= PrioritizedLearner.per_steps_max_batch <= 256


@pytest.mark.parametrize("first,n_steps,utd,T,S", [(1, 40, 1, 10, 4), (7, 25, 2, 6, 3), (3, 9, 4, 100, 50), (10, 1, 1, 10, 5), (5, 30, 3, 7, 7)])
def test_update_params_many_places_target_operations_where_the_plan_does(monkeypatch, first, n_steps, utd, T, S):
    from slimdqn.networks._agent import plan_step_runs

    def run(many):
        learner, _ = _learner(monkeypatch)
        agent, events = learner.agent, []
        agent.update_to_data, agent.target_update_frequency, agent.target_sync_frequency = utd, T, S

        def update_target_params(step):
            if step % T == 0:
                events.append(("update", step))
                return True, {"loss": float(step)}
            if step % S == 0:
                events.append(("sync", step))
            return False, {}

        agent.update_target_params = update_target_params
        learner.step = lambda: events.append(("grad", 1))
        learner.steps = lambda n: events.extend([("grad", 1)] * int(n))
        if many:
            return learner.update_params_many(first, n_steps), events
        out = []
        for s in range(first, first + n_steps):  # the loop of VectorTrainer._gradient_step
            if s % utd == 0:
                learner.step()
            updated, logs = update_target_params(s)
            if updated:
                out.append((s, logs))
        return out, events

    got, loop = run(True), run(False)
    assert got == loop
    plan = plan_step_runs(first, n_steps, utd, T, S)
    assert [e for e in got[1] if e[0] != "grad"] == [(op, last) for _, op, last in plan if op is not None]
    assert sum(1 for e in got[1] if e[0] == "grad") == sum(n for n, _, _ in plan)
