"""Host-side checks of the multi-step learner call: ``plan_step_runs`` against a brute-force simulation of the two-method loop,
``update_params_many`` and ``VectorTrainer`` on stub agents that record their calls (the sequence of sampler draws, learner
steps, target operations and log records must be the plain loop's), and the two C entries ``idqn_learn_steps_on_replay_fc`` /
``_dev`` declared, exported and bound (ABI version 4: entries were added, none changed).  No GPU needed; the device side is
``tests/test_gpu_fc_learn_steps.py``."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("idqn_learn_steps_on_replay_fc", "idqn_learn_steps_on_replay_fc_dev")


def test_entries_are_declared_exported_and_bound():
    import ctypes as C

    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    single = _hip.SYMBOLS["idqn_learn_on_replay_fc"][1]
    for name in NAMES:
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        # the single step's arguments with n_steps (int32) in front of batch
        assert _hip.SYMBOLS[name] == (C.c_int, single[:6] + [C.c_int32] + single[6:])
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
    assert re.search(r"#define\s+IDQN_MAX_STEPS_PER_CALL\s+%d\b" % _hip.MAX_STEPS_PER_CALL, header)
    assert re.search(r"#define\s+IDQN_STEPS_STAGING_DEPTH\s+%d\b" % _hip.STEPS_STAGING_DEPTH, header)
    assert _hip.MAX_STEPS_PER_CALL == 32
    assert lib.idqn_abi_version() == 4


def _loop_events(first, n, utd, tuf, tsf):
    """The two-method loop of the trainer, as events."""
    ev = []
    for s in range(first, first + n):
        if s % utd == 0:  # update_online_params
            ev.append(("grad", None))
        if s % tuf == 0:  # update_target_params
            ev.append(("update", s))
        elif tsf is not None and s % tsf == 0:
            ev.append(("sync", s))
    return ev


@pytest.mark.parametrize("utd", [1, 1.0, 2, 4])
@pytest.mark.parametrize("tuf,tsf", [(12, 5), (12, 4), (10, 5), (7, 7), (3, 1), (6, None), (1, None), (1, 1)])
def test_plan_step_runs_is_the_loop(utd, tuf, tsf):
    from slimdqn.networks._agent import plan_step_runs

    for first, n in itertools.product([0, 1, 2, 5, 11, 12, 13, 59, 60, 1000], [0, 1, 2, 3, 8, 32, 45]):
        runs = plan_step_runs(first, n, utd, tuf, tsf)
        ev, prev = [], first - 1
        for n_grad, op, last in runs:
            assert n_grad >= 0 and op in (None, "sync", "update") and prev < last < first + n
            assert n_grad == sum(1 for s in range(prev + 1, last + 1) if s % utd == 0), "a run's gradient steps are its range's"
            ev += [("grad", None)] * n_grad
            if op is not None:
                ev.append((op, last))
            prev = last
        assert ev == _loop_events(first, n, utd, tuf, tsf), (first, n, utd, tuf, tsf)
        assert all(op is not None for _, op, _ in runs[:-1]), "only the last run may end without a target operation"
        if n == 0:
            assert runs == []


class _Cum:
    def __init__(self, owner):
        self.owner = owner

    def zero_(self):
        self.owner.cum[:] = 0.0


def _stub(kind, utd=2, tuf=12, tsf=5, K=3):
    """An ``iDQN`` that never touches a device and records what the loop asks of it.  ``kind``: "many" leaves the four methods
    of the loop stock and records ``_sample_and_learn_many``; "single" has a step of its own (``_sample_and_learn``), which
    makes ``update_params_many`` the plain loop."""
    from slimdqn.networks.idqn import iDQN

    class Base(iDQN):
        def __init__(self):
            self.n_networks, self.update_to_data, self.target_update_frequency, self.target_sync_frequency = K, utd, tuf, tsf
            self.events, self.cum, self._cum = [], np.zeros(K), _Cum(self)

        def _one(self, rb):
            self.events.append(("draw", rb.draw()))
            self.events.append(("learn", sum(e[0] == "learn" for e in self.events)))
            self.cum += np.arange(1, K + 1) * 0.5

        def _local_target_update(self):
            self.events.append(("update",))

        def _local_target_sync(self):
            self.events.append(("sync",))

        def _all_cumulated_losses(self):
            return self.cum.copy()

        def __del__(self):
            pass

    if kind == "many":
        class Agent(Base):
            def _sample_and_learn_many(self, rb, n):
                self.events.append(("many", n))
                for _ in range(n):
                    self._one(rb)
    else:
        class Agent(Base):
            def _sample_and_learn(self, rb):
                self._one(rb)
    return Agent()


class _Draws:
    def __init__(self):
        self.n = 0

    def draw(self):
        self.n += 1
        return self.n


def _strip(events):
    return [e for e in events if e[0] != "many"]


@pytest.mark.parametrize("utd,tuf,tsf", [(2, 12, 5), (1, 6, 4), (1.0, 5, 5), (4, 12, 9)])
def test_update_params_many_on_stubs_is_the_loop(utd, tuf, tsf):
    many, single, loop = _stub("many", utd, tuf, tsf), _stub("single", utd, tuf, tsf), _stub("single", utd, tuf, tsf)
    rbs = [_Draws() for _ in range(3)]
    got = many.update_params_many(7, 40, rbs[0])
    plain = single.update_params_many(7, 40, rbs[1])  # a step of its own: the plain loop inside the method
    want = []
    for s in range(7, 47):
        loop.update_online_params(s, rbs[2])
        updated, logs = loop.update_target_params(s)
        if updated:
            want.append((s, logs))
    assert any(e[0] == "many" and e[1] > 1 for e in many.events), "the stock agent did not batch its gradient steps"
    assert not any(e[0] == "many" for e in single.events)
    assert _strip(many.events) == loop.events == single.events
    assert got == want == plain and len(want) >= 3
    assert rbs[0].n == rbs[1].n == rbs[2].n
    assert many.update_params_many(50, 0, rbs[0]) == [] and rbs[0].n == rbs[2].n


class _Log:
    def __init__(self):
        self.records = []

    def log(self, d):
        self.records.append(dict(d))


def _trainer(agent, fuse, n_envs=4):
    from experiments.base.dqn import VectorTrainer

    class T(VectorTrainer):
        def _environment_step(self, active):
            self.vsteps = getattr(self, "vsteps", 0) + 1
            return [1.0] * n_envs, [self.vsteps % (3 + i) == 0 for i in range(n_envs)]

    p = {"epsilon_end": 0.1, "epsilon_duration": 10, "n_training_steps_per_epoch": 30, "n_initial_samples": 9, "n_epochs": 2,
         "wandb": _Log()}
    if fuse is not None:
        p["fuse_gradient_steps"] = fuse

    class Env:
        def reset(self):
            pass

    t = T(0, p, agent, [Env() for _ in range(n_envs)], _Draws())
    return t, t.run()


def test_vector_trainer_on_stubs():
    fused, plain = _stub("many"), _stub("single")
    (tf, out_f), (tp, out_p) = _trainer(fused, None), _trainer(plain, False)
    assert any(e[0] == "many" for e in fused.events) and not any(e[0] == "many" for e in plain.events)
    assert _strip(fused.events) == plain.events and len(plain.events) > 20
    assert out_f == out_p and tf.total_steps == tp.total_steps and tf.rb.n == tp.rb.n
    assert tf.p["wandb"].records == tp.p["wandb"].records
    assert sum("loss" in r for r in tp.p["wandb"].records) >= 3

    class NoMany:  # an agent without the method takes today's loop
        def __init__(self):
            self.calls = []

        def update_online_params(self, step, rb):
            self.calls.append(("online", step))

        def update_target_params(self, step):
            self.calls.append(("target", step))
            return step % 10 == 0, {"loss": float(step)}

        def get_model(self):
            return {}

    a = NoMany()
    t, _ = _trainer(a, None)
    steps = list(range(10, t.total_steps + 1))
    assert a.calls == [c for s in steps for c in (("online", s), ("target", s))]
    assert [r["n_training_steps"] for r in t.p["wandb"].records if "loss" in r] == [s for s in steps if s % 10 == 0]
