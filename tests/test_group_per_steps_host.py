"""Host logic of the n-step prioritized seed groups (no GPU): the entry is declared, exported and bound and the ctypes records
match the header; ``PrioritizedGroupLearner.steps`` draws n ``random(B)`` per member, member by member, chunks at 32 steps, falls
back to the single steps on the rows already drawn after a first refusal and routes by ``group_per_steps_sizes``,
``group_per_steps_min`` and ``IDQN_PER_STEPS``; ``update_params_many`` plans once on the shared schedule; ``SeedVectorTrainer``
takes ``learner=``.  The device is a stub: a fake library records the group calls.  On the parent commit the symbol and the
methods do not exist."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_group_per_learn_steps_on_replay_fc"


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert NAME in _hip.SYMBOLS, f"{NAME} is not bound in slimdqn/_hip.py"
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), f"{NAME} is not declared in include/idqn_hip.h"
    plain = _hip.SYMBOLS["idqn_group_learn_steps_on_replay_fc"][1]
    assert _hip.SYMBOLS[NAME][1] == plain[:2] + [C.POINTER(_hip.PerSteps)] + plain[3:], "the plain n-step group call with per[S] for the slots"
    if os.path.exists(_hip.LIB_PATH):
        nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
        exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                                  capture_output=True, text=True).stdout
        assert re.search(r"\sT\s+" + NAME + r"$", exported, re.M), f"{NAME} is not exported by the library"
        lib = _hip.lib()
        assert getattr(lib, NAME).argtypes == _hip.SYMBOLS[NAME][1]
        assert lib.idqn_abi_version() == 4  # an entry added only


def test_ctypes_records_match_the_header(tmp_path):
    """sizeof and the offset of the last field of ``idqn_per_steps_t`` / ``idqn_per_step_t`` / ``idqn_group_ring_t`` as the C
    compiler lays them out, against the ctypes structures."""
    import shutil

    from slimdqn import _hip

    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "idqn_hip.h"\nint main() { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(idqn_per_steps_t), offsetof(idqn_per_steps_t, tree_scratch_dev), sizeof(idqn_per_step_t), "
                   "offsetof(idqn_per_step_t, tau_dev), sizeof(idqn_group_ring_t), offsetof(idqn_group_ring_t, stack)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cc, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_hip.PerSteps), _hip.PerSteps.tree_scratch_dev.offset, C.sizeof(_hip.PerStep), _hip.PerStep.tau_dev.offset,
            C.sizeof(_hip.GroupRing), _hip.GroupRing.stack.offset]
    assert got == want
    assert [f for f, _ in _hip.PerSteps._fields_] == [f for f, _ in _hip.PerStep._fields_[:-1]]


# ---- stubs -----------------------------------------------------------------------------------------------------------
class _T:
    """Stands in for a device tensor (and for a row of one)."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def __getitem__(self, i):
        return _T(self.address + 100000 * (i + 1))


class _Ring:
    add_count = 100

    def __init__(self, g, B):
        self.g, self._batch_size = g, B

    def sample_slots(self):
        raise AssertionError("a prioritized step draws no slots on the host")

    def ring_view(self):
        return (_T(16 * self.g + 16), 64, 32, _T(8), 1, (8,), np.float32)


class _FakeLib:
    """Records the group calls; ``refuse`` names what answers IDQN_E_INVALID."""

    def __init__(self, log, refuse=()):
        self.log, self.refuse = log, set(refuse)

    def idqn_group_create(self, arr, n, out):
        if "create" in self.refuse:
            return -1
        out._obj.value = 77
        self.log.append(("create", [arr[i] for i in range(n)]))
        return 0

    def idqn_group_destroy(self, g):
        return 0

    def idqn_group_per_learn_on_replay_fc(self, g, rings, per, B, div, flags, stream):
        us = [np.ctypeslib.as_array(C.cast(p.uniforms_host, C.POINTER(C.c_double)), (B,)).copy() for p in per]
        self.log.append(("group_per", us, [p.leaves_dev for p in per]))
        return 0

    def idqn_group_per_learn_steps_on_replay_fc(self, g, rings, per, n, B, div, flags, stream):
        Us = [np.ctypeslib.as_array(C.cast(p.uniforms_host, C.POINTER(C.c_double)), (n, B)).copy() for p in per]
        self.log.append(("group_per_steps", Us, [r.frames_dev for r in rings],
                         [(p.leaves_dev, p.weights_dev, p.td_abs_dev, p.priorities_dev, p.n_items, p.depth, p.beta) for p in per], n, B, div, flags))
        return -1 if "steps" in self.refuse else 0

    def idqn_last_error(self):
        return b"stub refusal"


def _make(monkeypatch, S, B=4, refuse=()):
    """A ``PrioritizedGroupLearner`` over S stub members; ``log`` takes the library's and the members' calls."""
    from slimdqn import _hip
    from slimdqn.networks._agent import DeviceAgent
    from slimdqn.networks.group import AgentGroup
    from slimdqn.sample_collection.per import PrioritizedGroupLearner, PrioritizedLearner

    log = []
    agents, learners = [], []
    for g in range(S):
        a = DeviceAgent.__new__(DeviceAgent)
        a._K, a._arch, a._obs, a._handle, a._losses = 3, "fc", (8, 1, 1), C.c_void_p(500 + g), f"losses {g}"
        a._ensure_handle = lambda batch: None
        a.update_to_data, a.target_update_frequency, a.target_sync_frequency = 1, 4, 3
        a.update_target_params = lambda step, g=g: log.append(("target", g, step)) or (step % 4 == 0, {"loss": g})
        agents.append(a)
        lr = PrioritizedLearner.__new__(PrioritizedLearner)
        lr.agent, lr.rb = a, _Ring(g, B)
        sampler = type("S", (), {"__len__": lambda self, g=g: 40 + g})()
        sampler._rng_key, sampler._alpha, sampler._max_priority_dev = np.random.default_rng(11 + g), 0.6, _T(5000 + g)
        sampler._sum_tree = type("Tree", (), {})()
        sampler._sum_tree._nodes_dev, sampler._sum_tree._depth, sampler._sum_tree._scratch = _T(1000 + g), 7, _T(2000 + g)
        lr.sampler = sampler
        lr.beta, lr.eps, lr.reduce_max, lr.stratified = 0.4 + 0.1 * g, 1e-6, 0, 1
        lr._leaves, lr._weights, lr._td_abs, lr._priorities = _T(10 + g), _T(20 + g), _T(30 + g), _T(40 + g)
        lr._steps_rows = (_T(110 + g), _T(120 + g), _T(130 + g), _T(140 + g))
        lr.step_with_uniforms = lambda u, g=g: log.append(("member", g, u.copy())) or f"member losses {g}"
        lr.update_params_many = lambda first, n, g=g: log.append(("member_many", g, first, n)) or [(first, {"member": g})]
        learners.append(lr)
    gl = PrioritizedGroupLearner.__new__(PrioritizedGroupLearner)
    gl.group, gl.rbs, gl.learners = AgentGroup(agents), [lr.rb for lr in learners], learners
    gl.group_per_sizes = gl.group_per_steps_sizes = frozenset({S})  # the routes, whatever the measured defaults
    gl.group_per_steps_min = 2
    lib = _FakeLib(log, refuse)
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    for name in ("IDQN_LEARN_ON_REPLAY", "IDQN_PER_FUSED", "IDQN_PER_STEPS"):
        monkeypatch.delenv(name, raising=False)
    return gl, log


def _expected_draws(S, B, n):
    """[member]: [n][B], what each member's generator gives when it is drawn ``random(B)`` n times."""
    return [np.stack([r.random(B) for _ in range(n)]) for r in (np.random.default_rng(11 + g) for g in range(S))]


def _kinds(log):
    return [e[0] for e in log if e[0] in ("group_per_steps", "group_per", "member")]


def test_draw_order_counts_and_the_records(monkeypatch):
    gl, log = _make(monkeypatch, 3)
    order = []
    for g, lr in enumerate(gl.learners):
        real = lr.sampler._rng_key

        class Counting:
            def random(self, n, g=g, real=real):
                order.append((g, n))
                return real.random(n)

        lr.sampler._rng_key = Counting()
    out = gl.steps(5)
    assert order == [(g, 4) for g in range(3) for _ in range(5)], "n draws of random(B) per member, member by member"
    calls = [e for e in log if e[0] == "group_per_steps"]
    assert len(calls) == 1 and _kinds(log) == ["group_per_steps"]
    e, want = calls[0], _expected_draws(3, 4, 5)
    assert all(np.array_equal(a, b) for a, b in zip(e[1], want))
    assert e[2] == [16, 32, 48], "every member's own ring"
    assert e[3] == [(110 + g, 120 + g, 130 + g, 140 + g, 40 + g, 7, 0.4 + 0.1 * g) for g in range(3)], "every member's own row buffers and tree"
    assert e[4:] == (5, 4, 4, 0)
    assert out == ["losses 0", "losses 1", "losses 2"] and gl._group_per_steps_ok is True
    for g, lr in enumerate(gl.learners):  # the learners' own buffers: the last step's rows
        assert [t.data_ptr() for t in (lr._leaves, lr._weights, lr._td_abs, lr._priorities)] == [b + g + 100000 * 5 for b in (110, 120, 130, 140)]
    assert gl.steps(0) == ["losses 0", "losses 1", "losses 2"] and len(order) == 15, "no steps, no draws"


def test_chunks_of_32(monkeypatch):
    gl, log = _make(monkeypatch, 2)
    gl.steps(70)
    calls = [e for e in log if e[0] == "group_per_steps"]
    assert [e[4] for e in calls] == [32, 32, 6] and _kinds(log) == ["group_per_steps"] * 3
    want = _expected_draws(2, 4, 70)
    for g in range(2):
        assert np.array_equal(np.concatenate([e[1][g] for e in calls]), want[g]), "every row once, in order"


@pytest.mark.parametrize("refuse", ["steps", "create"])
def test_a_first_refusal_reuses_the_drawn_rows_and_sticks(monkeypatch, refuse):
    gl, log = _make(monkeypatch, 2, refuse=[refuse])
    gl.steps(3)
    gl.steps(2)
    want = _expected_draws(2, 4, 5)
    tried = [e for e in log if e[0] == "group_per_steps"]
    assert len(tried) == (1 if refuse == "steps" else 0), "never retried"
    assert gl._group_per_steps_ok is False
    if refuse == "steps":
        assert gl.group_per_steps_refusal == "stub refusal"
        singles = [e for e in log if e[0] == "group_per"]  # the single group call serves the rows
        assert len(singles) == 5 and not any(e[0] == "member" for e in log)
        for i, e in enumerate(singles):
            assert all(np.array_equal(e[1][g], want[g][i]) for g in range(2)), "a refusal costs no draw"
    else:  # no group at all: the members' own steps
        members = [e for e in log if e[0] == "member"]
        assert [e[1] for e in members] == [0, 1] * 5
        for i in range(5):
            assert all(np.array_equal(members[2 * i + g][2], want[g][i]) for g in range(2))


def test_a_later_refusal_raises(monkeypatch):
    from slimdqn import _hip

    gl, log = _make(monkeypatch, 2)
    gl.steps(2)
    _hip.lib().refuse.add("steps")
    with pytest.raises(_hip.HipExtensionError):
        gl.steps(2)


def test_size_minimum_and_environment_gates(monkeypatch):
    from slimdqn.sample_collection.per import PrioritizedGroupLearner

    gl, log = _make(monkeypatch, 2)
    gl.group_per_steps_sizes = frozenset({3, 4})  # a size that is not on: the single group steps
    gl.steps(3)
    assert _kinds(log) == ["group_per"] * 3
    gl, log = _make(monkeypatch, 2)
    gl.group_per_steps_min = 4  # a run below the minimum
    gl.steps(3)
    gl.steps(4)
    assert _kinds(log) == ["group_per"] * 3 + ["group_per_steps"]
    gl, log = _make(monkeypatch, 2)
    monkeypatch.setenv("IDQN_PER_STEPS", "0")
    gl.steps(3)
    assert _kinds(log) == ["group_per"] * 3 and gl.__dict__.get("_group_per_steps_ok") is None
    monkeypatch.delenv("IDQN_PER_STEPS")
    gl, log = _make(monkeypatch, 2)
    monkeypatch.setenv("IDQN_PER_FUSED", "0")  # _group_route's own conditions hold for the n-step call too
    gl.steps(2)
    assert _kinds(log) == ["member"] * 4
    monkeypatch.delenv("IDQN_PER_FUSED")
    gl, log = _make(monkeypatch, 2, B=33)
    gl.steps(2)
    assert _kinds(log) == ["member"] * 4
    gl, log = _make(monkeypatch, 2)
    gl.group.agents[1]._arch = "cnn"
    gl.steps(2)
    assert _kinds(log) == ["member"] * 4
    assert isinstance(PrioritizedGroupLearner.group_per_steps_sizes, frozenset)
    assert all(2 <= s <= 32 for s in PrioritizedGroupLearner.group_per_steps_sizes) and PrioritizedGroupLearner.group_per_steps_min >= 1


def test_update_params_many_plans_once_on_the_shared_schedule(monkeypatch):
    gl, log = _make(monkeypatch, 2)
    out = gl.update_params_many(1, 9)  # target update every 4, sync every 3: runs end at 3, 4, 6, 8, 9
    steps = [e[4] for e in log if e[0] == "group_per_steps"]
    assert sum(steps) + sum(1 for e in log if e[0] == "group_per") == 9
    targets = [e for e in log if e[0] == "target"]
    assert [t[1] for t in targets] == [0, 1] * (len(targets) // 2), "the members' own target operations, in member order"
    assert out == [[(4, {"loss": 0}), (8, {"loss": 0})], [(4, {"loss": 1}), (8, {"loss": 1})]]
    assert not any(e[0] == "member_many" for e in log)
    gl, log = _make(monkeypatch, 2)
    gl.group.agents[1].target_update_frequency = 5  # schedules differ: every member learner's own loop
    assert gl.update_params_many(3, 4) == [[(3, {"member": 0})], [(3, {"member": 1})]]
    assert [e for e in log if e[0] != "create"] == [("member_many", 0, 3, 4), ("member_many", 1, 3, 4)]


# ---- SeedVectorTrainer ---------------------------------------------------------------------------------------------------
class _Env:
    n_actions = 4

    def __init__(self, seed):
        self.length, self.n_steps = 4 + seed, 0
        self.state = self.observation = np.zeros(2, np.float32)

    def reset(self):
        self.n_steps = 0

    def step(self, action):
        self.n_steps += 1
        return 0.5, self.n_steps >= self.length


class _Log:
    def __init__(self):
        self.records = []

    def log(self, d):
        self.records.append(d)


class _Agent:
    update_to_data = 1

    def __init__(self, seed, calls):
        self.seed, self.calls, self.params = seed, calls, object()

    def update_online_params(self, step, rb):
        self.calls.append(("online", self.seed, step))

    def update_target_params(self, step):
        return False, {}

    def update_params_many(self, first, n, rb):
        self.calls.append(("agent_many", self.seed, first, n))
        return []

    def get_model(self):
        return {}


class _StubGroup:
    def __init__(self, agents, calls):
        self.agents, self.calls = agents, calls

    def _stock(self):
        return True

    def select_heads(self, keys, members):
        return [0 for _ in members]

    def best_actions(self, which, heads, states, members):
        return np.zeros(len(members), np.int64)

    def update_params_many(self, first, n, rbs):
        self.calls.append(("group_many", first, n))
        return [[] for _ in self.agents]

    def close(self):
        pass


class _StubCollector:
    def add_many(self, entries, live):
        pass


class _StubLearner:
    def __init__(self, S, calls):
        self.calls = calls
        mk = lambda i: type("L", (), {"step": lambda self: calls.append(("learner_member_step", i)),
                                      "update_params_many": lambda self, first, n: calls.append(("learner_member", i, first, n)) or [(first, {"m": i})]})()
        self.learners = [mk(i) for i in range(S)]

    def update_params_many(self, first, n):
        self.calls.append(("learner", first, n))
        return [[(first, {"g": i})] for i in range(len(self.learners))]


def _train(initial, with_learner, fuse=True):
    from experiments.base.seeds import SeedVectorTrainer
    from slimdqn import prng

    calls, S, E = [], len(initial), 2
    ps = [{"seed": s, "epsilon_end": 0.1, "epsilon_duration": 30, "n_training_steps_per_epoch": 12, "n_initial_samples": n, "n_epochs": 1,
           "horizon": 7, "wandb": _Log(), "fuse_gradient_steps": fuse} for s, n in enumerate(initial)]
    agents = [_Agent(s, calls) for s in range(S)]
    rbs = [type("Rb", (), {"_clipping": None})() for _ in range(S)]
    kw = {"learner": _StubLearner(S, calls)} if with_learner else {}
    t = SeedVectorTrainer([prng.PRNGKey(s) for s in range(S)], ps, agents, [[_Env(s) for _ in range(E)] for s in range(S)], rbs,
                          group=_StubGroup(agents, calls), collector=_StubCollector(), **kw)
    t.run()
    return t, calls, ps


def test_seed_vector_trainer_sends_shared_runs_to_the_learner(capsys):
    t, calls, ps = _train([4, 8], True)
    assert not any(c[0] in ("online", "agent_many", "group_many") for c in calls), "the learner replaces the agents' gradient steps"
    # seed 0 learns from step 5 on, seed 1 from step 9 on: until then seed 0's own learner, then one learner call per vector step
    first_group = next(i for i, c in enumerate(calls) if c[0] == "learner")
    assert calls[:first_group] == [("learner_member", 0, 5, 2), ("learner_member", 0, 7, 2)]
    assert calls[first_group] == ("learner", 9, 2)
    assert all(c[0] in ("learner", "learner_member") for c in calls)
    # the logs of a run reach the seeds' own loggers
    assert {"n_training_steps": 9, "g": 1} in ps[1]["wandb"].records and {"n_training_steps": 5, "m": 0} in ps[0]["wandb"].records
    # seed 1's episodes are longer: it outlives seed 0 and learns alone at the end
    assert calls[-1][0] == "learner_member" and calls[-1][1] == 1


def test_seed_vector_trainer_non_fused_path_steps_the_members_learners(capsys):
    t, calls, _ = _train([4, 4], True, fuse=False)
    assert calls and all(c[0] == "learner_member_step" for c in calls)
    assert calls[:4] == [("learner_member_step", 0)] * 2 + [("learner_member_step", 1)] * 2, "E = 2 steps per seed per vector step"


def test_seed_vector_trainer_without_a_learner_makes_the_parents_calls(capsys):
    t, calls, _ = _train([4, 8], False)
    assert t.learner is None and not any(c[0].startswith("learner") for c in calls)
    assert calls[:3] == [("agent_many", 0, 5, 2), ("agent_many", 0, 7, 2), ("group_many", 9, 2)]


def test_train_seeds_vector_passes_the_learner_and_its_group(monkeypatch):
    from experiments.base import seeds

    seen = {}

    class Fake:
        def __init__(self, *a, **kw):
            seen.update(kw)

        def run(self):
            return "ran"

    monkeypatch.setattr(seeds, "SeedVectorTrainer", Fake)
    learner = type("GL", (), {"group": "the group"})()
    assert seeds.train_seeds_vector([], [], [], [], [], learner=learner) == "ran"
    assert seen["learner"] is learner and seen["group"] == "the group"
    seen.clear()
    seeds.train_seeds_vector([], [], [], [], [])
    assert seen["learner"] is None and seen["group"] is None
