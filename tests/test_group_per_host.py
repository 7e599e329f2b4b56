"""Host logic of the prioritized seed groups (no GPU): the entry is declared, exported and bound; ``PrioritizedGroupLearner``
draws one ``random(B)`` per member per step in member order on both routes, falls back to the members on the uniforms already
drawn after a refusal and routes by ``group_per_sizes``, the batch size and the members; ``SeedTrainer`` takes ``learner=``.
The device is a stub: a fake library records the group calls.  On the parent commit the symbol and the class do not exist."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_group_per_learn_on_replay_fc"


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert NAME in _hip.SYMBOLS, f"{NAME} is not bound in slimdqn/_hip.py"
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), f"{NAME} is not declared in include/idqn_hip.h"
    plain = _hip.SYMBOLS["idqn_group_learn_on_replay_fc"][1]
    assert _hip.SYMBOLS[NAME][1] == plain[:2] + [C.POINTER(_hip.PerStep)] + plain[3:], "the plain group step with per[S] for the slots"
    if os.path.exists(_hip.LIB_PATH):
        nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
        exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                                  capture_output=True, text=True).stdout
        assert re.search(r"\sT\s+" + NAME + r"$", exported, re.M), f"{NAME} is not exported by the library"
        lib = _hip.lib()
        assert getattr(lib, NAME).argtypes == _hip.SYMBOLS[NAME][1]
        assert lib.idqn_abi_version() == 4  # an entry added only


# ---- stubs -----------------------------------------------------------------------------------------------------------
class _T:
    """Stands in for a device tensor."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


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
        self.log.append(("group_per", us, [r.frames_dev for r in rings], [(p.leaves_dev, p.n_items, p.depth, p.beta, p.tau_dev) for p in per], B, div, flags))
        return -1 if "per" in self.refuse else 0

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
        lr.step_with_uniforms = lambda u, g=g: log.append(("member", g, u.copy())) or f"member losses {g}"
        learners.append(lr)
    gl = PrioritizedGroupLearner.__new__(PrioritizedGroupLearner)
    gl.group, gl.rbs, gl.learners = AgentGroup(agents), [lr.rb for lr in learners], learners
    gl.group_per_sizes = frozenset({S})  # the routes, whatever the measured default
    lib = _FakeLib(log, refuse)
    monkeypatch.setattr(_hip, "lib", lambda: lib)
    monkeypatch.setattr(_hip, "current_stream", lambda: None)
    monkeypatch.delenv("IDQN_LEARN_ON_REPLAY", raising=False)
    monkeypatch.delenv("IDQN_PER_FUSED", raising=False)
    return gl, log


def _expected_draws(S, B, steps):
    """[step][member]: what each member's generator gives when it is drawn ``random(B)`` once per step."""
    rngs = [np.random.default_rng(11 + g) for g in range(S)]
    return [[r.random(B) for r in rngs] for _ in range(steps)]


def _same_draws(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("route", ["group", "members"])
def test_one_draw_per_member_per_step_in_member_order(monkeypatch, route):
    gl, log = _make(monkeypatch, 3)
    if route == "members":
        monkeypatch.setenv("IDQN_PER_FUSED", "0")
    order = []
    for g, lr in enumerate(gl.learners):
        real = lr.sampler._rng_key

        class Counting:
            def random(self, n, g=g, real=real):
                order.append((g, n))
                return real.random(n)

        lr.sampler._rng_key = Counting()
    out = [gl.step() for _ in range(3)]
    assert order == [(g, 4) for _ in range(3) for g in range(3)], "one random(B) per member per step, in member order"
    want = _expected_draws(3, 4, 3)
    if route == "group":
        calls = [e for e in log if e[0] == "group_per"]
        assert len(calls) == 3 and not any(e[0] == "member" for e in log)
        for e, w in zip(calls, want):
            assert _same_draws(e[1], w)
            assert e[2] == [16, 32, 48], "every member's own ring"
            assert e[3] == [(10 + g, 40 + g, 7, 0.4 + 0.1 * g, None) for g in range(3)], "every member's own tree record"
            assert e[4:] == (4, 4, 0)
        assert [e for e in log if e[0] == "create"] == [("create", [500, 501, 502])], "one group, made once"
        assert out[0] == ["losses 0", "losses 1", "losses 2"] and gl._group_per_ok is True
    else:
        assert not any(e[0] in ("group_per", "create") for e in log)
        for step, w in enumerate(want):
            got = [e for e in log if e[0] == "member"][3 * step : 3 * step + 3]
            assert [e[1] for e in got] == [0, 1, 2] and _same_draws([e[2] for e in got], w)
        assert out[0] == ["member losses 0", "member losses 1", "member losses 2"] and gl.__dict__.get("_group_per_ok") is None


@pytest.mark.parametrize("refuse", ["per", "create"])
def test_a_first_refusal_reaches_the_members_with_the_same_uniforms_and_sticks(monkeypatch, refuse):
    gl, log = _make(monkeypatch, 2, refuse=[refuse])
    gl.step()
    gl.step()
    want = _expected_draws(2, 4, 2)
    tried = [e for e in log if e[0] == "group_per"]
    assert len(tried) == (1 if refuse == "per" else 0), "never retried"
    if refuse == "per":
        assert _same_draws(tried[0][1], want[0]) and gl.group_per_refusal == "stub refusal"
    members = [e for e in log if e[0] == "member"]
    assert [e[1] for e in members] == [0, 1, 0, 1]
    assert _same_draws([e[2] for e in members], want[0] + want[1]), "a refusal costs no draw"
    assert gl._group_per_ok is False


def test_a_later_refusal_raises(monkeypatch):
    from slimdqn import _hip

    gl, log = _make(monkeypatch, 2)
    gl.step()
    _hip.lib().refuse.add("per")
    with pytest.raises(_hip.HipExtensionError):
        gl.step()


def test_routing_by_size_batch_and_members(monkeypatch):
    from slimdqn.sample_collection.per import PrioritizedGroupLearner

    route = lambda log: [e[0] for e in log if e[0] in ("group_per", "member")]
    gl, log = _make(monkeypatch, 2)
    gl.group_per_sizes = frozenset({3, 4})  # a size that is not shipped
    gl.step()
    assert route(log) == ["member", "member"]
    gl, log = _make(monkeypatch, 2, B=33)  # B > 32
    gl.step()
    assert route(log) == ["member", "member"]
    gl, log = _make(monkeypatch, 2, B=32)
    gl.step()
    assert route(log) == ["group_per"]
    gl, log = _make(monkeypatch, 2)  # a member that is not stock: another architecture
    gl.group.agents[1]._arch = "cnn"
    gl.step()
    assert route(log) == ["member", "member"]
    gl, log = _make(monkeypatch, 2)  # a member whose ring does not serve the replay-sourced step
    gl.rbs[1].ring_view = lambda: (_T(1), 64, 32, _T(8), 1, (8,), np.uint8)
    gl.step()
    assert route(log) == ["member", "member"]
    gl, log = _make(monkeypatch, 2)  # the agent-side switch
    monkeypatch.setenv("IDQN_LEARN_ON_REPLAY", "0")
    gl.step()
    assert route(log) == ["member", "member"]
    assert isinstance(PrioritizedGroupLearner.group_per_sizes, frozenset)
    assert all(2 <= s <= 32 for s in PrioritizedGroupLearner.group_per_sizes), "S = 1 has nothing to group"


# ---- SeedTrainer ---------------------------------------------------------------------------------------------------------
class _Env:
    n_actions = 4

    def __init__(self, seed):
        self.length, self.t, self.n_steps = 5 + seed, 0, 0
        self.state = self.observation = np.zeros(2, np.float32)

    def reset(self):
        self.n_steps = 0

    def step(self, action):
        self.t += 1
        self.n_steps += 1
        return 0.5, self.n_steps >= self.length


class _Rb:
    _clipping = None

    def add(self, tr):
        pass


class _Log:
    def log(self, d):
        pass


class _Agent:
    def __init__(self, seed, calls):
        self.seed, self.n_networks, self.calls, self.params, self.update_to_data = seed, 3, calls, object(), 1

    def update_online_params(self, step, rb):
        self.calls.append(("online", self.seed, step))

    def update_target_params(self, step):
        self.calls.append(("target", self.seed, step))
        return False, {}

    def get_model(self):
        return {}


class _StubGroup:
    def __init__(self, agents, calls):
        self.agents, self.calls = agents, calls

    def select_heads(self, keys, members):
        return [0 for _ in members]

    def best_actions(self, which, heads, states, members):
        return np.zeros(len(members), np.int64)

    def update_online_params(self, step, rbs):
        self.calls.append(("group_online", step))

    def update_target_params(self, step):
        return [a.update_target_params(step) for a in self.agents]

    def close(self):
        pass


class _StubLearner:
    def __init__(self, S, calls):
        self.calls = calls
        self.learners = [type("L", (), {"step": lambda self, i=i: calls.append(("learner_member", i))})() for i in range(S)]

    def step(self):
        self.calls.append(("learner",))


def _train(initial, with_learner):
    from experiments.base.seeds import SeedTrainer
    from slimdqn import prng

    calls = []
    ps = [{"seed": s, "epsilon_end": 0.1, "epsilon_duration": 30, "n_training_steps_per_epoch": 12, "n_initial_samples": n,
           "n_epochs": 1, "horizon": 7, "wandb": _Log()} for s, n in enumerate(initial)]
    agents = [_Agent(s, calls) for s in range(len(initial))]
    kw = {"learner": _StubLearner(len(initial), calls)} if with_learner else {}
    st = SeedTrainer([prng.PRNGKey(s) for s in range(len(initial))], ps, agents, [_Env(s) for s in range(len(initial))],
                     [_Rb() for _ in initial], group=_StubGroup(agents, calls), **kw)
    st.run()
    return st, calls


def test_seed_trainer_calls_the_learner_exactly_when_all_seeds_learn(capsys):
    st, calls = _train([3, 6], True)
    # seed 0 learns from step 4 on, seed 1 from step 7 on; both are live while both learn
    assert not any(c[0] in ("online", "group_online") for c in calls), "the learner replaces update_online_params"
    firsts = [c for c in calls if c[0] in ("learner", "learner_member")]
    assert firsts[:3] == [("learner_member", 0)] * 3, "steps 4..6: seed 0 learns alone, through its own learner"
    assert firsts[3] == ("learner",), "step 7: all seeds learn, one group call"
    # from the first group call on: one learner call per step while both seeds are live, never a member call beside it
    i = calls.index(("learner",))
    both = [c for c in calls[i:] if c[0] != "target"]
    n_group = sum(1 for c in both if c == ("learner",))
    assert n_group >= 1 and all(c in (("learner",), ("learner_member", 0), ("learner_member", 1)) for c in both)
    targets = [c for c in calls if c[0] == "target"]
    group_steps = {c[2] for c in targets if sum(1 for d in targets if d[2] == c[2]) == 2 and c[2] > 6}
    assert n_group == len(group_steps), "exactly the steps at which every seed learned"


def test_seed_trainer_honours_update_to_data_with_a_learner(capsys):
    from experiments.base.seeds import SeedTrainer

    calls = []
    st = SeedTrainer.__new__(SeedTrainer)
    agents = [_Agent(s, calls) for s in range(2)]
    agents[1].update_to_data = 2
    st.seeds = [type("Seed", (), {"agent": a})() for a in agents]
    st.learner = _StubLearner(2, calls)
    for st.total_steps in (4, 5):
        st._prioritized_steps([0, 1])
    assert calls == [("learner",), ("learner_member", 0)]


def test_seed_trainer_without_a_learner_makes_the_parents_calls(capsys):
    st, calls = _train([3, 6], False)
    assert st.learner is None
    assert not any(c[0] in ("learner", "learner_member") for c in calls)
    # the parent's sequence: the seeds that learn alone call their agents, a step at which all learn is one group call
    assert calls[:6] == [("online", 0, 4), ("target", 0, 4), ("online", 0, 5), ("target", 0, 5), ("online", 0, 6), ("target", 0, 6)]
    assert calls[6:9] == [("group_online", 7), ("target", 0, 7), ("target", 1, 7)]
    assert sum(1 for c in calls if c[0] == "group_online") >= 1
