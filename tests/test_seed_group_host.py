"""Host logic of the seed groups (no GPU): the five entries are declared, exported and bound; ``AgentGroup`` draws every member's
keys as the member alone would, cuts runs as ``plan_step_runs`` does and falls back to the members after a refusal;
``SeedTrainer`` is ``Trainer`` per seed.  The device is a stub: a fake library records the group calls."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["idqn_group_create", "idqn_group_destroy", "idqn_group_learn_on_replay_fc", "idqn_group_learn_steps_on_replay_fc",
         "idqn_group_act_host_fc"]


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
    assert lib.idqn_abi_version() == 4  # entries added only
    # idqn_group_ring_t as the header lays it out
    assert C.sizeof(_hip.GroupRing) == 40 and _hip.GroupRing.rows_dev.offset == 24 and _hip.GroupRing.stack.offset == 32
    # the steps entry is the single one with n_steps (int32) in front of batch
    single = _hip.SYMBOLS["idqn_group_learn_on_replay_fc"][1]
    assert _hip.SYMBOLS["idqn_group_learn_steps_on_replay_fc"][1] == single[:3] + [C.c_int32] + single[3:]


# ---- stubs -----------------------------------------------------------------------------------------------------------
class _Ptr:
    def __init__(self, v):
        self.v = v

    def data_ptr(self):
        return self.v


class _Ring:
    """A buffer whose draws are a counter: draw i of buffer g is [1000 g + i] * B."""

    def __init__(self, g, B=4):
        self.g, self.B, self.n, self._batch_size = g, B, 0, B

    def sample_slots(self):
        self.n += 1
        return np.full(self.B, 1000 * self.g + self.n, np.int64)

    def ring_view(self):
        return (_Ptr(16 * self.g + 16), 64, 32, _Ptr(8), 1, (8,), np.float32)

    def _gather(self, slots):
        return ("gathered", slots.copy())


class _FakeLib:
    """Records the group calls; ``refuse`` names the entries that answer IDQN_E_INVALID."""

    def __init__(self, log, refuse=()):
        self.log, self.refuse = log, set(refuse)

    def idqn_group_create(self, arr, n, out):
        if "create" in self.refuse:
            return -1
        out._obj.value = 77
        self.log.append(("create", [arr[i] for i in range(n)]))
        return 0

    def idqn_group_destroy(self, g):
        self.log.append(("destroy",))
        return 0

    def _slots(self, ptr, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (n,)).reshape(shape).copy()

    def idqn_group_learn_on_replay_fc(self, g, rings, slots, B, div, flags, stream):
        if "learn" in self.refuse:
            return -1
        S = len(rings)
        self.log.append(("group", self._slots(slots, (S, B))[:, 0].tolist(), [r.frames_dev for r in rings]))
        return 0

    def idqn_group_learn_steps_on_replay_fc(self, g, rings, slots, n, B, div, flags, stream):
        if "steps" in self.refuse:
            return -1
        self.log.append(("group_steps", n, self._slots(slots, (len(rings), n, B))[:, :, 0].tolist()))
        return 0

    def idqn_last_error(self):
        return b"stub"


def _make(S, log, utd=1, tuf=12, tsf=5, K=3):
    from slimdqn.networks.idqn import iDQN

    class Agent(iDQN):
        def __init__(self, g):
            self.g, self.n_networks, self.update_to_data, self.target_update_frequency, self.target_sync_frequency = g, K, utd, tuf, tsf
            self._arch, self._obs, self._handle, self.cum = "fc", (8, 1, 1), C.c_void_p(500 + g), np.zeros(K)

        def _ensure_handle(self, batch):
            pass

        def _learn_on_replay_fc(self, rb, view, slots=None, slots_dev=None, gather=None):
            log.append(("solo", self.g, int(slots[0])))

        def _local_target_update(self):
            log.append(("update", self.g))

        def _local_target_sync(self):
            log.append(("sync", self.g))

        def _all_cumulated_losses(self):
            return self.cum.copy()

        @property
        def _cum(self):
            class Z:
                def zero_(s):
                    pass
            return Z()

        def __del__(self):
            pass

    return [Agent(g) for g in range(S)], [_Ring(g) for g in range(S)]


@pytest.fixture
def fake(monkeypatch):
    from slimdqn import _hip

    log = []

    def install(refuse=()):
        lib = _FakeLib(log, refuse)
        monkeypatch.setattr(_hip, "lib", lambda: lib)
        monkeypatch.setattr(_hip, "current_stream", lambda: None)
        return log

    return install


def test_members_draw_their_own_streams_and_one_call_serves_all(fake):
    from slimdqn.networks.group import AgentGroup

    log = fake()
    agents, rbs = _make(3, log)
    group = AgentGroup(agents)
    for step in range(4):
        group.update_online_params(step, rbs)
    calls = [e for e in log if e[0] == "group"]
    assert [e[1] for e in calls] == [[i, 1000 + i, 2000 + i] for i in range(1, 5)], "draw i of member g is the member's i-th draw"
    assert calls[0][2] == [16, 32, 48], "every member's own ring"
    assert [e for e in log if e[0] == "create"] == [("create", [500, 501, 502])], "one group, made once"
    assert not any(e[0] == "solo" for e in log) and [rb.n for rb in rbs] == [4, 4, 4]
    group.close()
    assert log[-1] == ("destroy",)


@pytest.mark.parametrize("utd,tuf,tsf", [(1, 12, 5), (2, 30, 15), (1, 40, 7)])
def test_run_splitting_is_plan_step_runs(fake, utd, tuf, tsf):
    from slimdqn.networks._agent import plan_step_runs
    from slimdqn.networks.group import AgentGroup

    log = fake()
    agents, rbs = _make(2, log, utd, tuf, tsf)
    group = AgentGroup(agents)
    out = group.update_params_many(7, 50, rbs)
    want, draw = [], 0
    for n_grad, op, last in plan_step_runs(7, 50, utd, tuf, tsf):
        if n_grad >= agents[0].learn_steps_min:
            want.append(("group_steps", n_grad, [[1000 * g + draw + i + 1 for i in range(n_grad)] for g in range(2)]))
        else:
            want += [("group", [1000 * g + draw + i + 1 for g in range(2)]) for i in range(n_grad)]
        draw += n_grad
        if op is not None:
            want += [(op, g) for g in range(2)]
    got = [e[:2] if e[0] == "group" else e for e in log if e[0] != "create"]
    assert got == want
    assert any(e[0] == "group_steps" for e in got) and [rb.n for rb in rbs] == [draw, draw]
    updates = [s for s in range(7, 57) if s % tuf == 0]
    assert [[s for s, _ in o] for o in out] == [updates, updates]


@pytest.mark.parametrize("refuse,n", [("create", 6), ("learn", 3), ("steps", 6)])  # (3 steps: below learn_steps_min, single steps)
def test_fallback_after_a_refusal_uses_the_slots_already_drawn(fake, refuse, n):
    from slimdqn.networks.group import AgentGroup

    log = fake([refuse])
    agents, rbs = _make(2, log)
    group = AgentGroup(agents)
    group._sample_and_learn_many(rbs, n)
    group._sample_and_learn_many(rbs, n)
    assert [rb.n for rb in rbs] == [2 * n, 2 * n], "a refusal costs no draw"
    if refuse == "steps":  # the single group step serves the drawn slots, one set at a time, then every later step
        assert [e[1] for e in log if e[0] == "group"] == [[i, 1000 + i] for i in range(1, 13)]
        assert group._group_steps_ok is False and group._group_learn_ok is True
        assert not any(e[0] in ("solo", "group_steps") for e in log)
    else:  # the members' own step, member by member, on their own draws in order
        assert not any(e[0] in ("group", "group_steps") for e in log)
        for g in range(2):
            assert [e[2] for e in log if e[0] == "solo" and e[1] == g] == [1000 * g + i for i in range(1, 2 * n + 1)]


def test_agents_outside_the_domain_run_alone(fake):
    from slimdqn.networks.group import AgentGroup

    log = fake()
    agents, rbs = _make(2, log)
    agents[1]._arch = "cnn"
    calls = []
    for a in agents:
        a._sample_and_learn = lambda rb, a=a: calls.append((a.g, rb.g))
    AgentGroup(agents).update_online_params(0, rbs)
    assert calls == [(0, 0), (1, 1)] and log == []
    with pytest.raises(ValueError):
        AgentGroup([])
    with pytest.raises(ValueError):
        AgentGroup(agents * 17)


# ---- SeedTrainer ---------------------------------------------------------------------------------------------------------
class _Env:
    """A chain whose episode length depends on the seed; the state is a counter."""

    n_actions = 4

    def __init__(self, seed):
        self.length, self.t, self.n_steps, self.actions = 5 + seed, 0, 0, []
        self.state = self.observation = np.zeros(2, np.float32)

    def reset(self):
        self.n_steps = 0
        self.state = self.observation = np.array([self.t, 0], np.float32)

    def step(self, action):
        self.t += 1
        self.n_steps += 1
        self.actions.append(int(action))
        self.state = self.observation = np.array([self.t, self.n_steps], np.float32)
        return float(action) - 1.0, self.n_steps >= self.length


class _Rb:
    _clipping = None

    def __init__(self):
        self.added = []

    def add(self, tr):
        self.added.append((float(tr.observation[0]), int(tr.action), float(tr.reward), bool(tr.is_terminal)))


class _Log:
    def __init__(self):
        self.records = []

    def log(self, d):
        self.records.append(dict(d))


class _SoloAgent:
    """Greedy action = a hash of state and head; records the loop's calls."""

    def __init__(self, seed):
        self.seed, self.n_networks, self.calls, self.params = seed, 3, [], object()

    def greedy(self, head, state):
        return int(state[0] * 7 + head + self.seed) % 4

    def best_action(self, params, state, key):
        from slimdqn import prng
        from slimdqn.sample_collection.utils import HostAction

        return HostAction(self.greedy(prng.randint(key, 0, self.n_networks), state))

    def update_online_params(self, step, rb):
        self.calls.append(("online", step, len(rb.added)))

    def update_target_params(self, step):
        self.calls.append(("target", step))
        return step % 10 == 0, {"loss": float(step + self.seed)}

    def get_model(self):
        return {"seed": self.seed}


class _StubGroup:
    def __init__(self, agents):
        self.agents, self.act_calls = agents, 0

    def select_heads(self, keys, members):
        from slimdqn import prng

        return [prng.randint(k, 0, self.agents[m].n_networks) for k, m in zip(keys, members)]

    def best_actions(self, which, heads, states, members):
        self.act_calls += 1
        return np.array([self.agents[m].greedy(h, s) for m, h, s in zip(members, heads, states)])

    def update_online_params(self, step, rbs):
        for a, rb in zip(self.agents, rbs):
            a.update_online_params(step, rb)

    def update_target_params(self, step):
        return [a.update_target_params(step) for a in self.agents]

    def close(self):
        pass


def _p(seed, n_epochs=2):
    return {"seed": seed, "epsilon_end": 0.1, "epsilon_duration": 30, "n_training_steps_per_epoch": 25, "n_initial_samples": 9,
            "n_epochs": n_epochs, "horizon": 7, "wandb": _Log()}


def test_seed_trainer_is_trainer_per_seed(capsys):
    from experiments.base.dqn import Trainer
    from experiments.base.seeds import SeedTrainer
    from slimdqn import prng

    seeds = [0, 1, 2]
    saved = {"group": [], "solo": []}
    solo = []
    for s in seeds:
        t = Trainer(prng.PRNGKey(s), _p(s), _SoloAgent(s), _Env(s), _Rb(),
                    save_fn=lambda p, r, l, m: saved["solo"].append((p["seed"], [list(x) for x in r], m)))
        solo.append((t, t.run()))
    agents = [_SoloAgent(s) for s in seeds]
    st = SeedTrainer([prng.PRNGKey(s) for s in seeds], [_p(s) for s in seeds], agents, [_Env(s) for s in seeds], [_Rb() for _ in seeds],
                     save_fn=lambda p, r, l, m: saved["group"].append((p["seed"], [list(x) for x in r], m)), group=_StubGroup(agents))
    out = st.run()
    for i, (t, (returns, lengths)) in enumerate(solo):
        assert out[i] == (returns, lengths)
        assert st.seeds[i].env.actions == t.env.actions and len(t.env.actions) >= 50
        assert st.seeds[i].rb.added == t.rb.added
        assert agents[i].calls == t.agent.calls
        assert st.seeds[i].p["wandb"].records == t.p["wandb"].records
    assert sorted(saved["group"], key=lambda x: (x[0], len(x[1]))) == sorted(saved["solo"], key=lambda x: (x[0], len(x[1])))
    assert len({len(t.env.actions) for t, _ in solo}) > 1, "the seeds were meant to finish at different steps"
    assert 0 < st.group.act_calls <= max(len(t.env.actions) for t, _ in solo), "at most one acting call per step"
