"""Vectorised impala acting on the device (``idqn_act_host_many_impala``, csrc/imp_act_many_kernels.h): for every case of
tests/impala_act_shapes.py the Q rows and actions of ONE call equal, byte for byte, the loop of ``idqn_act_host`` on the same
handle -- no tolerance.  Then: one captured chain per (n, buffers) reused with other heads, the other parameter set, after a
learner step and after a target sync; the two switches in child processes; the handle after a many-state call against a fresh
one (the method of tests/test_gpu_handle_history.py); the refusals, with the arenas untouched and the stream idle; the Python
route (``_act_many_imp_ok``) and a short ``VectorTrainer`` run with the route on and forced off.
Reference ops: slimdqn/networks/idqn.py:126-131, slimdqn/sample_collection/utils.py:8-21, architectures/dqn.py:7-29,54-60.
Without the entry every test here fails at the missing symbol or at the flag assertion."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import impala_act_shapes as T
import impala_shapes as S

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_act_host_many_impala"
ALL_SIZES = frozenset(range(1, 33))
ARENAS = ("_online", "_target", "_mu", "_nu", "_grad", "_count", "_losses")


def _make(row):
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = T.case(row)
    agent = iDQN(0, obs, A, K, feats, "impala", S.LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=S.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    agent.act_many_imp_sizes = ALL_SIZES
    return agent


@functools.lru_cache(maxsize=None)
def _shared(row):
    return _make(row)


def _single(agent, which, head, state):
    """(Q row bytes, action) of idqn_act_host for one host state."""
    act = int(agent._best_action(which, head, np.asarray(state)))
    return agent._q_out[0].cpu().numpy().tobytes(), act


@functools.lru_cache(maxsize=None)
def _single_of(row, which, head, index):
    """The single-state route on the shared (never trained) agent of a row, computed once per (set, head, state)."""
    return _single(_shared(row), which, head, T.states(row, index + 1)[index])


def _many(agent, which, heads, states):
    acts = agent._best_actions(which, heads, states)
    assert agent.__dict__.get("_act_many_imp_ok") is True, "this is the loop"
    assert agent.__dict__.get("_act_many_ok") is False and agent.__dict__.get("_act_many_fc_ok") is False
    assert acts.dtype == np.int64 and acts.shape == (len(heads),)
    return agent._q_out[: len(heads)].cpu().numpy().copy(), acts


@pytest.mark.parametrize("row,n,assign,which", T.CASES, ids=["-".join(str(x) for x in c) for c in T.CASES])
def test_one_call_gives_the_loops_bytes(row, n, assign, which):
    agent = _shared(row)
    obs, feats, A, K, B = T.shape(row)
    heads, states = T.heads(assign, n, K), T.states(row, n)
    q, acts = _many(agent, which, heads, states)
    assert q.shape == (n, A)
    pool = 2 * B  # the states repeat with this period
    for e, k in enumerate(heads):
        q1, a1 = _single_of(row, which, k, e % pool)
        assert q[e].tobytes() == q1, (row, e, k, q[e], np.frombuffer(q1, np.float32))
        assert int(acts[e]) == a1, (row, e, k)
    if row == "tie":  # the tie row's pools tie exactly on head 0; the Q rows are still told apart from head 1's
        assert q[0].tobytes() != q[1].tobytes()
    if row == "no_hidden":
        assert A == 40 and np.isfinite(q).all()


def test_equal_q_values_give_the_first_maximum():
    """The last Dense kernel of one head zeroed, its bias with equal entries: action 0 from both routes."""
    import torch

    agent = _make("five_heads")
    K = T.shape("five_heads")[3]
    agent.params["params"]["Dense_1"]["kernel"][K - 1].zero_()
    agent.params["params"]["Dense_1"]["bias"][K - 1].fill_(0.25)
    torch.cuda.synchronize()
    heads, states = [K - 1, 0, K - 1, 2, K - 1], T.states("five_heads", 5)
    q, acts = _many(agent, 0, heads, states)
    for e, k in enumerate(heads):
        q1, a1 = _single(agent, 0, k, states[e])
        assert q[e].tobytes() == q1 and int(acts[e]) == a1
        if k == K - 1:
            assert (q[e] == 0.25).all() and int(acts[e]) == 0


def _pin_buffers(agent, states, rows=33):
    import torch

    pin = torch.empty((rows, int(np.prod(agent._obs))), dtype=torch.uint8).pin_memory()
    for i in range(rows):
        pin[i] = torch.from_numpy(np.array(states[i % len(states)]).reshape(-1))
    q_out = torch.full((rows, agent.network.n_actions), -123.0, dtype=torch.float32, device="cuda")
    acts = torch.full((40,), -9, dtype=torch.int32).pin_memory()
    return pin, q_out, acts


def _c_call(agent, which, heads, pin, n, q_out, acts):
    from slimdqn import _hip

    h = np.ascontiguousarray(np.asarray(heads, np.int32))
    return getattr(_hip.lib(), NAME)(agent._handle, which, h.ctypes.data, C.c_void_p(pin.data_ptr()), n, _hip.ptr(q_out),
                                     C.c_void_p(acts.data_ptr()), _hip.current_stream())


def test_one_chain_serves_other_heads_sets_and_changed_parameters():
    """The same (n, buffers) -- one captured chain -- with other heads, with ``which`` flipped, after a learner step and after a
    target sync; rows and actions beyond n keep their sentinel.  Every call is held to the loop at that moment."""
    import torch

    agent = _make("five_heads")
    obs, feats, A, K, B, p, pt, batch = T.case("five_heads")
    agent._ensure_handle(32)
    n, states = 6, T.states("five_heads", 6)
    pin, q_out, acts = _pin_buffers(agent, states)
    seen = []

    def check(which, heads):
        assert _c_call(agent, which, heads, pin, n, q_out, acts) == 0
        torch.cuda.synchronize()
        q, a = q_out.cpu().numpy().copy(), acts.numpy().copy()
        assert (q[n:] == -123.0).all() and (a[n:] == -9).all()
        for e, k in enumerate(heads):
            q1, a1 = _single(agent, which, k, states[e])
            assert q[e].tobytes() == q1 and int(a[e]) == a1, (which, heads, e)
        seen.append(q[:n].tobytes())

    rot, desc = T.heads("rot", n, K), T.heads("desc", n, K)
    check(0, rot)
    check(0, desc)
    check(1, desc)
    agent._learn(Batch(*[np.array(x) for x in batch]))
    check(0, desc)
    check(1, desc)
    agent._local_target_sync()
    check(1, desc)
    check(0, T.heads("skip", n, K))
    assert seen[0] != seen[1] and seen[1] != seen[2], "other heads, the other parameter set"
    assert seen[1] != seen[3] and seen[2] == seen[4], "a learner step moves the online set and leaves the target set alone"
    assert seen[4] != seen[5], "a target sync moves the target set"


def switch_child_digest():
    """What a child process of test_switches_give_the_default_modes_bytes computes."""
    out = {}
    for row, calls in (("mid", ((0, "rot", 3), (1, "one", 9))), ("no_hidden", ((0, "one", 2),))):
        agent, K = _make(row), T.shape(row)[3]
        hsh = hashlib.sha256()
        for which, assign, n in calls:
            heads, states = T.heads(assign, n, K), T.states(row, n)
            q, acts = _many(agent, which, heads, states)
            for e, k in enumerate(heads):
                q1, a1 = _single(agent, which, k, states[e])
                assert q[e].tobytes() == q1 and int(acts[e]) == a1, (row, which, heads, e)
            hsh.update(q.tobytes() + acts.tobytes())
        out[row] = hsh.hexdigest()
    return out


SWITCH_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_impala_act_many as M
print("RESULT" + json.dumps(M.switch_child_digest()))
"""


def test_switches_give_the_default_modes_bytes():
    """IDQN_ACT_GRAPH=0 (eager launches) and IDQN_ACT_POLL=0 (device-to-host copy + synchronise): read once per process, so each
    mode is a fresh child process, one at a time, under a time limit of its own.  Each child holds the rows to its own loop;
    across the modes the bytes equal the default mode's."""
    digests = {}
    for mode in ((), ("IDQN_ACT_GRAPH",), ("IDQN_ACT_POLL",)):
        env = dict(os.environ)
        for s in ("IDQN_ACT_GRAPH", "IDQN_ACT_POLL", "IDQN_HIP_LIB"):
            env.pop(s, None)
        for s in mode:
            env[s] = "0"
        out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SWITCH_CHILD], env=env, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, (mode, out.stderr[-3000:])
        line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1]
        digests[mode] = json.loads(line[len("RESULT"):])
    assert all(d == digests[()] for d in digests.values()), digests


def test_the_handle_is_undisturbed():
    """The ops run one after the other on ONE used handle, many-state calls between them; each is repeated on a freshly created
    agent that was given the used agent's arenas from just before the op.  Results and arenas: the same bytes."""
    import torch

    row = "five_heads"
    obs, feats, A, K, B, p, pt, batch = T.case(row)
    states = T.states(row, 8)
    used = _make(row)
    used._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(used, states)

    def many(which, heads):
        def run(a):
            a._ensure_handle(32)
            for b in (q_out, acts):
                b.fill_(-5)
            assert _c_call(a, which, heads, pin, len(heads), q_out, acts) == 0
            return q_out.cpu().numpy().tobytes() + acts.numpy().tobytes()
        return run

    def act_host(a):
        q1, a1 = _single(a, 1, K - 1, states[3])
        return q1 + bytes([a1])

    def q_values(a):
        return a._q_values(0, 1, np.stack(states[:5])).cpu().numpy().tobytes()

    def learn(a):
        return a._learn(Batch(*[np.array(x) for x in batch])).cpu().numpy().tobytes()

    state_arenas = ("_online", "_target", "_mu", "_nu", "_count", "_cum")
    rot, desc = T.heads("rot", 7, K), T.heads("desc", 7, K)
    ops = [many(0, rot), learn, many(1, desc), q_values, many(0, desc), act_host, many(1, [K - 1] * 32), learn, act_host]
    for i, op in enumerate(ops):
        torch.cuda.synchronize()
        before = {a: getattr(used, a).clone() for a in state_arenas}
        got = op(used)
        torch.cuda.synchronize()
        fresh = _make(row)
        for a in state_arenas:
            getattr(fresh, a).copy_(before[a])
        torch.cuda.synchronize()
        want = op(fresh)
        torch.cuda.synchronize()
        assert got == want, i
        for a in state_arenas:
            assert getattr(used, a).cpu().numpy().tobytes() == getattr(fresh, a).cpu().numpy().tobytes(), (i, a)
        fresh._destroy_handle()


# ---- refusals ------------------------------------------------------------------------------------------------------------
OTHER_KINDS = {  # kind: (arch, obs, features, A, K, IDQN_CONV)
    "fc": ("fc", 8, [16, 16], 4, 3, None),
    "gcnn": ("cnn", (20, 20, 1), [8, 8, 8], 40, 3, None),
    "plane": ("cnn", (20, 20, 4), [32, 32, 32, 128], 5, 2, "bf16x3"),
    "f32": ("cnn", (20, 20, 4), [32, 32, 32, 128], 5, 2, "f32"),
}


def _snapshot(agent):
    import torch

    torch.cuda.synchronize()
    return {a: getattr(agent, a).cpu().numpy().tobytes() for a in ARENAS}


def _assert_refused(agent, rc, before, q_out, acts, what):
    import torch

    from slimdqn import _hip

    text = _hip.lib().idqn_last_error().decode(errors="replace")
    assert rc == _hip.E_INVALID, (what, rc)
    assert text and NAME in text, (what, text)
    assert torch.cuda.current_stream().query(), (what, "a refused call left work on the stream")
    assert _snapshot(agent) == before, what
    assert (q_out.cpu().numpy() == -123.0).all() and (acts.numpy() == -9).all(), (what, "a refused call wrote its outputs")


@pytest.mark.parametrize("kind", list(OTHER_KINDS))
def test_other_architectures_are_refused(kind, monkeypatch):
    from slimdqn.networks.idqn import iDQN

    arch, obs, feats, A, K, conv = OTHER_KINDS[kind]
    if conv:
        monkeypatch.setenv("IDQN_CONV", conv)  # (read by idqn_create)
    else:
        monkeypatch.delenv("IDQN_CONV", raising=False)
    agent = iDQN(3, obs, A, K, list(feats), arch, 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-6)
    agent._ensure_handle(32)
    size = int(np.prod(agent._obs))
    pin, q_out, acts = _pin_buffers(agent, [np.zeros(size, np.uint8)])
    before = _snapshot(agent)
    _assert_refused(agent, _c_call(agent, 0, [0, 0], pin, 2, q_out, acts), before, q_out, acts, kind)
    agent._destroy_handle()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    from slimdqn import _hip

    row = "odd_even"
    agent, K = _make(row), T.shape(row)[3]
    agent._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(agent, T.states(row, 4))
    lib = _hip.lib()
    before = _snapshot(agent)
    for which, heads, n in ((0, [0], 0), (0, [0] * 33, 33), (0, [0, K, 0], 3), (0, [0, -1], 2), (2, [0, 0], 2), (-1, [0], 1)):
        _assert_refused(agent, _c_call(agent, which, heads, pin, n, q_out, acts), before, q_out, acts, (which, heads, n))
    heads = np.zeros(2, np.int32)
    good = [agent._handle, 0, heads.ctypes.data, C.c_void_p(pin.data_ptr()), 2, _hip.ptr(q_out), C.c_void_p(acts.data_ptr()),
            _hip.current_stream()]
    for i in (0, 2, 3, 5, 6):
        args = list(good)
        args[i] = None
        rc = getattr(lib, NAME)(*args)
        assert b"null pointer" in lib.idqn_last_error()
        _assert_refused(agent, rc, before, q_out, acts, ("null", i))
    # an idqn_act_host_begin that nobody has collected yet
    one, one_out = pin[0], acts[36:]
    _hip.check(lib.idqn_act_host_begin(agent._handle, 0, 0, C.c_void_p(one.data_ptr()), _hip.ptr(q_out[32:]),
                                       C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_begin")
    rc = _c_call(agent, 0, [0, 0], pin, 2, q_out, acts)
    text = lib.idqn_last_error().decode(errors="replace")
    _hip.check(lib.idqn_act_host_end(agent._handle, C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
    assert rc == _hip.E_INVALID and NAME in text and "idqn_act_host_begin" in text
    assert _snapshot(agent) == before
    assert (q_out[:32].cpu().numpy() == -123.0).all() and (acts[:32].numpy() == -9).all()
    # and the handle still serves
    assert _c_call(agent, 0, [0, K - 1], pin, 2, q_out, acts) == 0
    agent._destroy_handle()


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_best_actions_sets_the_flag_and_respects_the_sizes():
    row = "odd_even"
    obs, feats, A, K, B = T.shape(row)
    agent = _make(row)
    states, heads = T.states(row, 7), T.heads("rot", 7, K)
    agent.act_many_imp_sizes = frozenset({7})
    got = agent._best_actions(0, heads, states)
    rows = agent._q_out[:7].cpu().numpy().copy()
    assert agent.__dict__.get("_act_many_imp_ok") is True
    assert agent.__dict__.get("_act_many_ok") is False and agent.__dict__.get("_act_many_fc_ok") is False
    agent.act_many_imp_sizes = frozenset()  # forced off: the loop, the same bytes
    loop = agent._best_actions(0, heads, states)
    assert loop.tolist() == got.tolist() and agent._q_out[:7].cpu().numpy().tobytes() == rows.tobytes()
    agent._destroy_handle()


def _trainer_run(route_on):
    import torch

    from experiments.base.dqn import VectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticAtari
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection import utils
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    obs, A, feats, K, E, capacity = (84, 84, 4), 4, [3, 7, 5, 9], 2, 3, 48
    agent = iDQN(0, obs, A, K, feats, "impala", 1e-3, 0.99, 1, 2, 8, 6, adam_eps=1e-6)
    agent.act_many_imp_sizes = ALL_SIZES if route_on else frozenset()
    envs = [SyntheticAtari(e, n_actions=A, episode_length=(9, 6, 11)[e]) for e in range(E)]
    rb = VectorReplayBuffer(UniformSamplingDistribution(0), 8, capacity, stack_size=4, update_horizon=1, gamma=0.99,
                            clipping=lambda r: float(np.clip(r, -1, 1)), n_envs=E)
    trajectory, real_select = [], utils.select_actions

    def select_actions(*a, **kw):
        actions = real_select(*a, **kw)
        trajectory.append([int(x) for x in actions])
        return actions

    utils.select_actions = select_actions
    try:
        p = dict(epsilon_end=0.05, epsilon_duration=10, n_epochs=1, n_training_steps_per_epoch=45, n_initial_samples=12, horizon=1000,
                 wandb=NullLogger())
        trainer = VectorTrainer(prng.PRNGKey(1), p, agent, envs, rb)
        trainer.run()
    finally:
        utils.select_actions = real_select
    torch.cuda.synchronize()
    arenas = {a: getattr(agent, a).cpu().numpy().tobytes() for a in ("_online", "_target", "_mu", "_nu", "_count")}
    memory = {}
    for key in range(max(0, rb.add_count - capacity), rb.add_count):
        el = rb._memory[key]
        memory[key] = (np.asarray(el.state).tobytes(), np.asarray(el.next_state).tobytes(), int(el.action), float(el.reward),
                       bool(el.is_terminal), bool(el.episode_end))
    flags = (agent.__dict__.get("_act_many_imp_ok"), agent.__dict__.get("_act_many_ok"), agent.__dict__.get("_act_many_fc_ok"))
    agent._destroy_handle()
    return trajectory, arenas, memory, rb.add_count, trainer.total_steps, flags


def test_vector_trainer_with_the_route_on_and_forced_off():
    on, off = _trainer_run(True), _trainer_run(False)
    assert on[5][0] is True and off[5][0] is None, "the route served one run and was never asked in the other"
    assert on[4] == off[4] >= 45 and on[3] == off[3] > 0
    assert on[0] == off[0] and len(on[0]) >= 15, "the same trajectory"
    assert on[2].keys() == off[2].keys() and all(on[2][k] == off[2][k] for k in on[2]), "the same replay contents"
    assert on[1] == off[1], "the same parameters and Adam state"
