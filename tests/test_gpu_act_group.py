"""Acting groups (``idqn_act_group_create`` / ``idqn_act_group_host``, csrc/act_many_kernels.h; ``AgentGroup.best_actions`` with cnn
members) against the single-state path (``idqn_act_host``) of the MEMBER every state names.  The group kernels are the bodies of
``idqn_act_host_many``'s with the parameter base read from a table, so every comparison is byte equality; the ``cnn_small`` rows
are also held to the fp64 oracle at the 2e-6 relative bound of tests/test_gpu_act_many.py.

Members get distinct parameters: member g loads the case's heads rolled by g, online and target exchanged on odd g, so that a
wrong member, head or parameter set changes bytes.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def _member(name, g):
    """Member g of a group on FP case ``name``; also the (set, head) of the case that its (which, k) holds."""
    from oracle import make_golden as G
    from slimdqn.networks.idqn import iDQN

    arch, obs, A, feats, K, B, steps = G.FP_CASES[name]
    p, pt, batches = G.fp_case_inputs(name)
    sets = (p, pt) if g % 2 == 0 else (pt, p)
    agent = iDQN(0, obs, A, K, feats, arch, 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    agent._load_flat(agent._online, {k: np.roll(np.asarray(v), g, axis=0) for k, v in sets[0].items()})
    agent._load_flat(agent._target, {k: np.roll(np.asarray(v), g, axis=0) for k, v in sets[1].items()})
    agent._ensure_handle(32)
    source = {(w, k): ((w + g) % 2, (k - g) % K) for w in (0, 1) for k in range(K)}
    return agent, source


class _Group:
    """The C object over ``agents`` with buffers of its own."""

    def __init__(self, agents):
        import torch

        from slimdqn import _hip

        self.agents = list(agents)
        handles = (C.c_void_p * len(self.agents))(*[a._handle.value for a in self.agents])
        self.g = C.c_void_p()
        _hip.check(_hip.lib().idqn_act_group_create(handles, len(self.agents), C.byref(self.g)), "idqn_act_group_create")
        a0 = self.agents[0]
        self.pin = torch.empty((33, int(np.prod(a0._obs))), dtype=torch.uint8).pin_memory()
        self.q_out = torch.full((33, a0.network.n_actions), -123.0, dtype=torch.float32, device="cuda")
        self.acts = torch.full((40,), -9, dtype=torch.int32).pin_memory()

    def raw(self, which, members, heads, n, g=None, pin=True, q=True, acts=True, m_ptr=True, h_ptr=True):
        from slimdqn import _hip

        m = np.ascontiguousarray(np.asarray(members, np.int32))
        h = np.ascontiguousarray(np.asarray(heads, np.int32))
        return _hip.lib().idqn_act_group_host(self.g if g is None else g, which, m.ctypes.data if m_ptr else None, h.ctypes.data if h_ptr else None,
                                              C.c_void_p(self.pin.data_ptr()) if pin else None, n, _hip.ptr(self.q_out) if q else None,
                                              C.c_void_p(self.acts.data_ptr()) if acts else None, _hip.current_stream())

    def call(self, which, members, heads, states):
        import torch

        from slimdqn import _hip

        n = len(heads)
        for i, s in enumerate(states):
            self.pin[i] = torch.from_numpy(np.ascontiguousarray(s).reshape(-1))
        _hip.check(self.raw(which, members, heads, n), "idqn_act_group_host")
        return self.q_out[:n].cpu().numpy().copy(), self.acts[:n].numpy().copy()

    def close(self):
        from slimdqn import _hip

        if self.g is not None:
            _hip.lib().idqn_act_group_destroy(self.g)
            self.g = None


def _single(agent, which, head, state):
    act = int(agent._best_action(which, head, np.asarray(state)))
    return agent._q_out[0].cpu().numpy().copy(), act


@functools.lru_cache(maxsize=None)
def _small():
    """cnn_small: three members, the groups over the first two and over all three, the members' own single-state (Q row, action)
    for every (member, set, head, state), computed once, and the oracle's Q rows of the case's (set, head)."""
    from oracle import make_golden as G
    from oracle import qnet_ref as Q

    arch, obs, A, feats, K, B, steps = G.FP_CASES["cnn_small"]
    p, pt, batches = G.fp_case_inputs("cnn_small")
    states = batches[0][0]
    members = [_member("cnn_small", g) for g in range(3)]
    agents = [a for a, _ in members]
    single = {(g, w, k, i): _single(agents[g], w, k, states[i]) for g in range(3) for w in (0, 1) for k in range(K) for i in range(32)}
    oracle = {(w, k): Q.forward(Q.head(params, k), states[:32], arch) for w, params in ((0, p), (1, pt)) for k in range(K)}
    groups = {2: _Group(agents[:2]), 3: _Group(agents)}
    return agents, [src for _, src in members], states, single, oracle, groups, K


def _pattern(kind, n, S, K):
    """(members, heads) of n states."""
    if kind == "one_pair":  # n = 32: four register chunks of one Dense_0 group
        return [S - 1] * n, [K - 1] * n
    if kind == "every_state_another_member":
        return [e % S for e in range(n)], [(e // S) % K for e in range(n)]
    if kind == "same_head_on_different_members":  # must not share a W0 stream
        return [(e // 2) % S for e in range(n)], [1] * n
    if kind == "lone":  # unsorted input: a lone state of another member in the middle
        m = [0] * n
        m[n // 2] = S - 1
        return m, [0] * n
    assert kind == "alternating"
    return [(S - 1) if e % 2 else 0 for e in range(n)], [0 if e % 2 else K - 1 for e in range(n)]


PATTERNS = ["one_pair", "every_state_another_member", "same_head_on_different_members", "lone", "alternating"]


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("n", [1, 2, 5, 32])
@pytest.mark.parametrize("S", [2, 3])
def test_rows_are_the_members_single_state_bytes(S, n, kind):
    agents, sources, states, single, oracle, groups, K = _small()
    members, heads = _pattern(kind, n, S, K)
    for which in (0, 1):
        q, acts = groups[S].call(which, members, heads, [states[e] for e in range(n)])
        for e, (g, k) in enumerate(zip(members, heads)):
            q1, a1 = single[(g, which, k, e)]
            assert q[e].tobytes() == q1.tobytes(), (which, members, heads, e, q[e], q1)
            assert int(acts[e]) == a1
            want = oracle[sources[g][(which, k)]][e]
            assert np.abs(q[e] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (which, members, heads, e, q[e], want)
            assert int(acts[e]) == int(np.argmax(want))


def test_atari_k5_two_members_seven_states():
    """F = 7744 (row groups that do not divide evenly), J = 512, K = 5, S = 2: Dense_0 groups of 2, 1, 1, 2, 1 states."""
    from oracle import make_golden as G

    states = G.fp_case_inputs("cnn_atari_k5")[2][0][0]
    agents = [_member("cnn_atari_k5", g)[0] for g in range(2)]
    group = _Group(agents)
    members, heads = [1, 0, 1, 0, 0, 1, 1], [0, 4, 2, 2, 4, 2, 0]
    for which in (0, 1):
        q, acts = group.call(which, members, heads, [states[e] for e in range(7)])
        for e, (g, k) in enumerate(zip(members, heads)):
            q1, a1 = _single(agents[g], which, k, states[e])
            assert q[e].tobytes() == q1.tobytes(), (which, e, q[e], q1)
            assert int(acts[e]) == a1
    group.close()


def test_ties_give_the_first_maximum():
    import torch

    agents = [_member("cnn_small", g)[0] for g in range(2)]
    states = _small()[2]
    for a in agents:
        a.params["params"]["Dense_1"]["kernel"].zero_()
        a.params["params"]["Dense_1"]["bias"].zero_()
    torch.cuda.synchronize()
    group = _Group(agents)
    q, acts = group.call(0, [0, 1, 1, 0, 1], [0, 1, 1, 0, 1], [states[e] for e in range(5)])
    assert (q == 0).all() and acts.tolist() == [0] * 5
    group.close()


def _assert_call(group, agents, which, members, heads, states):
    q, acts = group.call(which, members, heads, states)
    for e, (g, k) in enumerate(zip(members, heads)):
        q1, a1 = _single(agents[g], which, k, states[e])
        assert q[e].tobytes() == q1.tobytes(), (which, members, heads, e, q[e], q1)
        assert int(acts[e]) == a1
    return q


def test_one_group_takes_changing_n_members_and_heads():
    """One group, one set of buffers: the graphs per n are reused with other members, heads, sets and states -- the assignment
    travels as data."""
    agents, sources, states, single, oracle, groups, K = _small()
    g3 = groups[3]
    first = _assert_call(g3, agents, 0, [0, 0, 2, 1, 1], [0, 0, 1, 0, 1], [states[e] for e in range(5)])
    second = _assert_call(g3, agents, 1, [2, 1, 1, 0, 2], [1, 1, 0, 1, 1], [states[e] for e in range(10, 15)])
    assert first.tobytes() != second.tobytes()
    _assert_call(g3, agents, 0, [1], [1], [states[20]])
    _assert_call(g3, agents, 1, [e % 3 for e in range(32)], [e % 2 for e in range(32)], [states[31 - e] for e in range(32)])
    _assert_call(g3, agents, 0, [2, 1, 1, 0, 2], [0, 1, 0, 1, 1], [states[e] for e in range(3, 8)])


SWITCH_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_act_group as T
T.test_one_group_takes_changing_n_members_and_heads()
print("RESULT" + json.dumps({"ok": True}))
"""


@pytest.mark.parametrize("switch", ["IDQN_ACT_GRAPH", "IDQN_ACT_POLL"])
def test_changing_calls_with_the_switch_off(switch):
    """IDQN_ACT_GRAPH=0 (eager launches) and IDQN_ACT_POLL=0 (device-to-host copy + synchronise), each read once per process:
    the same calls in a fresh child process."""
    env = dict(os.environ)
    env[switch] = "0"
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SWITCH_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1]
    assert json.loads(line[len("RESULT"):]) == {"ok": True}


def test_a_learner_step_between_two_calls_is_seen():
    from oracle import make_golden as G

    batch = G.fp_case_inputs("cnn_small")[2][0]
    agents = [_member("cnn_small", g)[0] for g in range(2)]
    states = batch[0]
    group = _Group(agents)
    members, heads, sts = [1, 0, 1, 0], [0, 1, 1, 0], [states[e] for e in range(4)]
    before = _assert_call(group, agents, 0, members, heads, sts)
    agents[1]._learn(Batch(*batch))
    after = _assert_call(group, agents, 0, members, heads, sts)  # (against the member's own path AFTER the step)
    assert before[[1, 3]].tobytes() == after[[1, 3]].tobytes(), "member 0 did not learn"
    assert (before[[0, 2]] != after[[0, 2]]).any(axis=1).all(), "member 1's step is not seen"
    group.close()


def test_no_residue_on_the_members():
    """Members whose own ``_best_action`` / ``_best_actions`` are interleaved with group calls, and fresh ones from the same
    parameters: the same bytes from every own call, then from a learner step, a single-state call and ``_q_values``."""
    import torch
    from oracle import make_golden as G

    batch = G.fp_case_inputs("cnn_small")[2][0]
    states = batch[0]
    used = [_member("cnn_small", g)[0] for g in range(2)]
    fresh = [_member("cnn_small", g)[0] for g in range(2)]
    group = _Group(used)
    got = {id(a): [] for a in used + fresh}

    def own(agents):
        for a in agents:
            acts = a._best_actions(1, [1, 0, 1], [states[e] for e in range(3)])
            got[id(a)].append((a._q_out[:3].cpu().numpy().tobytes(), np.asarray(acts).tobytes()))
            got[id(a)].append((_single(a, 0, 1, states[4])[0].tobytes(), b""))

    group.call(0, [1, 0, 1], [0, 1, 1], [states[e] for e in range(3)])
    own(used)
    group.call(1, [0] * 32, [1] * 32, [states[e] for e in range(32)])
    own(used)
    group.call(0, [1, 1], [0, 0], [states[e] for e in range(2)])
    own(fresh), own(fresh)
    for a in used + fresh:
        losses = a._learn(Batch(*batch)).cpu().numpy().copy()
        q1, a1 = _single(a, 0, 1, states[4])
        qn = a._q_values(1, 0, states[:5]).cpu().numpy().copy()
        torch.cuda.synchronize()
        got[id(a)].append((losses.tobytes(), a._online.cpu().numpy().tobytes(), a._mu.cpu().numpy().tobytes(), q1.tobytes(), a1, qn.tobytes()))
    for u, f in zip(used, fresh):
        assert got[id(u)] == got[id(f)]
    group.close()


def _create(agents):
    from slimdqn import _hip

    for a in agents:
        a._ensure_handle(32)
    handles = (C.c_void_p * len(agents))(*[a._handle.value for a in agents])
    g = C.c_void_p()
    rc = _hip.lib().idqn_act_group_create(handles, len(agents), C.byref(g))
    return rc, g, _hip.lib().idqn_last_error().decode(errors="replace")


def test_creation_refusals():
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.iiqn import iIQN

    agents = _small()[0]
    base = agents[0]
    small = lambda obs=(20, 20, 4), A=5, K=2, feats=(32, 32, 32, 128), arch="cnn": iDQN(0, obs, A, K, list(feats), arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)  # noqa: E731
    cases = [
        ("fc", [base, small(obs=8, A=5, feats=(100, 100), arch="fc")], "MLP (fc) handle"),
        ("general shape", [base, small(feats=(2, 3, 1, 15))], "general-shape"),
        ("quantile heads", [base, iIQN(3, (20, 20, 4), 5, 2, [32, 32, 32, 256], "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=4)], "quantile heads"),
        ("J > 512", [small(feats=(32, 32, 32, 640))], "J = 640 > 512"),
        ("A > 32", [small(A=33)], "A = 33 > 32"),
        ("general shape, member 1", [base, small(feats=(32, 48, 32, 128))], "member 1 is a general-shape"),
        ("observation", [base, small(obs=(24, 20, 4))], "differs from member 0"),
        ("features", [base, small(feats=(32, 64, 32, 128))], "differs from member 0"),
        ("n_actions", [base, small(A=6)], "differs from member 0"),
        ("n_heads", [base, small(K=3)], "differs from member 0"),
        ("named twice", [base, agents[1], base], "same handle"),
    ]
    for what, members, text in cases:
        rc, g, msg = _create(members)
        assert rc == _hip.E_INVALID and g.value is None, what
        assert text in msg and "idqn_act_group_create" in msg, (what, msg)
    lib = _hip.lib()
    g = C.c_void_p()
    handles = (C.c_void_p * 33)(*[base._handle.value] * 33)
    for n in (0, 33, -1):
        assert lib.idqn_act_group_create(handles, n, C.byref(g)) == _hip.E_INVALID and "must be in [1, 32]" in lib.idqn_last_error().decode()
    assert lib.idqn_act_group_create(None, 2, C.byref(g)) == _hip.E_INVALID and "null pointer" in lib.idqn_last_error().decode()
    assert lib.idqn_act_group_create(handles, 2, None) == _hip.E_INVALID and "null pointer" in lib.idqn_last_error().decode()
    # a group of ONE member is fine
    rc, g, _ = _create([base])
    assert rc == 0
    lib.idqn_act_group_destroy(g)


GENERIC_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_act_group as T
rc, g, msg = T._create([T._member("cnn_small", g)[0] for g in range(2)])
print("RESULT" + json.dumps({"rc": rc, "msg": msg}))
"""


def test_creation_is_refused_under_act_generic():
    from slimdqn import _hip

    env = dict(os.environ)
    env["IDQN_ACT_GENERIC"] = "1"
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + GENERIC_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][len("RESULT"):])
    assert got["rc"] == _hip.E_INVALID and "IDQN_ACT_GENERIC" in got["msg"]


def test_call_refusals_enqueue_nothing_and_the_next_call_is_exact():
    import torch

    from slimdqn import _hip

    agents = [_member("cnn_small", g)[0] for g in range(2)]
    states = _small()[2]
    group = _Group(agents)
    for i in range(33):
        group.pin[i] = torch.from_numpy(np.ascontiguousarray(states[i % 32]).reshape(-1))
    lib, K = _hip.lib(), 2

    def refused(text, *a, **kw):
        assert group.raw(*a, **kw) == _hip.E_INVALID, (text, a, kw)
        msg = lib.idqn_last_error().decode()
        assert text in msg and "idqn_act_group_host" in msg, (text, msg)
        torch.cuda.synchronize()
        assert (group.q_out.cpu().numpy() == -123.0).all() and (group.acts[:36].numpy() == -9).all(), "a refused call enqueued work"

    for kw in (dict(pin=False), dict(q=False), dict(acts=False), dict(m_ptr=False), dict(h_ptr=False)):
        refused("null pointer", 0, [0, 1], [0, 1], 2, **kw)
    assert lib.idqn_act_group_host(None, 0, None, None, None, 1, None, None, None) == _hip.E_INVALID
    refused("n is outside [1, 32]", 0, [0], [0], 0)
    refused("n is outside [1, 32]", 0, [0] * 33, [0] * 33, 33)
    refused("which", 2, [0, 1], [0, 1], 2)
    refused("member is outside", 0, [0, 2, 0], [0, 0, 0], 3)
    refused("member is outside", 0, [0, -1], [0, 0], 2)
    refused("head is outside", 0, [0, 1, 0], [0, K, 0], 3)
    refused("head is outside", 1, [0, 1], [-1, 0], 2)
    # a member with an idqn_act_host_begin that nobody has collected yet
    one_out = group.acts[36:]
    _hip.check(lib.idqn_act_host_begin(agents[1]._handle, 0, 0, C.c_void_p(group.pin[0].data_ptr()), _hip.ptr(agents[1]._q_out),
                                       C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_begin")
    refused("idqn_act_host_begin", 0, [0, 0], [0, 1], 2)
    _hip.check(lib.idqn_act_host_end(agents[1]._handle, C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
    # a valid call after the refusals is exact
    members, heads = [1, 0, 0, 1], [1, 0, 1, 0]
    assert group.raw(1, members, heads, 4) == 0
    q, acts = group.q_out[:4].cpu().numpy(), group.acts[:4].numpy().copy()
    for e, (g, k) in enumerate(zip(members, heads)):
        q1, a1 = _single(agents[g], 1, k, states[e])
        assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1
    assert (group.acts[4:32].numpy() == -9).all() and (group.q_out[4:32].cpu().numpy() == -123.0).all()
    group.close()


def test_agent_group_best_actions_takes_the_route_and_equals_the_loop():
    from slimdqn.networks.group import AgentGroup

    # members of its own (the handle of one is re-created below, which would leave the shared fixture's C groups with a freed
    # handle); they hold the fixture members' parameters, so the fixture's single-state rows, only read here, are theirs
    states, single = _small()[2], _small()[3]
    agents = [_member("cnn_small", g)[0] for g in range(3)]
    on, off = AgentGroup(agents), AgentGroup(agents)
    on.act_group_sizes, off.act_group_sizes = frozenset({3}), frozenset()
    members, heads = [2, 0, 1, 1, 2, 0, 0], [1, 0, 1, 0, 0, 1, 1]
    sts = [np.asarray(states[e]) for e in range(7)]
    a_on = on.best_actions(1, heads, sts, members)
    rows = on.q_out[:7].cpu().numpy().copy()
    assert on._group_act_cnn_ok is True and on.__dict__.get("_group_act_ok") is None
    a_off = off.best_actions(1, heads, sts, members)
    assert off.__dict__.get("_group_act_cnn_ok") is None, "the size is off: the loop"
    assert a_on.tolist() == a_off.tolist() == [single[(g, 1, k, e)][1] for e, (g, k) in enumerate(zip(members, heads))]
    for e, (g, k) in enumerate(zip(members, heads)):
        assert rows[e].tobytes() == single[(g, 1, k, e)][0].tobytes()
    # default members: one state per member, in order
    assert on.best_actions(0, [1, 0, 1], sts[:3]).tolist() == [single[(g, 0, k, g)][1] for g, k in enumerate([1, 0, 1])]
    # a member re-creates its handle (a larger batch): the group follows
    agents[1]._ensure_handle(64)
    assert on.best_actions(1, heads, sts, members).tolist() == a_on.tolist() and on._act_group_handles[1] == agents[1]._handle.value
    assert on.q_out[:7].cpu().numpy().tobytes() == rows.tobytes()
    on.close(), off.close()


class _SmallAtari:
    """20 x 20 frames, 4-stack states, rewards that depend on the action; the protocol of slimdqn/environments/synthetic.py."""

    def __init__(self, seed, n_actions=5, episode_length=9):
        rng = np.random.default_rng(seed)
        self.n_actions, self.episode_length = n_actions, episode_length
        self.state_height, self.state_width, self.n_stacked_frames = 20, 20, 4
        self._pool = rng.integers(0, 256, (64, 20, 20), dtype=np.uint8)
        self._n = 0

    @property
    def observation(self):
        return np.copy(self.state[:, :, -1])

    def reset(self):
        self.state = np.zeros((20, 20, 4), np.uint8)
        self.state[:, :, -1] = self._pool[self._n % 64]
        self._n += 1
        self.n_steps = 0

    def step(self, action):
        self.state = np.concatenate([self.state[:, :, 1:], self._pool[self._n % 64][:, :, None]], axis=2)
        self._n += 1
        self.n_steps += 1
        return float((int(action) + self._n) % 3 - 1), bool(self.n_steps >= self.episode_length)


def _trainer_run(vector, route_on):
    import torch

    from experiments.base.seeds import SeedTrainer, SeedVectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.networks.group import AgentGroup
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    S, E = 2, 3
    ps = [dict(seed=s, epsilon_end=0.05, epsilon_duration=20, n_epochs=2, n_training_steps_per_epoch=24 + 6 * s, n_initial_samples=8 + 2 * s,
               horizon=12, wandb=NullLogger()) for s in range(S)]
    agents = [iDQN(prng.PRNGKey(50 + s), (20, 20, 4), 5, 2, [32, 32, 32, 128], "cnn", 1e-3, 0.99, 1, 1, 10, 4, adam_eps=1.5e-4) for s in range(S)]
    kw = dict(stack_size=4, update_horizon=1, gamma=0.99)
    if vector:
        rbs = [VectorReplayBuffer(UniformSamplingDistribution(s), 16, 120, n_envs=E, **kw) for s in range(S)]
        envs = [[_SmallAtari(10 * s + e, episode_length=(9, 7)[e % 2]) for e in range(E)] for s in range(S)]
    else:
        rbs = [ReplayBuffer(UniformSamplingDistribution(s), batch_size=16, max_capacity=60, **kw) for s in range(S)]
        envs = [_SmallAtari(s, episode_length=9 + 2 * s) for s in range(S)]
    group = AgentGroup(agents)
    group.act_group_sizes = frozenset({S}) if route_on else frozenset()
    trainer = (SeedVectorTrainer if vector else SeedTrainer)([prng.PRNGKey(70 + s) for s in range(S)], ps, agents, envs, rbs, group=group)
    calls = []
    inner = group.best_actions
    group.best_actions = lambda *a, **k: calls.append(len(a[1])) or inner(*a, **k)
    out = trainer.run()
    torch.cuda.synchronize()
    state = []
    for a, rb in zip(agents, rbs):
        if hasattr(rb, "_flush_meta"):
            rb._flush_meta()
        # replay contents: every element row, and one more batch drawn from the buffer (the frames the rows name, stacked; the ring
        # itself is allocated uninitialised, and which of its slots were ever written is the buffer's own business)
        batch = rb.sample()
        drawn = tuple(np.asarray(getattr(batch, n)).tobytes() for n in ("state", "action", "reward", "next_state", "is_terminal"))
        state.append((a._online.cpu().numpy().tobytes(), a._target.cpu().numpy().tobytes(), a._mu.cpu().numpy().tobytes(), rb._add_count,
                      drawn, rb._meta_dev.cpu().numpy().tobytes(), int(a._count[0].item())))
    return out, state, [p["wandb"].records for p in ps], group.__dict__.get("_group_act_cnn_ok"), calls


@pytest.mark.parametrize("vector", [False, True])
def test_trainers_are_the_same_with_the_route_on_and_off(vector):
    on, off = _trainer_run(vector, True), _trainer_run(vector, False)
    assert on[3] is True and off[3] is None
    assert len(on[4]) > 5 and (not vector or max(on[4]) > 2), "the greedy states of several seeds shared calls"
    assert on[0] == off[0], "returns and lengths"
    assert on[2] == off[2], "log records"
    for g, (a, b) in enumerate(zip(on[1], off[1])):
        assert a == b, f"seed {g}: parameters, moments or replay contents differ"
        assert a[-1] > 10, "the seeds learned"


ENTRY_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import torch
from experiments.atari import idqn, idqn_seeds
from test_gpu_seed_group import _same
flags = ["-en", "seeds", "-at", "cnn", "-f", "32", "64", "64", "512", "-nn", "2", "-ne", "2", "-ntspe", "40", "-nis", "20", "-ed", "30", "-tuf", "10", "-tsf", "5", "-rbc", "100", "-horizon", "15"]
result = {}
for E in (1, 2):
    ps, agents = idqn_seeds.run(flags + ["--first_seed", "3", "--last_seed", "4"] + (["--n_envs", "2"] if E > 1 else []), save_root=os.path.join(TMP, "group%d" % E))
    assert [p["seed"] for p in ps] == [3, 4]
    result["counts%d" % E] = [int(a._count[0].item()) for a in agents]
    result["losses%d" % E] = [any("loss" in r for r in p["wandb"].records) for p in ps]
    if E == 1:  # against the single-seed entry point, per seed
        for p, a in zip(ps, agents):
            p1, a1 = idqn.run(flags + ["-s", str(p["seed"])], save_root=os.path.join(TMP, "solo"))
            torch.cuda.synchronize()
            _same(a, a1, "seed %d" % p["seed"])
            assert p["wandb"].records == p1["wandb"].records
print("RESULT" + json.dumps(result))
"""


def test_atari_seeds_entry_point_equals_single_seed_runs(tmp_path):
    """``experiments/atari/idqn_seeds.py`` on seeds 3..4 (the acting group's default size 2) against ``experiments/atari/idqn.py``
    once per seed: every agent's bytes and every log record; then the same seeds with ``--n_envs 2``, which has no single-seed
    entry to compare with and is run for its wiring.  In a child process: the entry points switch ``IDQN_STEP_GRAPH`` on for
    the process they run in."""
    env = dict(os.environ)
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\nTMP = %r\n" % (ROOT, str(tmp_path)) + ENTRY_CHILD], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][len("RESULT"):])
    assert min(got["counts1"]) > 20 and min(got["counts2"]) > 20 and all(got["losses1"]) and all(got["losses2"]), got
