"""Vectorised acting (``idqn_act_host_many``, csrc/act_many_kernels.h; ``DeviceAgent._best_actions``) against the
single-state path (``idqn_act_host``, csrc/act_kernels.h) on the SAME handle.  The per-state arithmetic of the new kernels is
the single-state path's operation for operation, so every comparison here is byte equality: row e of the Q-values and action e
of a call are what ``_best_action(which, heads[e], states[e])`` leaves in ``_q_out[0]`` and returns.  The ``cnn_small`` rows
are also held to the oracle at the bar ``tests/test_gpu_acting.py`` applies to the single-state path.
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


def _make(name):
    from oracle import make_golden as G
    from slimdqn.networks.idqn import iDQN

    arch, obs, A, feats, K, B, steps = G.FP_CASES[name]
    p, pt, batches = G.fp_case_inputs(name)
    agent = iDQN(0, obs, A, K, feats, arch, 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent, arch, A, K, p, pt, batches[0]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _make(name)


def _single(agent, which, head, state):
    """(Q row, action) of the single-state path for one host state."""
    act = int(agent._best_action(which, head, np.asarray(state)))
    return agent._q_out[0].cpu().numpy().copy(), act


def _many(agent, which, heads, states):
    acts = agent._best_actions(which, heads, states)
    assert agent.__dict__.get("_act_many_ok") is True, "the batched entry was refused: this is the loop"
    return agent._q_out[: len(heads)].cpu().numpy().copy(), np.asarray(acts)


def _assert_rows_equal(agent, which, heads, states, q, acts):
    assert q.shape[0] == len(heads) and acts.shape == (len(heads),)
    for e, head in enumerate(heads):
        q1, a1 = _single(agent, which, head, states[e])
        assert q[e].tobytes() == q1.tobytes(), (which, heads, e, q[e], q1)
        assert int(acts[e]) == a1, (which, heads, e)


@functools.lru_cache(maxsize=None)
def _small_reference():
    """cnn_small: the single-state path's (Q row, action) for every (set, head, state), computed once; and the oracle's Q."""
    from oracle import qnet_ref as Q

    agent, arch, A, K, p, pt, batch = _case("cnn_small")
    states = batch[0]
    single = {(w, k, i): _single(agent, w, k, states[i]) for w in (0, 1) for k in range(K) for i in range(32)}
    oracle = {(w, k): Q.forward(Q.head(params, k), states[:32], arch) for w, params in ((0, p), (1, pt)) for k in range(K)}
    return single, oracle


def _pattern(kind, E):
    if kind == "all0":
        return [0] * E
    if kind == "all1":
        return [1] * E
    if kind == "alternating":
        return [e % 2 for e in range(E)]
    heads = [0] * E  # one lone state on the other head in the middle: unsorted input, groups of 1 and E - 1
    heads[E // 2] = 1
    return heads


@pytest.mark.parametrize("kind", ["all0", "all1", "alternating", "lone"])
@pytest.mark.parametrize("E", [1, 2, 5, 32])
def test_cnn_small_rows_are_the_single_state_paths_bytes(E, kind):
    agent, arch, A, K, p, pt, batch = _case("cnn_small")
    single, oracle = _small_reference()
    states = batch[0]
    heads = _pattern(kind, E)
    for which in (0, 1):
        q, acts = _many(agent, which, heads, [states[e] for e in range(E)])
        for e, k in enumerate(heads):
            q1, a1 = single[(which, k, e)]
            assert q[e].tobytes() == q1.tobytes(), (which, heads, e, q[e], q1)
            assert int(acts[e]) == a1
            want = oracle[(which, k)][e]
            assert np.abs(q[e] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (which, heads, e, q[e], want)
            assert int(acts[e]) == int(np.argmax(want))


def test_atari_k5_seven_states_five_heads():
    """F = 7744 (row groups that do not divide evenly), J = 512, groups of 2, 2, 1, 1, 1 states."""
    agent, arch, A, K, p, pt, batch = _case("cnn_atari_k5")
    heads = [0, 4, 2, 2, 0, 3, 1]
    states = [batch[0][e] for e in range(7)]
    q, acts = _many(agent, 0, heads, states)
    _assert_rows_equal(agent, 0, heads, states, q, acts)


def test_atari_18_actions():
    """A = 18: more actions than the head kernel has waves."""
    agent, arch, A, K, p, pt, batch = _case("cnn_atari_a18_b64")
    heads = [1, 0, 1]
    states = [batch[0][e] for e in (5, 6, 7)]
    q, acts = _many(agent, 1, heads, states)
    assert q.shape == (3, 18)
    _assert_rows_equal(agent, 1, heads, states, q, acts)


def test_ties_give_the_first_maximum():
    import torch

    agent, arch, A, K, p, pt, batch = _make("cnn_small")
    agent.params["params"]["Dense_1"]["kernel"].zero_()
    agent.params["params"]["Dense_1"]["bias"].zero_()
    torch.cuda.synchronize()
    q, acts = _many(agent, 0, [0, 1, 1, 0, 1], [batch[0][e] for e in range(5)])
    assert (q == 0).all() and acts.tolist() == [0] * 5


def test_graph_is_reused_with_new_states_and_heads():
    """Two calls with the same buffers (one instantiated graph) but other states and heads: the second call's rows are the
    single-state path's on ITS inputs -- the head and group tables travel as data."""
    agent, arch, A, K, p, pt, batch = _case("cnn_small")
    states = batch[0]
    first = _many(agent, 0, [0, 0, 1, 0, 1], [states[e] for e in range(5)])
    heads2, states2 = [1, 1, 0, 1, 1], [states[e] for e in range(10, 15)]
    q2, acts2 = _many(agent, 1, heads2, states2)
    _assert_rows_equal(agent, 1, heads2, states2, q2, acts2)
    assert first[0].tobytes() != q2.tobytes()


SWITCH_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_act_many as T
T.test_graph_is_reused_with_new_states_and_heads()
T.test_atari_k5_seven_states_five_heads()
print("RESULT" + json.dumps({"ok": True}))
"""


@pytest.mark.parametrize("switch", ["IDQN_ACT_GRAPH", "IDQN_ACT_POLL"])
def test_graph_reuse_with_the_switch_off(switch):
    """IDQN_ACT_GRAPH=0 (eager launches) and IDQN_ACT_POLL=0 (device-to-host copy + synchronise), each read once per process:
    the same comparisons in a fresh child process."""
    env = dict(os.environ)
    env[switch] = "0"
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SWITCH_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1]
    assert json.loads(line[len("RESULT"):]) == {"ok": True}


def test_no_residue_on_the_handle():
    """A handle that has run idqn_act_host_many and a fresh one, from the same state and inputs: a learn step, an
    idqn_act_host call and a q_values call give the same bytes (the single-state mailbox and its counters are untouched)."""
    import torch

    used, arch, A, K, p, pt, batch = _make("cnn_small")
    fresh = _make("cnn_small")[0]
    states = batch[0]
    _many(used, 0, [1, 0, 1], [states[e] for e in range(3)])
    _many(used, 1, [0] * 32, [states[e] for e in range(32)])
    out = []
    for agent in (used, fresh):
        b = Batch(*batch)
        losses = agent._learn(b).cpu().numpy().copy()
        q1, a1 = _single(agent, 0, 1, states[4])
        qn = agent._q_values(1, 0, states[:5]).cpu().numpy().copy()
        torch.cuda.synchronize()
        out.append((losses, agent._online.cpu().numpy(), agent._mu.cpu().numpy(), q1, np.asarray([a1]), qn))
    for x, y in zip(*out):
        assert x.tobytes() == y.tobytes()


def _c_call(agent, which, heads, pin, n, q_out, acts):
    from slimdqn import _hip

    h = np.ascontiguousarray(np.asarray(heads, np.int32))
    return _hip.lib().idqn_act_host_many(agent._handle, which, h.ctypes.data, C.c_void_p(pin.data_ptr()), n, _hip.ptr(q_out),
                                         C.c_void_p(acts.data_ptr()), _hip.current_stream())


def _refusal_buffers(agent, states):
    import torch

    dt = torch.uint8 if agent._arch == "cnn" else torch.float32
    pin = torch.empty((33, int(np.prod(agent._obs))), dtype=dt).pin_memory()
    for i in range(33):
        pin[i] = torch.from_numpy(np.ascontiguousarray(states[i % len(states)]).reshape(-1))
    q_out = torch.full((33, agent.network.n_actions), -123.0, dtype=torch.float32, device="cuda")
    acts = torch.full((40,), -9, dtype=torch.int32).pin_memory()
    return pin, q_out, acts


def _assert_untouched(q_out, acts):
    import torch

    torch.cuda.synchronize()
    assert (q_out.cpu().numpy() == -123.0).all() and (acts.numpy() == -9).all(), "a refused call enqueued work"


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    from slimdqn import _hip

    agent, arch, A, K, p, pt, batch = _case("cnn_small")
    agent._ensure_handle(32)
    states = batch[0]
    pin, q_out, acts = _refusal_buffers(agent, states)
    lib = _hip.lib()
    for which, heads, n in ((0, [0], 0), (0, [0] * 33, 33), (0, [0, K, 0], 3), (0, [0, -1], 2), (2, [0, 1], 2)):
        assert _c_call(agent, which, heads, pin, n, q_out, acts) == _hip.E_INVALID, (which, heads, n)
        _assert_untouched(q_out, acts)
    # an idqn_act_host_begin that nobody has collected yet
    one, one_out = pin[0], acts[36:]
    _hip.check(lib.idqn_act_host_begin(agent._handle, 0, 0, C.c_void_p(one.data_ptr()), _hip.ptr(q_out[32:]),
                                       C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_begin")
    assert _c_call(agent, 0, [0, 1], pin, 2, q_out, acts) == _hip.E_INVALID
    _hip.check(lib.idqn_act_host_end(agent._handle, C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
    import torch

    torch.cuda.synchronize()
    assert (q_out[:32].cpu().numpy() == -123.0).all() and (acts[:32].numpy() == -9).all()
    # a valid call after the refusals is correct
    heads = [1, 0, 0, 1]
    assert _c_call(agent, 1, heads, pin, 4, q_out, acts) == 0
    q = q_out[:4].cpu().numpy()
    for e, k in enumerate(heads):
        q1, a1 = _single(agent, 1, k, states[e])
        assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1
    assert (acts[4:32].numpy() == -9).all() and (q_out[4:32].cpu().numpy() == -123.0).all()


@pytest.mark.parametrize("kind", ["fc", "general"])
def test_handles_outside_the_domain_refuse_and_best_actions_loops(kind):
    from oracle import qnet_ref as Q
    from slimdqn import _hip, prng
    from slimdqn.networks.idqn import iDQN

    if kind == "fc":
        agent = iDQN(0, 8, 4, 3, [100, 100], "fc", 1e-3, 0.99, 1, 1, 10**9, 10**9)
        states = Q.synthetic_batch(3, 6, 8, 4, "fc")[0]
    else:
        agent = iDQN(0, (84, 84, 4), 6, 1, [2, 3, 1, 15], "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9)
        states = Q.synthetic_batch(3, 6, (84, 84, 4), 6, "cnn")[0]
    agent._ensure_handle(32)
    pin, q_out, acts = _refusal_buffers(agent, states)
    assert _c_call(agent, 0, [0, 0, 0], pin, 3, q_out, acts) == _hip.E_INVALID
    _assert_untouched(q_out, acts)
    keys = prng.split(prng.PRNGKey(5), 6)
    hosts = [np.asarray(s) for s in states]
    got = agent.best_actions(agent.params, hosts, keys)
    assert agent._act_many_ok is False
    rows = agent._q_out[:6].cpu().numpy().copy()
    for i in range(6):
        a1 = int(agent.best_action(agent.params, hosts[i], keys[i]).item())
        assert int(got[i]) == a1
        assert rows[i].tobytes() == agent._q_out[0].cpu().numpy().tobytes()
    assert [int(a) for a in agent.best_actions(agent.params, hosts, keys)] == [int(a) for a in got]  # the loop, from now on


def test_best_actions_draws_each_head_from_its_key():
    """iDQN.best_actions is [best_action(params, s, k).item()] -- heads drawn per key -- and select_actions on top of it
    equals select_action per environment on the device agent."""
    from slimdqn import prng
    from slimdqn.sample_collection.utils import select_action, select_actions

    agent, arch, A, K, p, pt, batch = _case("cnn_small")
    states = [np.asarray(batch[0][e]) for e in range(9)]
    keys = prng.split(prng.PRNGKey(77), 9)
    assert len({prng.randint(k, 0, K) for k in keys}) == K
    got = agent.best_actions(agent.target_params, states, keys)
    assert [int(a) for a in got] == [int(agent.best_action(agent.target_params, s, k).item()) for s, k in zip(states, keys)]
    eps = lambda n: 0.3  # noqa: E731
    want = [select_action(agent.best_action, agent.params, s, k, A, eps, 0).item() for s, k in zip(states, keys)]
    assert select_actions(agent.best_actions, agent.params, states, keys, A, eps, 0) == want
