"""Vectorised acting on MLP and general-shape cnn handles (``idqn_act_host_many_fc``, csrc/fc_act_many_kernels.h;
``DeviceAgent._best_actions``) against the single-state route (``idqn_act_host``: k_fc_q1 / k_fc_q, k_gconv_fwd + k_fc_q) on the
SAME handle.  The per-state arithmetic of the new kernels is that route's operation for operation, so every comparison is
byte equality: row e of the Q-values and action e of a call are what ``_best_action(which, heads[e], states[e])`` leaves in
``_q_out[0]`` and returns.  The oracle is never the code under test; one loose check ties the LunarLander rows to
``oracle.qnet_ref.forward`` in fp64 at the bar ``tests/test_gpu_acting.py`` applies to that handle's single-state route.

The shapes are the smallest at which each index path can go wrong, not all the workload's own:
  lunar     obs 8, A 4, K 3, [100, 100]     LunarLander: din = 100 gives a ragged 13-row wave slice and ragged 16-chunks,
                                            dout = 100 a ragged lane pass
  fc_tiny   obs 5, A 3, K 2, [7]
  fc_limit  obs 3, A 2, K 1, [512, 1, 64]   a width at the k_fc_q1 limit, a width of 1
  fc_wide   obs 6, A 5, K 2, [520]          just past FC_MAX_WIDTH: the k_fc_q twin
  gc_smoke  (84, 84, 4), A 6, K 1, [2, 3, 1, 15]     the reference's smoke shape
  gc_small  (12, 10, 3), A 3, K 3, [3, 2, 4, 5, 6]   three input channels, two hidden dense layers
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

CASES = {
    "lunar": ("fc", 8, 4, 3, [100, 100]),
    "fc_tiny": ("fc", 5, 3, 2, [7]),
    "fc_limit": ("fc", 3, 2, 1, [512, 1, 64]),
    "fc_wide": ("fc", 6, 5, 2, [520]),
    "gc_smoke": ("cnn", (84, 84, 4), 6, 1, [2, 3, 1, 15]),
    "gc_small": ("cnn", (12, 10, 3), 3, 3, [3, 2, 4, 5, 6]),
}
N_STATES = 32


def _inputs(name):
    """Online and target parameters that differ, with non-zero biases, and 32 states."""
    from oracle import qnet_ref as Q

    arch, obs, A, K, feats = CASES[name]
    seed = sorted(CASES).index(name)
    rng = np.random.default_rng(100 + seed)
    sets = []
    for s in (10 + seed, 50 + seed):
        p = Q.init_params(s, arch, obs, A, feats, K)
        for leaf in p:
            if leaf.endswith("bias"):
                p[leaf] = rng.uniform(-0.5, 0.5, p[leaf].shape).astype(np.float32)
        sets.append(p)
    states = Q.synthetic_batch(7 + seed, N_STATES, obs, A, arch)[0]
    return sets[0], sets[1], states


def _make(name):
    from slimdqn.networks.idqn import iDQN

    arch, obs, A, K, feats = CASES[name]
    p, pt, states = _inputs(name)
    agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent, p, pt, states


def _single(agent, which, head, state):
    """(Q row, action) of the single-state route for one host state."""
    act = int(agent._best_action(which, head, np.asarray(state)))
    return agent._q_out[0].cpu().numpy().copy(), act


@functools.lru_cache(maxsize=None)
def _case(name):
    """The agent and the single-state route's (Q row, action) for every (set, head, state), computed once."""
    agent, p, pt, states = _make(name)
    K = CASES[name][3]
    single = {(w, k, i): _single(agent, w, k, states[i]) for w in (0, 1) for k in range(K) for i in range(N_STATES)}
    return agent, p, pt, states, single


def _pin_buffers(agent, states, rows=33):
    import torch

    dt = torch.uint8 if agent._arch == "cnn" else torch.float32
    pin = torch.empty((rows, int(np.prod(agent._obs))), dtype=dt).pin_memory()
    for i in range(rows):
        pin[i] = torch.from_numpy(np.ascontiguousarray(states[i % len(states)]).reshape(-1))
    q_out = torch.full((rows, agent.network.n_actions), -123.0, dtype=torch.float32, device="cuda")
    acts = torch.full((40,), -9, dtype=torch.int32).pin_memory()
    return pin, q_out, acts


def _c_call(agent, which, heads, pin, n, q_out, acts, entry="idqn_act_host_many_fc"):
    from slimdqn import _hip

    h = np.ascontiguousarray(np.asarray(heads, np.int32))
    return getattr(_hip.lib(), entry)(agent._handle, which, h.ctypes.data, C.c_void_p(pin.data_ptr()), n, _hip.ptr(q_out),
                                      C.c_void_p(acts.data_ptr()), _hip.current_stream())


def _many(agent, which, heads, states):
    acts = agent._best_actions(which, heads, states)
    assert agent.__dict__.get("_act_many_ok") is False and agent.__dict__.get("_act_many_fc_ok") is True, "this is the loop"
    return agent._q_out[: len(heads)].cpu().numpy().copy(), np.asarray(acts)


def _heads(kind, E, K, rng):
    if kind == "equal":
        return [K - 1] * E
    if kind == "distinct":  # every head occurs (where E allows), no two neighbours equal (where K allows)
        return [e % K for e in range(E)]
    return rng.integers(0, K, E).tolist()


@pytest.mark.parametrize("E", [1, 2, 7, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_rows_are_the_single_state_routes_bytes(name, E):
    agent, p, pt, states, single = _case(name)
    K = CASES[name][3]
    rng = np.random.default_rng(E)
    for kind in ("equal", "distinct", "drawn"):
        heads = _heads(kind, E, K, rng)
        first = int(rng.integers(0, N_STATES - E + 1))  # the call's state e is state first + e: positions and states decouple
        for which in (0, 1):
            q, acts = _many(agent, which, heads, [states[first + e] for e in range(E)])
            assert q.shape == (E, CASES[name][2]) and acts.shape == (E,) and acts.dtype == np.int64
            for e, k in enumerate(heads):
                q1, a1 = single[(which, k, first + e)]
                assert q[e].tobytes() == q1.tobytes(), (name, kind, which, heads, e, q[e], q1)
                assert int(acts[e]) == a1, (name, kind, which, heads, e)
    if K > 1 or name == "gc_smoke":  # the two parameter sets are told apart
        assert single[(0, 0, 0)][0].tobytes() != single[(1, 0, 0)][0].tobytes()


def test_lunar_rows_against_the_oracle():
    """The bar of tests/test_gpu_acting.py for the fc handle's single-state route: 2e-6 * max(1, |Q|)."""
    from oracle import qnet_ref as Q

    agent, p, pt, states, single = _case("lunar")
    arch, obs, A, K, feats = CASES["lunar"]
    heads = [e % K for e in range(N_STATES)]
    for which, params in ((0, p), (1, pt)):
        q, acts = _many(agent, which, heads, list(states))
        for k in range(K):
            want = Q.forward(Q.head(params, k), states, arch)
            for e in range(k, N_STATES, K):
                err = np.abs(q[e] - want[e]).max()
                assert err <= 2e-6 * max(1.0, np.abs(want[e]).max()), (which, k, e, q[e], want[e])
                assert int(acts[e]) == int(np.argmax(want[e]))


@pytest.mark.parametrize("name", ["lunar", "fc_wide", "gc_small"])
def test_buffers_beyond_n_keep_their_sentinel_and_head_tables_are_data(name):
    """The C entry on buffers of its own: rows and actions beyond n untouched; a second call with the same n and buffers (one
    captured chain) but another head table and parameter set is correct on ITS inputs.  (The library has no debug route that
    reports how many graphs a handle holds -- idqn_debug_buffer names device buffers only -- so correctness alone is asserted.)"""
    import torch

    agent, p, pt, states, single = _case(name)
    K = CASES[name][3]
    pin, q_out, acts = _pin_buffers(agent, states)
    n = 5
    calls = ((0, [e % K for e in range(n)]), (1, [(K - 1 - e) % K for e in range(n)]), (0, [0] * n))
    seen = []
    for which, heads in calls:
        assert _c_call(agent, which, heads, pin, n, q_out, acts) == 0
        q = q_out.cpu().numpy()
        for e, k in enumerate(heads):
            q1, a1 = single[(which, k, e)]
            assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1, (name, which, heads, e)
        torch.cuda.synchronize()
        assert (q[n:] == -123.0).all() and (acts[n:].numpy() == -9).all()
        seen.append(q[:n].tobytes())
    assert seen[0] != seen[1]


def _ops(agent, states, pin, q_out, acts, K):
    """The calls the vectorised entry is interleaved with; each returns the bytes it produced."""
    from slimdqn import _hip

    lib = _hip.lib()

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
        return q1.tobytes() + bytes([a1])

    def begin_end(a):
        a._ensure_handle(32)
        one, out = pin[2], acts[36:]
        _hip.check(lib.idqn_act_host_begin(a._handle, 0, 0, C.c_void_p(one.data_ptr()), _hip.ptr(q_out[32:]),
                                           C.c_void_p(out.data_ptr()), _hip.current_stream()), "idqn_act_host_begin")
        _hip.check(lib.idqn_act_host_end(a._handle, C.c_void_p(out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
        return q_out[32].cpu().numpy().tobytes() + bytes([int(out[0])])

    def q_values(a):
        return a._q_values(1, 0, states[:5]).cpu().numpy().tobytes()

    def learn(a):
        from oracle import qnet_ref as Q

        batch = Q.synthetic_batch(99, 32, a._obs if a._arch == "cnn" else a._obs[0], a.network.n_actions, a._arch)
        return a._learn(Batch(*batch)).cpu().numpy().tobytes()

    heads_a, heads_b = [e % K for e in range(7)], [(2 * e + 1) % K for e in range(7)]
    return [many(0, heads_a), act_host, many(1, heads_b), begin_end, many(0, heads_b), q_values, many(1, heads_a), learn,
            many(0, heads_a), many(1, [K - 1] * 32)]


ARENAS = ("_online", "_target", "_mu", "_nu", "_count", "_cum")


@pytest.mark.parametrize("name", ["lunar", "gc_small"])
def test_interleaved_calls_equal_a_fresh_handles(name):
    """In the spirit of tests/handle_history.py: the ops run one after the other on ONE used handle; each is repeated on a
    freshly created agent that was given the used agent's arenas from just before the op.  Results and arenas: the same bytes."""
    import torch

    used, p, pt, states = _make(name)
    K = CASES[name][3]
    used._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(used, states)
    for i, op in enumerate(_ops(used, states, pin, q_out, acts, K)):
        torch.cuda.synchronize()
        before = {a: getattr(used, a).clone() for a in ARENAS}
        got = op(used)
        torch.cuda.synchronize()
        fresh = _make(name)[0]
        for a in ARENAS:
            getattr(fresh, a).copy_(before[a])
        torch.cuda.synchronize()
        want = op(fresh)
        torch.cuda.synchronize()
        assert got == want, (name, i)
        for a in ARENAS:
            assert getattr(used, a).cpu().numpy().tobytes() == getattr(fresh, a).cpu().numpy().tobytes(), (name, i, a)
        fresh._destroy_handle()


@pytest.mark.parametrize("name", ["lunar", "fc_wide", "gc_small"])
def test_ties_give_the_first_maximum(name):
    """The last Dense kernel of one head zeroed, its bias with equal entries: action 0 from both routes."""
    import torch

    agent, p, pt, states = _make(name)
    K = CASES[name][3]
    last = "Dense_%d" % max(int(m.split("_")[1]) for m in agent.params["params"] if m.startswith("Dense_"))
    agent.params["params"][last]["kernel"][K - 1].zero_()
    agent.params["params"][last]["bias"][K - 1].fill_(0.25)
    torch.cuda.synchronize()
    heads = [K - 1, 0, K - 1, K - 1]
    q, acts = _many(agent, 0, heads, [states[e] for e in range(4)])
    for e, k in enumerate(heads):
        q1, a1 = _single(agent, 0, k, states[e])
        assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1
        if k == K - 1:
            assert (q[e] == 0.25).all() and int(acts[e]) == 0 and a1 == 0


def switch_child_digest():
    """What a child process of test_switches_give_the_default_modes_bytes computes: the bytes of a few calls on three handles."""
    import hashlib

    out = {}
    for name in ("lunar", "fc_wide", "gc_small"):
        agent, p, pt, states = _make(name)
        K = CASES[name][3]
        hsh = hashlib.sha256()
        for which, heads in ((0, [e % K for e in range(7)]), (1, [K - 1] * 7), (1, [(e + 1) % K for e in range(32)]), (0, [0])):
            q, acts = _many(agent, which, heads, [states[e] for e in range(len(heads))])
            for e, k in enumerate(heads):
                q1, a1 = _single(agent, which, k, states[e])
                assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1, (name, which, heads, e)
            hsh.update(q.tobytes() + acts.tobytes())
        out[name] = hsh.hexdigest()
    return out


SWITCH_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_fc_act_many as T
print("RESULT" + json.dumps(T.switch_child_digest()))
"""


def test_switches_give_the_default_modes_bytes():
    """IDQN_ACT_GRAPH=0 (eager launches), IDQN_ACT_POLL=0 (device-to-host copy + synchronise) and both: the switches are read
    once per process, so each mode is a fresh child process, one at a time, under a time limit of its own.  Each child holds
    the rows to its own single-state route; across the modes the bytes equal the default mode's."""
    digests = {}
    for mode in ((), ("IDQN_ACT_GRAPH",), ("IDQN_ACT_POLL",), ("IDQN_ACT_GRAPH", "IDQN_ACT_POLL")):
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


def _assert_untouched(q_out, acts):
    import torch

    torch.cuda.synchronize()
    assert (q_out.cpu().numpy() == -123.0).all() and (acts.numpy() == -9).all(), "a refused call enqueued work"


@pytest.mark.parametrize("name", ["lunar", "gc_small"])
def test_bad_arguments_are_refused_before_anything_is_enqueued(name):
    import torch

    from slimdqn import _hip

    agent, p, pt, states, single = _case(name)
    K = CASES[name][3]
    agent._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(agent, states)
    lib = _hip.lib()
    for which, heads, n in ((0, [0], 0), (0, [0] * 33, 33), (0, [0, K, 0], 3), (0, [0, -1], 2), (2, [0, 0], 2), (-1, [0], 1)):
        assert _c_call(agent, which, heads, pin, n, q_out, acts) == _hip.E_INVALID, (which, heads, n)
        assert b"idqn_act_host_many_fc" in lib.idqn_last_error()
        _assert_untouched(q_out, acts)
    # null pointers, one argument at a time
    heads = np.zeros(2, np.int32)
    good = [agent._handle, 0, heads.ctypes.data, C.c_void_p(pin.data_ptr()), 2, _hip.ptr(q_out), C.c_void_p(acts.data_ptr()),
            _hip.current_stream()]
    for i in (0, 2, 3, 5, 6):
        args = list(good)
        args[i] = None
        assert lib.idqn_act_host_many_fc(*args) == _hip.E_INVALID, i
        assert b"null pointer" in lib.idqn_last_error()
        _assert_untouched(q_out, acts)
    # an idqn_act_host_begin that nobody has collected yet
    one, one_out = pin[0], acts[36:]
    _hip.check(lib.idqn_act_host_begin(agent._handle, 0, 0, C.c_void_p(one.data_ptr()), _hip.ptr(q_out[32:]),
                                       C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_begin")
    assert _c_call(agent, 0, [0, 0], pin, 2, q_out, acts) == _hip.E_INVALID
    _hip.check(lib.idqn_act_host_end(agent._handle, C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
    torch.cuda.synchronize()
    assert (q_out[:32].cpu().numpy() == -123.0).all() and (acts[:32].numpy() == -9).all()
    # a valid call after the refusals is correct
    heads = [(e + 1) % K for e in range(4)]
    assert _c_call(agent, 1, heads, pin, 4, q_out, acts) == 0
    q = q_out[:4].cpu().numpy()
    for e, k in enumerate(heads):
        q1, a1 = single[(1, k, e)]
        assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1
    assert (acts[4:32].numpy() == -9).all() and (q_out[4:32].cpu().numpy() == -123.0).all()


def test_mfma_and_quantile_handles_refuse_and_the_first_entry_still_refuses_these():
    from oracle import make_golden as G
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.networks.iiqn import iIQN

    # the cnn_small case of tests/test_gpu_act_many.py: an MFMA-path handle
    arch, obs, A, feats, K, B, steps = G.FP_CASES["cnn_small"]
    p, pt, batches = G.fp_case_inputs("cnn_small")
    agent = iDQN(0, obs, A, K, feats, arch, 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    agent._load_flat(agent._online, p)
    agent._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(agent, batches[0][0])
    assert _c_call(agent, 0, [0, 1, 0], pin, 3, q_out, acts) == _hip.E_INVALID
    assert b"MFMA" in _hip.lib().idqn_last_error()
    _assert_untouched(q_out, acts)
    assert _c_call(agent, 0, [0, 1, 0], pin, 3, q_out, acts, entry="idqn_act_host_many") == 0  # ... which has its own entry
    # quantile heads
    (obs, A, feats, K, B, N) = G.IQN_CASES["iqn_small"][:6]
    iq = iIQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, n_quantiles=N)
    iq._ensure_handle(32)
    pin, q_out, acts = _pin_buffers(iq, batches[0][0])
    assert _c_call(iq, 0, [0, 1, 0], pin, 3, q_out, acts) == _hip.E_INVALID
    assert b"quantile" in _hip.lib().idqn_last_error()
    _assert_untouched(q_out, acts)
    # idqn_act_host_many keeps refusing the handles of this file
    for name in ("lunar", "gc_small"):
        agent, p, pt, states, single = _case(name)
        pin, q_out, acts = _pin_buffers(agent, states)
        assert _c_call(agent, 0, [0, 0, 0], pin, 3, q_out, acts, entry="idqn_act_host_many") == _hip.E_INVALID
        _assert_untouched(q_out, acts)


def test_collection_with_the_call_equals_collection_with_the_loop():
    """Two agents from one seed on a LunarLander-shaped synthetic setup, one forced to loop: 40 collect_vector_samples steps
    at E = 5 with gradient steps in between leave the same replay contents, sampled batches and online arenas."""
    import torch

    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.utils import collect_vector_samples, linear_schedule
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    E, B = 5, 16
    p = dict(horizon=1000)
    eps = linear_schedule(1.0, 0.05, 20)  # exploring at first, almost always greedy by step 20
    runs = []
    for loop in (False, True):
        agent = iDQN(3, 8, 4, 3, [100, 100], "fc", 1e-3, 0.99, 1, 1, 10**9, 10**9)
        if loop:
            agent._act_many_fc_ok = False
        envs = [SyntheticVector(e, episode_length=(7, 5, 11, 4, 9)[e]) for e in range(E)]
        for env in envs:
            env.reset()
        rb = VectorReplayBuffer(UniformSamplingDistribution(0), B, 400, stack_size=1, update_horizon=1, gamma=0.99, n_envs=E)
        key = prng.PRNGKey(11)
        losses, batches, n_many = [], [], 0
        for step in range(40):
            key, sub = prng.split(key)
            collect_vector_samples(prng.split(sub, E), envs, agent, rb, p, eps, step)
            if step >= 8:
                batch = rb.sample()
                fields = (batch.state, batch.action, batch.reward, batch.next_state, batch.is_terminal)
                batches.append(b"".join(getattr(f, "tensor", f).cpu().numpy().tobytes() for f in fields))
                losses.append(agent._learn(batch).cpu().numpy().tobytes())
        torch.cuda.synchronize()
        assert agent.__dict__.get("_act_many_fc_ok") is (not loop)
        assert len(losses) == 32
        # the replay contents: the element rows, and every field of 128 more draws (the ring itself is allocated uninitialised,
        # its unwritten slots are nobody's)
        last = rb.sample(128)
        contents = b"".join(getattr(f, "tensor", f).cpu().numpy().tobytes()
                            for f in (last.state, last.action, last.reward, last.next_state, last.is_terminal))
        runs.append((losses, batches, agent._online.cpu().numpy().tobytes(), contents, rb._meta_dev.cpu().numpy().tobytes(),
                     [int(rb._add_count)]))
    for x, y in zip(*runs):
        assert x == y
