"""Vectorised i-IQN acting (``idqn_iqn_act_host_many``, csrc/iqn_act_many_kernels.h; ``iIQN.best_actions``) against the
single-state path (``idqn_iqn_act_host``, csrc/iqn_act_kernels.h) on the SAME handle.  The per-state arithmetic of the new
kernels is the single-state path's operation for operation, so every comparison with it is byte equality: row e of the
Q-values and action e of a call are what ``_act_host(which, heads[e], states[e], taus[e])`` leaves in ``_q_out[0]`` and returns.

The ``iqn_small`` rows are also held to the fp64 oracle (``oracle.iqn_ref.greedy_action``) at the bar
``tests/test_gpu_iqn_acting.py`` applies to the single-state path: 2e-6 * max(1, max|want|), and the oracle's action.  Those
inputs come from ``SEED``, picked on the CPU with the oracle alone (``python tests/test_gpu_iqn_act_many.py [seed]`` prints
the gaps of a seed) so that the oracle's two largest Q-values are more than 1e-4 * max(1, max|want|) apart in every row; the
test asserts that gap first.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]
from test_gpu_iqn_acting import _agent, _case  # noqa: E402  (the case builders of the single-state tests)

pytestmark = pytest.mark.gpu
SEED = 0
SC = 4  # IQN_ACT_MANY_SC of csrc/iqn_act_many_kernels.h (slimdqn._hip.IQN_ACT_MANY_SC; the host test ties the two)
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


_ccase = functools.lru_cache(maxsize=None)(_case)  # (a case's parameters and states are built once and never written)


@functools.lru_cache(maxsize=None)
def _shared(name):
    """One agent per case for the tests that do not change it, and the case."""
    return _agent(name), _ccase(name)


def _state(name, e):
    states = _ccase(name)[7]
    return np.asarray(states[e % len(states)])


def _tau(name, e, salt=0):
    """The N fractions of state e: different for every state."""
    N = _ccase(name)[4]
    return np.random.default_rng([17, sum(name.encode()), e, salt]).random(N).astype(np.float32)


def _single(agent, which, head, state, tau):
    """(Q row, action) of the single-state path."""
    act = int(agent._act_host(which, head, np.asarray(state), tau, None).item())
    return agent._q_out[0].cpu().numpy().copy(), act


@functools.lru_cache(maxsize=None)
def _reference(name, which, head, e, salt=0):
    """The single-state path's (Q row, action) for (which, head, state e, tau e) on the shared agent: computed once."""
    return _single(_shared(name)[0], which, head, _state(name, e), _tau(name, e, salt))


def _many(agent, which, heads, states, taus):
    acts = agent._act_host_many(which, heads, states, np.stack(taus))
    assert agent.__dict__.get("_iqn_act_many_ok") is True, "the batched entry was refused: this is the loop"
    return agent._q_out[: len(heads)].cpu().numpy().copy(), np.asarray(acts)


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


def _assert_rows(name, which, heads, q, acts, first=0, salt=0):
    assert q.shape[0] == len(heads) and acts.shape == (len(heads),)
    for e, k in enumerate(heads):
        q1, a1 = _reference(name, which, k, first + e, salt)
        assert q[e].tobytes() == q1.tobytes(), (name, which, heads, e, q[e], q1)
        assert int(acts[e]) == a1, (name, which, heads, e)


def _run(name, which, heads, first=0, salt=0):
    agent = _shared(name)[0]
    E = len(heads)
    return _many(agent, which, heads, [_state(name, first + e) for e in range(E)], [_tau(name, first + e, salt) for e in range(E)])


def test_chunk_size_is_the_headers():
    from slimdqn import _hip

    assert SC == _hip.IQN_ACT_MANY_SC


@pytest.mark.parametrize("kind", ["all0", "all1", "alternating", "lone"])
@pytest.mark.parametrize("E", [1, 2, SC, SC + 1, 32])
@pytest.mark.parametrize("name", ["iqn_small", "iqn_small_ragged"])
def test_rows_are_the_single_state_paths_bytes(name, E, kind):
    heads = _pattern(kind, E)
    for which in (0, 1):
        q, acts = _run(name, which, heads)
        _assert_rows(name, which, heads, q, acts)


def test_atari_k5_seven_states_five_heads():
    """F = 7744 (row groups that do not divide evenly), J = 512, N = 32, groups of 2, 2, 1, 1, 1 states."""
    heads = [0, 4, 2, 2, 0, 3, 1]
    q, acts = _run("iqn_atari_k5", 0, heads)
    _assert_rows("iqn_atari_k5", 0, heads, q, acts)


def test_atari_n64_three_states():
    """N = 64: two fraction tiles per state (MT = 2), a group of two states and a lone one."""
    heads = [1, 0, 1]
    q, acts = _run("atari_n64", 1, heads)
    assert q.shape == (3, 6)
    _assert_rows("atari_n64", 1, heads, q, acts)


def _oracle_inputs(seed=SEED):
    """iqn_small: both parameter sets, 6 states each on heads [0, 1, 1, 0, 1, 0] with fractions of the seed."""
    name = "iqn_small"
    obs, A, feats, K, N, p, pt, states = _ccase(name)
    out = []
    for which in (0, 1):
        rng = np.random.default_rng([seed, 23, which])
        heads = [0, 1, 1, 0, 1, 0]
        sts = [np.asarray(states[(3 * which + e) % len(states)]) for e in range(6)]
        out.append((which, heads, sts, [rng.random(N).astype(np.float32) for _ in range(6)]))
    return out


def _oracle(seed=SEED):
    """[(which, [(action, Q, relative top-two gap) per row])] from the fp64 oracle alone."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    obs, A, feats, K, N, p, pt, states = _ccase("iqn_small")
    res = []
    for which, heads, sts, taus in _oracle_inputs(seed):
        rows = []
        for k, s, tau in zip(heads, sts, taus):
            act, want = I.greedy_action(Q.head(pt if which else p, k), s, tau)
            top = np.sort(want)[::-1]
            rows.append((act, want, (top[0] - top[1]) / max(1.0, np.abs(want).max())))
        res.append((which, rows))
    return res


def test_rows_against_the_oracle():
    agent = _shared("iqn_small")[0]
    for (which, heads, sts, taus), (_, rows) in zip(_oracle_inputs(), _oracle()):
        for act, want, gap in rows:
            assert gap > 1e-4, f"seed {SEED} leaves a gap of {gap}: pick another one"
        q, acts = _many(agent, which, heads, sts, taus)
        for e, (act, want, gap) in enumerate(rows):
            err = np.abs(q[e] - want).max() / max(1.0, np.abs(want).max())
            print(f"which={which} row {e} head={heads[e]}: |q - oracle| = {err:.3g} x scale")
            assert err <= 2e-6, (which, e, q[e], want)
            assert int(acts[e]) == act


def test_graph_is_reused_with_new_inputs():
    """Two calls with the same buffers (one instantiated graph) but other states, heads, fractions and parameter set: the
    second call's rows are the single-state path's on ITS inputs -- table and fractions travel as data."""
    name = "iqn_small"
    first = _run(name, 0, [0, 0, 1, 0, 1])
    heads2 = [1, 1, 0, 1, 1]
    q2, acts2 = _run(name, 1, heads2, first=10, salt=1)
    _assert_rows(name, 1, heads2, q2, acts2, first=10, salt=1)
    assert first[0].tobytes() != q2.tobytes()


SWITCH_CHILD = r"""
import json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import numpy as np
import test_gpu_iqn_act_many as T
T.test_graph_is_reused_with_new_inputs()
T.test_atari_k5_seven_states_five_heads()
T.test_atari_n64_three_states()
out = [T._run("iqn_small", 0, [0, 0, 1, 0, 1]), T._run("iqn_small", 1, [1, 1, 0, 1, 1], first=10, salt=1),
       T._run("iqn_atari_k5", 0, [0, 4, 2, 2, 0, 3, 1]), T._run("atari_n64", 1, [1, 0, 1])]
print("RESULT" + json.dumps([[q.view(np.uint32).tolist(), a.tolist()] for q, a in out]))
"""


@pytest.mark.parametrize("switch", ["IDQN_ACT_GRAPH", "IDQN_ACT_POLL"])
def test_graph_reuse_and_atari_with_the_switch_off(switch):
    """IDQN_ACT_GRAPH=0 (eager launches) and IDQN_ACT_POLL=0 (device-to-host copy + synchronise), each read once per process:
    the graph-reuse test and both Atari cases (N = 32 and N = 64) in a fresh child process, and the bytes of this (default) process."""
    env = dict(os.environ)
    env[switch] = "0"
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SWITCH_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    child = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][len("RESULT"):])
    here = [_run("iqn_small", 0, [0, 0, 1, 0, 1]), _run("iqn_small", 1, [1, 1, 0, 1, 1], first=10, salt=1),
            _run("iqn_atari_k5", 0, [0, 4, 2, 2, 0, 3, 1]), _run("atari_n64", 1, [1, 0, 1])]
    assert [[q.view(np.uint32).tolist(), a.tolist()] for q, a in here] == child


def test_ties_give_the_first_maximum():
    import torch

    name = "iqn_small"
    agent = _agent(name)
    agent.params["params"]["Dense_1"]["kernel"].zero_()
    agent.params["params"]["Dense_1"]["bias"].zero_()
    torch.cuda.synchronize()
    q, acts = _many(agent, 0, [0, 1, 1, 0, 1], [_state(name, e) for e in range(5)], [_tau(name, e) for e in range(5)])
    assert (q == 0).all() and acts.tolist() == [0] * 5


def _c_call(agent, which, heads, pin, tau_pin, n, q_out, acts):
    from slimdqn import _hip

    h = None if heads is None else np.ascontiguousarray(np.asarray(heads, np.int32))
    return _hip.lib().idqn_iqn_act_host_many(agent._handle, which, None if h is None else h.ctypes.data,
                                             None if pin is None else C.c_void_p(pin.data_ptr()),
                                             None if tau_pin is None else C.c_void_p(tau_pin.data_ptr()), n, _hip.ptr(q_out),
                                             None if acts is None else C.c_void_p(acts.data_ptr()), _hip.current_stream())


def _refusal_buffers(agent, name, N):
    import torch

    pin = torch.empty((33, int(np.prod(agent._obs))), dtype=torch.uint8).pin_memory()
    tau_pin = torch.empty((33, N), dtype=torch.float32).pin_memory()
    for i in range(33):
        pin[i] = torch.from_numpy(np.ascontiguousarray(_state(name, i)).reshape(-1))
        tau_pin[i] = torch.from_numpy(_tau(name, i))
    q_out = torch.full((33, agent.network.n_actions), -123.0, dtype=torch.float32, device="cuda")
    acts = torch.full((40,), -9, dtype=torch.int32).pin_memory()
    return pin, tau_pin, q_out, acts


def _assert_untouched(q_out, acts):
    import torch

    torch.cuda.synchronize()
    assert (q_out.cpu().numpy() == -123.0).all() and (acts.numpy() == -9).all(), "a refused call enqueued work"


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    name = "iqn_small"
    agent, (obs, A, feats, K, N, p, pt, states) = _shared(name)
    agent._ensure_handle(32)
    pin, tau_pin, q_out, acts = _refusal_buffers(agent, name, N)
    lib = _hip.lib()
    for which, heads, n in ((0, [0], 0), (0, [0] * 33, 33), (0, [0, K, 0], 3), (0, [0, -1], 2), (2, [0, 1], 2)):
        assert _c_call(agent, which, heads, pin, tau_pin, n, q_out, acts) == _hip.E_INVALID, (which, heads, n)
        _assert_untouched(q_out, acts)
    # each null pointer
    for bad in ((None, pin, tau_pin, q_out, acts), ([0, 1], None, tau_pin, q_out, acts), ([0, 1], pin, None, q_out, acts),
                ([0, 1], pin, tau_pin, None, acts), ([0, 1], pin, tau_pin, q_out, None)):
        heads, b_pin, b_tau, b_q, b_acts = bad
        assert _c_call(agent, 0, heads, b_pin, b_tau, 2, b_q, b_acts) == _hip.E_INVALID
        _assert_untouched(q_out, acts)
    assert lib.idqn_iqn_act_host_many(None, 0, np.zeros(2, np.int32).ctypes.data, C.c_void_p(pin.data_ptr()),
                                      C.c_void_p(tau_pin.data_ptr()), 2, _hip.ptr(q_out), C.c_void_p(acts.data_ptr()),
                                      _hip.current_stream()) == _hip.E_INVALID
    _assert_untouched(q_out, acts)
    # an idqn_iqn_act_host_begin that nobody has collected yet
    one_out = acts[36:]
    _hip.check(lib.idqn_iqn_act_host_begin(agent._handle, 0, 0, C.c_void_p(pin[0].data_ptr()), C.c_void_p(tau_pin[0].data_ptr()),
                                           _hip.ptr(q_out[32:]), C.c_void_p(one_out.data_ptr()), _hip.current_stream()),
               "idqn_iqn_act_host_begin")
    assert _c_call(agent, 0, [0, 1], pin, tau_pin, 2, q_out, acts) == _hip.E_INVALID
    _hip.check(lib.idqn_act_host_end(agent._handle, C.c_void_p(one_out.data_ptr()), _hip.current_stream()), "idqn_act_host_end")
    torch.cuda.synchronize()
    assert (q_out[:32].cpu().numpy() == -123.0).all() and (acts[:32].numpy() == -9).all()
    # a valid call after the refusals is correct and writes only its n rows
    heads = [1, 0, 0, 1]
    assert _c_call(agent, 1, heads, pin, tau_pin, 4, q_out, acts) == 0
    q = q_out[:4].cpu().numpy()
    for e, k in enumerate(heads):
        q1, a1 = _reference(name, 1, k, e)
        assert q[e].tobytes() == q1.tobytes() and int(acts[e]) == a1
    assert (acts[4:32].numpy() == -9).all() and (q_out[4:32].cpu().numpy() == -123.0).all()
    # a handle without quantile heads
    dqn = iDQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    dqn._ensure_handle(32)
    q_out.fill_(-123.0)
    acts.fill_(-9)
    assert _c_call(dqn, 0, [0, 1], pin, tau_pin, 2, q_out, acts) == _hip.E_INVALID
    _assert_untouched(q_out, acts)


def test_no_residue_on_the_handle():
    """A handle that has run idqn_iqn_act_host_many with E = 3 and E = 32 and a fresh one, from the same state and inputs: a
    learn step, an idqn_iqn_act_host call and a q_values call give the same bytes, parameters and Adam state included."""
    import torch

    from oracle import make_golden as G

    name = "iqn_small"
    used, fresh = _agent(name), _agent(name)
    batch = G.iqn_case_inputs(name)[2]
    _many(used, 0, [1, 0, 1], [_state(name, e) for e in range(3)], [_tau(name, e) for e in range(3)])
    _many(used, 1, [0] * 32, [_state(name, e) for e in range(32)], [_tau(name, e) for e in range(32)])
    out = []
    for agent in (used, fresh):
        losses = agent._learn(Batch(*batch)).cpu().numpy().copy()
        q1, a1 = _single(agent, 0, 1, _state(name, 4), _tau(name, 4))
        qn = agent.q_values(agent.target_params, batch[0][:5], 0, taus=np.stack([_tau(name, e) for e in range(5)], 1)).cpu().numpy().copy()
        torch.cuda.synchronize()
        out.append((losses, agent._online.cpu().numpy(), agent._mu.cpu().numpy(), agent._nu.cpu().numpy(), q1, np.asarray([a1]), qn))
    for x, y in zip(*out):
        assert x.tobytes() == y.tobytes()


def test_public_path_draws_head_and_fractions_from_each_key():
    """iIQN.best_actions is [best_action(params, s, k).item()] in ONE call, select_actions on top of it equals select_action per
    environment, and keyed calls leave the training stream of fractions alone."""
    from slimdqn import prng
    from slimdqn.sample_collection.utils import select_action, select_actions

    name = "iqn_small"
    agent, (obs, A, feats, K, N, p, pt, states) = _shared(name)
    hosts = [_state(name, e) for e in range(9)]
    keys = prng.split(prng.PRNGKey(77), 9)
    assert len({prng.randint(k, 0, K) for k in keys}) == K
    before = json.dumps(agent._tau_rng.bit_generator.state, default=str)
    got = agent.best_actions(agent.target_params, hosts, keys)
    assert agent.__dict__.get("_iqn_act_many_ok") is True, "the batched entry was refused: this is the loop"
    rows = agent._q_out[:9].cpu().numpy().copy()
    assert got.dtype == np.int64
    for i in range(9):
        a1 = int(agent.best_action(agent.target_params, hosts[i], keys[i]).item())
        assert int(got[i]) == a1
        assert rows[i].tobytes() == agent._q_out[0].cpu().numpy().tobytes()
    eps = lambda n: 0.3  # noqa: E731
    want = [select_action(agent.best_action, agent.params, s, k, A, eps, 0).item() for s, k in zip(hosts, keys)]
    assert select_actions(agent.best_actions, agent.params, hosts, keys, A, eps, 0) == want
    assert json.dumps(agent._tau_rng.bit_generator.state, default=str) == before


if __name__ == "__main__":  # the gaps of a seed, from the oracle alone (no GPU): python tests/test_gpu_iqn_act_many.py [seed]
    sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    print(seed, "iqn_small", "smallest gap", min(g for _, rows in _oracle(seed) for _, _, g in rows))
