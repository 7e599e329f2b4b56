"""The three many-state acting entries (``idqn_act_host_many``, ``idqn_act_host_many_fc``, ``idqn_iqn_act_host_many``) share
one slot on the handle, one driver and one mailbox wait with each other, and the wait with the single-state path
(csrc/qnet.hip: ``ActManySlot``, ``act_many_run``, ``mailbox_wait``).  One sequence per kind of handle, in the default mode
(graph + poll), interleaves many-state calls of different n with single-state calls: both mailboxes (sequence number at
index 1 and at index 32) and their counters advance independently, and the finished-workgroup count returns to zero between
calls of different n.  The criterion is the one of ``tests/test_gpu_act_many.py``: row e and action e of a call are the BYTES
the single-state path gives on the same handle for ``(which, heads[e], state e)``, and nothing beyond n is written.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]

pytestmark = pytest.mark.gpu
Q_SENTINEL, A_SENTINEL = -123.0, -9


def _setup(name):
    """(agent, K, entry, state(e), tau(e) or None) of a fresh agent."""
    if name == "cnn_small":
        import test_gpu_act_many as T

        agent, arch, A, K, p, pt, batch = T._make(name)
        return agent, K, "idqn_act_host_many", lambda e: np.asarray(batch[0][e]), None
    if name == "iqn_small":
        import test_gpu_iqn_act_many as T

        return T._agent(name), T._ccase(name)[3], "idqn_iqn_act_host_many", lambda e: T._state(name, e), lambda e: T._tau(name, e)
    import test_gpu_fc_act_many as T

    agent, p, pt, states = T._make(name)
    return agent, T.CASES[name][3], "idqn_act_host_many_fc", lambda e: np.asarray(states[e]), None


def _single(agent, which, head, state, tau, lazy=False):
    """(Q row, action) of the single-state path: one blocking call, or a begin / end pair."""
    agent.lazy_host_actions = lazy
    act = agent._best_action(which, head, state) if tau is None else agent._act_host(which, head, state, tau, None)
    act = int(act.item())  # (lazy: idqn_act_host_end)
    agent.lazy_host_actions = False
    return agent._q_out[0].cpu().numpy().copy(), act


class _Buffers:
    """Pinned states (and fractions), device Q rows and pinned actions of the caller: 33 rows, 40 action slots."""

    def __init__(self, agent, tau):
        import torch

        dt = torch.uint8 if agent._arch == "cnn" else torch.float32
        self.pin = torch.zeros((33, int(np.prod(agent._obs))), dtype=dt).pin_memory()
        self.tau = torch.zeros((33, agent._n_quantiles), dtype=torch.float32).pin_memory() if tau else None
        self.q_out = torch.empty((33, agent.network.n_actions), dtype=torch.float32, device="cuda")
        self.acts = torch.empty((40,), dtype=torch.int32).pin_memory()


def _many(agent, entry, buf, which, heads, first, state, tau):
    """One C call on buf for states first .. first + n - 1: (Q rows [n], actions [n]) after the sentinels were checked."""
    import torch

    from slimdqn import _hip

    n = len(heads)
    for e in range(n):
        buf.pin[e] = torch.from_numpy(np.ascontiguousarray(state(first + e)).reshape(-1))
        if tau:
            buf.tau[e] = torch.from_numpy(tau(first + e))
    buf.q_out.fill_(Q_SENTINEL)
    buf.acts.fill_(A_SENTINEL)
    torch.cuda.synchronize()
    h = np.ascontiguousarray(np.asarray(heads, np.int32))
    args = [agent._handle, which, h.ctypes.data, C.c_void_p(buf.pin.data_ptr())]
    args += [C.c_void_p(buf.tau.data_ptr())] if tau else []
    args += [n, _hip.ptr(buf.q_out), C.c_void_p(buf.acts.data_ptr()), _hip.current_stream()]
    _hip.check(getattr(_hip.lib(), entry)(*args), entry)
    acts = buf.acts.numpy().copy()  # (the call has returned: the actions are there without a synchronisation)
    q = buf.q_out.cpu().numpy()
    assert (q[n:] == Q_SENTINEL).all() and (acts[n:] == A_SENTINEL).all(), (entry, n)
    return q[:n].copy(), acts[:n]


@pytest.mark.parametrize("name", ["cnn_small", "iqn_small", "lunar", "gc_small"])
def test_interleaved_calls_are_the_single_state_paths_bytes(name):
    agent, K, entry, state, tau = _setup(name)
    agent._ensure_handle(32)
    a, b = _Buffers(agent, tau), _Buffers(agent, tau)
    t = tau or (lambda e: None)
    # (kind, buffers, which, heads, first state); a many-state call is the FIRST thing the handle does
    steps = [("many", a, 0, [(e + 1) % K for e in range(3)], 0),
             ("single", None, 1, [K - 1], 3),
             ("many", b, 1, [e % K for e in range(32)], 0),
             ("many", b, 0, [K - 1], 5),
             ("begin_end", None, 0, [0], 6),
             ("many", a, 1, [0, K - 1], 7)]  # n = 2 on the n = 3 call's buffers
    got = []
    for kind, buf, which, heads, first in steps:
        if kind == "many":
            got.append(_many(agent, entry, buf, which, heads, first, state, tau))
        else:
            q, act = _single(agent, which, heads[0], state(first), t(first), lazy=kind == "begin_end")
            got.append((q[None], np.asarray([act])))
    # the single-state path on the same handle, afterwards: the sequence above is not interleaved with its own reference
    for (kind, buf, which, heads, first), (q, acts) in zip(steps, got):
        assert q.shape[0] == len(heads) and acts.shape == (len(heads),)
        for e, k in enumerate(heads):
            q1, a1 = _single(agent, which, k, state(first + e), t(first + e))
            assert q[e].tobytes() == q1.tobytes(), (name, kind, which, heads, e, q[e], q1)
            assert int(acts[e]) == a1, (name, kind, which, heads, e)
            # the action is the first maximum of the row that was written, whichever mailbox delivered it
            assert int(acts[e]) == int(np.argmax(q[e])), (name, kind, which, heads, e, q[e])
