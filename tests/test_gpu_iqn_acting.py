"""GPU checks of the single-state i-IQN acting path (``idqn_iqn_act_host`` / ``_begin``, csrc/iqn_act_kernels.h) -- an
extension like the rest of i-IQN: the fp64 oracle is ``oracle.iqn_ref.greedy_action``.

Bars: Q-values within 2e-6 * max(1, max|want|) of the oracle (the bar ``test_gpu_iqn.py::test_iqn_acting_against_oracle``
holds the batched route to), hence within 4e-6 of the batched route; the action equals the oracle's.  The inputs come from
``SEED``, picked on the CPU with the oracle alone (``python tests/test_gpu_iqn_acting.py`` prints the gaps of a seed) so
that the oracle's two largest Q-values are more than 1e-4 * max(1, max|want|) apart in every case -- 50 times the bar, so
the action is decided; the test asserts that gap first.  Replays, begin / end and the trainer loop are compared bit for bit.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0
ATARI = ((84, 84, 4), 6, [32, 64, 64, 512])
# name: (obs, A, features, K, N) -- the three golden cases' parameters, plus Atari-shaped agents with N = 64 and N = 1
EXTRA = {"atari_n64": ATARI + (2, 64), "atari_n1": ATARI + (2, 1)}
CASES = ["iqn_small", "iqn_small_ragged", "iqn_atari_k5", "atari_n64", "atari_n1"]


def _case(name):
    """(obs, A, feats, K, N, online params, target params, states [>= 4])"""
    from oracle import iqn_ref as I
    from oracle import make_golden as G
    from oracle import qnet_ref as Q

    if name in G.IQN_CASES:
        obs, A, feats, K, B, N = G.IQN_CASES[name]
        p, pt, batch, _ = G.iqn_case_inputs(name)
        return obs, A, feats, K, N, p, pt, batch[0]
    obs, A, feats, K, N = EXTRA[name]
    seed = sum(name.encode())
    p, pt = I.init_params(seed, obs, A, feats, K), I.init_params(seed + 1, obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    return obs, A, feats, K, N, p, pt, Q.synthetic_batch(seed + 10, 8, obs, A, "cnn")[0]


def _calls(name, seed=SEED):
    """Every head of both arenas on two states each, fresh fractions: [(which, head, state, tau [N])]."""
    obs, A, feats, K, N, p, pt, states = _case(name)
    rng = np.random.default_rng([seed, sum(name.encode())])
    out = []
    for which in (0, 1):
        for head in range(K):
            for j in range(2):
                state = states[(2 * head + j + which) % len(states)]
                out.append((which, head, state, rng.random(N).astype(np.float32)))
    return out


def _oracle(name, seed=SEED):
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    obs, A, feats, K, N, p, pt, states = _case(name)
    res = []
    for which, head, state, tau in _calls(name, seed):
        act, want = I.greedy_action(Q.head(pt if which else p, head), state, tau)
        top = np.sort(want)[::-1]
        res.append((act, want, (top[0] - top[1]) / max(1.0, np.abs(want).max())))
    return res


def _agent(name, lazy=False):
    from slimdqn.networks.iiqn import iIQN

    obs, A, feats, K, N, p, pt, _ = _case(name)
    agent = iIQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    agent.lazy_host_actions = lazy
    return agent


def _act(agent, which, head, state, tau):
    """One call of the host route: (action, Q-values [A] as the library left them in q_out_dev)."""
    act = agent._act_host(which, head, np.asarray(state), tau, None)
    return int(act.item()), agent._q_out[0].cpu().numpy().copy()


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_oracle_and_the_device_route(name):
    agent = _agent(name)
    for (which, head, state, tau), (want_act, want, gap) in zip(_calls(name), _oracle(name)):
        assert gap > 1e-4, f"seed {SEED} leaves a gap of {gap} in {name}: pick another one"
        scale = max(1.0, np.abs(want).max())
        act, q = _act(agent, which, head, state, tau)
        err = np.abs(q - want).max() / scale
        print(f"{name} which={which} head={head}: |q - oracle| = {err:.3g} x scale")
        assert err <= 2e-6, (name, which, head, q, want)
        assert act == want_act
        arena = agent.target_params if which else agent.params
        qd = agent.q_values(arena, state, head, taus=tau[:, None]).cpu().numpy()[0]
        assert np.abs(q - qd).max() <= 4e-6 * max(1.0, np.abs(qd).max()), (name, which, head, q, qd)


@pytest.mark.parametrize("name", ["iqn_small_ragged", "iqn_atari_k5", "atari_n64"])
def test_replay_is_bit_identical(name):
    """Calls 2.. of one agent replay captured graphs, alternating heads, arenas, states and fractions; each must give the bits
    of the FIRST call of a fresh agent on the same inputs (a capture followed by its first launch), and those of a process
    that runs with IDQN_ACT_GRAPH=0 and so issues every launch eagerly."""
    calls = _calls(name)
    order = [0, len(calls) - 1, 1, len(calls) // 2, 0, len(calls) - 1, 2][: 7 if name == "iqn_small_ragged" else 5]
    agent = _agent(name)
    got = [_act(agent, *calls[i]) for i in order]
    for i, (act, q) in zip(order[1:], got[1:]):
        fresh = _agent(name)
        act1, q1 = _act(fresh, *calls[i])
        assert act == act1 and q.tobytes() == q1.tobytes(), (name, i)
        del fresh
    code = (f"import sys, os, json\nsys.path[:0] = [{ROOT!r}, os.path.join({ROOT!r}, 'i-dqn_amd'), os.path.join({ROOT!r}, 'tests')]\n"
            f"import test_gpu_iqn_acting as T\nagent = T._agent({name!r})\ncalls = T._calls({name!r})\n"
            f"out = [T._act(agent, *calls[i]) for i in {order!r}]\n"
            "print('RESULT' + json.dumps([[a, q.view('uint32').tolist()] for a, q in out]))\n")
    env = dict(os.environ, IDQN_ACT_GRAPH="0")
    env.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    eager = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][6:])
    assert [[a, q.view(np.uint32).tolist()] for a, q in got] == eager


def test_begin_end_and_refusals():
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    name = "iqn_small"
    calls = _calls(name)
    sync = _agent(name)
    want = [_act(sync, *c) for c in calls[:4]]
    lazy = _agent(name, lazy=True)
    lib = _hip.lib()
    for (which, head, state, tau), (act, q) in zip(calls[:4], want):
        pending = lazy._act_host(which, head, np.asarray(state), tau, None)
        assert type(pending).__name__ == "_PendingHostAction"
        args = (lazy._handle, which, head, C.c_void_p(lazy._act_pin.data_ptr()), C.c_void_p(lazy._act_tau_pin.data_ptr()),
                _hip.ptr(lazy._q_out), C.c_void_p(lazy._act_out.data_ptr()), _hip.current_stream())
        # a second launch of either kind while one is pending: refused with the library's message, nothing enqueued
        with pytest.raises(_hip.HipExtensionError, match="already pending"):
            _hip.check(lib.idqn_iqn_act_host_begin(*args), "idqn_iqn_act_host_begin")
        with pytest.raises(_hip.HipExtensionError, match="pending"):
            _hip.check(lib.idqn_iqn_act_host(*args), "idqn_iqn_act_host")
        with pytest.raises(_hip.HipExtensionError, match="pending"):
            _hip.check(lib.idqn_act_host_begin(*(args[:4] + args[5:])), "idqn_act_host_begin")
        assert pending.item() == act and lazy._q_out[0].cpu().numpy().tobytes() == q.tobytes()
    # argument checks
    args = (lazy._handle, 0, 0, C.c_void_p(lazy._act_pin.data_ptr()), C.c_void_p(lazy._act_tau_pin.data_ptr()),
            _hip.ptr(lazy._q_out), C.c_void_p(lazy._act_out.data_ptr()), _hip.current_stream())
    for fn in (lib.idqn_iqn_act_host, lib.idqn_iqn_act_host_begin):
        for bad, pat in (((args[0], 2) + args[2:], "bad head / which"), (args[:2] + (lazy._K,) + args[3:], "bad head / which"),
                         (args[:2] + (-1,) + args[3:], "bad head / which"), (args[:4] + (None,) + args[5:], "null pointer"),
                         (args[:3] + (None,) + args[4:], "null pointer"), (args[:5] + (None,) + args[6:], "null pointer"),
                         (args[:6] + (None,) + args[7:], "null pointer")):
            with pytest.raises(_hip.HipExtensionError, match=pat):
                _hip.check(fn(*bad), "idqn_iqn_act_host")
    assert _act(lazy, *calls[0])[1].tobytes() == want[0][1].tobytes()  # (nothing was left pending by the refusals)
    # an uncollected action does not get in the way of the next call, nor of the agent's destruction
    lazy._act_host(calls[1][0], calls[1][1], np.asarray(calls[1][2]), calls[1][3], None)
    assert _act(lazy, *calls[2])[1].tobytes() == want[2][1].tobytes()
    lazy._act_host(calls[3][0], calls[3][1], np.asarray(calls[3][2]), calls[3][3], None)
    lazy._destroy_handle()
    assert lazy._act_in_flight is None
    del lazy
    # a handle without quantile heads refuses the entries
    obs, A, feats, K, N, p, pt, states = _case(name)
    dqn = iDQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    dqn.best_action(dqn.params, states[0], 3)  # (builds the handle and its pinned buffers)
    tau = np.full(4, 0.5, np.float32)
    import torch

    tau_pin = torch.from_numpy(tau).pin_memory()
    dargs = (dqn._handle, 0, 0, C.c_void_p(dqn._act_pin.data_ptr()), C.c_void_p(tau_pin.data_ptr()), _hip.ptr(dqn._q_out),
             C.c_void_p(dqn._act_out.data_ptr()), _hip.current_stream())
    for fn in (lib.idqn_iqn_act_host, lib.idqn_iqn_act_host_begin):
        with pytest.raises(_hip.HipExtensionError, match="without quantile heads"):
            _hip.check(fn(*dargs), "idqn_iqn_act_host")


def test_keys_decide_head_and_fractions():
    import torch

    from slimdqn import prng

    name = "iqn_small"
    agent = _agent(name)
    obs, A, feats, K, N, p, pt, states = _case(name)
    before = json.dumps(agent._tau_rng.bit_generator.state, default=str)
    for key in (3, 11, 12345):
        a1 = agent.best_action(agent.params, states[1], key)
        q1 = agent._q_out[0].cpu().numpy().copy()
        a2 = agent.best_action(agent.params, states[1], key)
        assert type(a1).__name__ == "_HostAction" and a1.item() == a2.item()
        assert q1.tobytes() == agent._q_out[0].cpu().numpy().tobytes()
        tau_host = agent._act_tau_np.copy()
        # the device-state route draws the same head and the same fractions for that key
        a3 = agent.best_action(agent.params, torch.as_tensor(states[1]).cuda(), key)
        want_tau = prng.generator(prng.split(key, 2)[1]).random((N, 1)).astype(np.float32)
        assert np.array_equal(tau_host, want_tau[:, 0])
        assert np.array_equal(agent._tau_act[:N].cpu().numpy(), want_tau[:, 0])
        head = prng.randint(key, 0, K)
        qd = agent.q_values(agent.params, states[1], head, taus=want_tau).cpu().numpy()[0]
        assert np.abs(q1 - qd).max() <= 4e-6 * max(1.0, np.abs(qd).max())
        assert int(a3.item()) == int(qd.argmax())
    assert json.dumps(agent._tau_rng.bit_generator.state, default=str) == before  # keyed acting leaves the training stream alone
    fresh = _agent(name)
    assert np.array_equal(agent.sample_fractions(32), fresh.sample_fractions(32))


TRAINER_CHILD = r"""
import json, sys, os, tempfile
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
import numpy as np
from slimdqn.networks import _agent as A
from slimdqn.networks.iiqn import iIQN
from experiments.atari.iiqn import run
n = {"pending": 0, "greedy": 0, "collected": 0}
init, item, best = A._PendingHostAction.__init__, A._PendingHostAction.item, iIQN.best_action
def count_init(self, agent):
    n["pending"] += 1
    init(self, agent)
def count_item(self):
    n["collected"] += self._value is None
    return item(self)
def count_best(self, *a, **k):
    n["greedy"] += 1
    out = best(self, *a, **k)
    n["lazy"] = n.get("lazy", 0) + isinstance(out, A._PendingHostAction)
    return out
A._PendingHostAction.__init__, A._PendingHostAction.item, iIQN.best_action = count_init, count_item, count_best
argv = ["-en", "g", "-s", "3", "-ne", "1", "-ntspe", "300", "-nis", "40", "-rbc", "400", "-nn", "2", "-at", "cnn",
        "-tuf", "20", "-tsf", "5", "-f", "32", "64", "64", "512", "-horizon", "60", "-bs", "32", "-nq", "8", "-ed", "100"]
p, agent = run(argv, save_root=tempfile.mkdtemp())
flat = agent._flat(agent._online)
probe = {name: v.reshape(2, -1)[:, :: max(1, v[0].size // 61)].astype(np.float64).tolist() for name, v in flat.items()}
print("RESULT" + json.dumps({"probe": probe, "count": int(agent._count[0].item()), "n": n,
                             "losses": np.asarray(agent.cumulated_losses, np.float64).tolist()}))
"""


def _trainer(**env):
    e = dict(os.environ)
    e.update(env)
    e.pop("IDQN_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + TRAINER_CHILD], env=e, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][6:])


def test_trainer_loop_with_and_without_overlap():
    """The Atari-shaped synthetic i-IQN trainer (experiments/atari/iiqn.py, the launcher's defaults) with the replay bookkeeping
    under the acting launch and with IDQN_LOOP_OVERLAP=0: same transitions, same steps -- bit-identical losses and parameters;
    in the default run every greedy action came back through a pending action."""
    a, b = _trainer(IDQN_LOOP_OVERLAP="1"), _trainer(IDQN_LOOP_OVERLAP="0")
    assert a["count"] == b["count"] and a["count"] >= 100
    assert a["losses"] == b["losses"]
    assert a["probe"] == b["probe"]
    assert a["n"]["greedy"] > 0 and a["n"]["lazy"] == a["n"]["greedy"] == a["n"]["pending"] == a["n"]["collected"], a["n"]
    assert b["n"]["greedy"] == a["n"]["greedy"] and b["n"]["pending"] == 0, b["n"]


if __name__ == "__main__":  # the gaps of a seed, from the oracle alone (no GPU): python tests/test_gpu_iqn_acting.py [seed]
    sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else SEED
    for name in CASES:
        print(seed, name, "smallest gap", min(g for _, _, g in _oracle(name, seed)))
