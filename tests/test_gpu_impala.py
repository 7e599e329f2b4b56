"""The impala architecture on the device (csrc/impala_kernels.h) against the fp64 oracle, row by row of tests/impala_shapes.py:
per-head loss and every leaf gradient, Q-values of both nets, the greedy action, the pool and Stack outputs, three chained
full steps (parameters and both Adam moments), a weighted step with |TD|; then byte identities (two fresh handles, the
replay-sourced step on both rings, PrioritizedLearner), ``best_actions`` against the loop, the refusing entries, and the
trainer as a script.  Reference: slimdqn/networks/architectures/dqn.py:7-29,54-60, slimdqn/networks/idqn.py:96-131.

Bars (tests/test_gpu_general_shapes.py): loss 1e-5 max(1, |loss|), gradients 2e-5 of the leaf's largest magnitude,
Q-values 1e-5.  A leaf that misses 2e-5 is held to 4 x the error of the float32 torch_ref run against the fp64 one on the
same inputs (impala_shapes.f32_errors), computed here, not chosen.

Row ``workload`` is the one that tells the conv's summation order: in fp64, head 0's Stack-1 pool has a window whose two largest
inputs are 5.7e-7 apart at a value of 0.80 (nine float32 ulps), and a conv that sums its 288 products as one running fma chain
picks the runner-up there, which moves ``Stack_1/Conv_0/kernel``'s gradient by 6.0e-3 and Stack 0's leaves by up to 4.0e-3 of
their largest magnitudes.  k_imp_conv sums each 72-product LDS pass on its own; the row's worst leaf is
then 3.4e-6 from the oracle.
"""
import ctypes as C
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import impala_shapes as S

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(S.ROWS)


def _agent(name):
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = iDQN(0, obs, A, K, feats, "impala", S.LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=S.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _batch(name):
    return Batch(*[np.array(a) for a in S.case(name)[7]])


def _grad_bar(name, k, leaf):
    return max(2e-5, 4 * S.f32_errors(name)[k][1][leaf])


@pytest.mark.parametrize("name", NAMES)
def test_row_against_the_oracle(name):
    from oracle import qnet_ref as Q
    from slimdqn import _hip

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    want = S.oracle(name)
    agent = _agent(name)
    assert [n for n, _, _ in agent._leaves] == [n for n, _ in Q.leaf_shapes("impala", obs, A, feats)]
    assert agent.params["params"]["Stack_2"]["Conv_4"]["kernel"].shape == (K, 3, 3, feats[2], feats[2])
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    G = agent._flat_grad()
    n32 = min(B, 32)
    for k in range(K):
        w = want[k]
        print(name, k, "loss", losses[k], w["loss"])
        assert abs(losses[k] - w["loss"]) <= 1e-5 * max(1.0, abs(w["loss"])), (k, losses[k], w["loss"])
        errs = {leaf: np.abs(G[leaf][k] - g).max() / (np.abs(g).max() + 1e-300) for leaf, g in w["grads"].items()}
        for leaf, err in errs.items():  # every figure first, then the bars
            print(name, k, leaf, "relative gradient error", err, "bar", _grad_bar(name, k, leaf))
        for leaf, err in errs.items():
            assert err <= _grad_bar(name, k, leaf), (leaf, err)
        # activations of the step just run: nets [online 0..K-1 | target 0..K-1] x B samples
        for which in (0, 1):
            pools, stacks = S.stack_outputs(name, k, which)
            for si in range(3):
                for nm, ref in (("imp_pool%d" % si, pools[si]), ("imp_stack%d" % si, stacks[si])):
                    got = agent._debug(nm).cpu().numpy()[(which * K + k) * ref.size : (which * K + k + 1) * ref.size].reshape(ref.shape)
                    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (nm, which, np.abs(got - ref).max())
        q = agent.q_values(agent.params, batch[0][:n32], k).cpu().numpy()
        assert np.abs(q - w["q"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q"]).max())
        qt = agent.q_values(agent.target_params, batch[3][:n32], k).cpu().numpy()
        assert np.abs(qt - w["q_next"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q_next"]).max())
        row = np.sort(w["q"][1])
        if row[-1] - row[-2] > 1e-4:  # (a near-tie of the oracle's own row decides nothing)
            assert int(agent._best_action(0, k, np.asarray(batch[0][1]))) == int(np.argmax(w["q"][1]))  # host state: idqn_act_host


@pytest.mark.parametrize("name", NAMES)
def test_three_chained_steps(name):
    """Parameters and both Adam moments after three full steps, against the oracle's gradients of the device's own
    parameters at each step (so an Adam sign flip of a tiny gradient cannot compound): as test_gpu_general_shapes.py does it."""
    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = _agent(name)
    b = _batch(name)
    for step in range(3):
        before = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        agent._learn(b)
        after = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        for k in range(K):
            _, grads = T.loss_and_grads(Q.head(before["_online"], k), Q.head(pt, k), batch, "impala", S.GAMMA_N)
            for leaf, g in grads.items():
                th, m, v = Q.adam_update(before["_online"][leaf][k].astype(np.float64), g, before["_mu"][leaf][k].astype(np.float64),
                                         before["_nu"][leaf][k].astype(np.float64), step, S.LR, S.EPS)
                gm = np.abs(g).max() + 1e-300
                assert np.abs(after["_mu"][leaf][k] - m).max() <= 1e-4 * gm, (step, leaf)
                assert np.abs(after["_nu"][leaf][k] - v).max() <= 1e-4 * gm * gm, (step, leaf)
                err = np.abs(after["_online"][leaf][k] - th)
                assert err.max() <= S.LR * 1.01 + 1e-6, (step, leaf)  # never more than one Adam step (lr) away
                assert np.median(err) <= 2e-5, (step, leaf, np.median(err))
    assert (agent._count.cpu().numpy() == 3).all()


@pytest.mark.parametrize("name", NAMES)
def test_weighted_step_and_td(name):
    import torch

    from slimdqn import _hip

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = _agent(name)
    wts = np.random.default_rng(5).uniform(0.2, 1.0, B).astype(np.float32)
    agent._ensure_handle(B)
    w_dev, td_dev = torch.from_numpy(wts).cuda(), torch.zeros(K * B, dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    try:
        losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    G, td = agent._flat_grad(), td_dev.cpu().numpy().reshape(K, B)
    for k in range(K):
        loss, grads, td_want = S.weighted_oracle(name, k, wts)
        assert abs(losses[k] - loss) <= 1e-5 * max(1.0, abs(loss))
        assert np.abs(td[k] - td_want).max() <= 1e-5 * max(1.0, np.abs(td_want).max())
        for leaf, g in grads.items():
            assert np.abs(G[leaf][k] - g).max() <= _grad_bar(name, k, leaf) * (np.abs(g).max() + 1e-300), leaf


@pytest.mark.parametrize("name", ["odd_even", "workload"])
def test_two_fresh_handles_give_equal_bytes(name):
    from slimdqn import _hip

    out = []
    for _ in range(2):
        agent = _agent(name)
        agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY)
        grads = agent._grad.cpu().numpy().tobytes()
        agent._learn(_batch(name))
        out.append((grads, agent._online.cpu().numpy().tobytes(), agent._mu.cpu().numpy().tobytes(), agent._nu.cpu().numpy().tobytes()))
    assert out[0] == out[1]


IMPALA_RING = ("impala", (12, 10), np.uint8, 2, (12, 10, 2), [3, 9, 4, 15], 2, 3, 5, "iDQN")


def _replay_module():
    import test_gpu_fc_learn_on_replay as R  # its buffers, seed choice and byte comparison, on a configuration of this file

    R.CONFIGS.setdefault("impala_12x10x2", IMPALA_RING)
    return R


def test_replay_sourced_step_is_gather_then_learn():
    R = _replay_module()
    fused = R._identity("impala_12x10x2", R._buffer)
    assert fused.__dict__.get("_replay_fused_ok") is None  # the plane entry was never asked


def test_replay_sourced_step_on_the_vector_ring():
    R = _replay_module()
    R._identity("impala_12x10x2", R._vector_buffer, first_slot=True)


def test_prioritized_learner_steps():
    import torch

    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    R = _replay_module()
    _, shape, dtype, stack, _, _, _, A, B, _ = IMPALA_RING

    def make(fuse):
        rb = ReplayBuffer(SlotPrioritizedSampler(4, R.CAPACITY), batch_size=B, max_capacity=R.CAPACITY, stack_size=stack,
                          update_horizon=R.HORIZON, gamma=0.99)
        rng = np.random.default_rng(17)
        for i in range(150):
            rb.add(TransitionElement(R._frame(rng, shape, dtype), int(rng.integers(A)), float(rng.normal()), i % 7 == 6, i % 7 == 6))
        rb.reuse_sample_buffers = True
        return PrioritizedLearner(R._agent("impala_12x10x2", fuse=fuse), rb)

    a, b = make(True), make(False)
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert a.__dict__.get("_fused_ok") is None  # the one-call form was not asked: the chain
    assert a.agent.__dict__.get("_replay_fc_ok") is True and b.agent.__dict__.get("_replay_fc_ok") is None
    R._assert_same(a.agent, b.agent)
    assert np.isfinite(a.agent._losses.cpu().numpy()).all() and (a.agent._count.cpu().numpy() == 3).all()
    assert a._td_abs.cpu().numpy().tobytes() == b._td_abs.cpu().numpy().tobytes()
    assert a.sampler._sum_tree._nodes_dev.cpu().numpy().tobytes() == b.sampler._sum_tree._nodes_dev.cpu().numpy().tobytes()


def test_best_actions_equals_the_loop():
    obs, feats, A, K, B, p, pt, batch = S.case("odd_even")
    agent = _agent("odd_even")
    states = [np.asarray(s) for s in list(batch[0]) + list(batch[3])][:7]
    heads = [i % K for i in range(len(states))]
    got = agent._best_actions(0, heads, states)
    rows = agent._q_out[: len(states)].cpu().numpy().copy()
    assert agent.__dict__.get("_act_many_ok") is False and agent.__dict__.get("_act_many_fc_ok") is False
    for i, (h, s) in enumerate(zip(heads, states)):
        assert int(agent._best_action(0, h, s)) == int(got[i])
        assert agent._q_out[0].cpu().numpy().tobytes() == rows[i].tobytes()


def test_unserved_entries_refuse_before_anything_is_enqueued():
    import torch

    from slimdqn import _hip

    obs, feats, A, K, B, p, pt, batch = S.case("odd_even")
    agent = _agent("odd_even")
    agent._ensure_handle(32)
    lib, h, q = _hip.lib(), agent._handle, _hip.current_stream()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    pin = torch.zeros(1 << 14, dtype=torch.uint8).pin_memory()
    ipin = torch.zeros(64, dtype=torch.int32).pin_memory()
    d, hp, ip = _hip.ptr(buf), C.c_void_p(pin.data_ptr()), C.c_void_p(ipin.data_ptr())
    torch.cuda.synchronize()
    state = {s: getattr(agent, s).cpu().numpy().tobytes() for s in ("_online", "_target", "_mu", "_nu", "_grad", "_count")}
    arr = (C.c_void_p * 1)(h.value)
    g = C.c_void_p()
    per = _hip.PerStep()
    per.weights_dev = per.td_abs_dev = buf.data_ptr()
    pers = _hip.PerSteps()
    for f in ("nodes_dev", "max_priority_dev", "leaves_dev", "weights_dev", "td_abs_dev", "priorities_dev", "tree_scratch_dev"):
        setattr(pers, f, buf.data_ptr())
    pers.uniforms_host, pers.depth, pers.n_items = pin.data_ptr(), 4, 8
    fac, n1, n2 = C.c_void_p(), C.c_int64(), C.c_int64()
    calls = {
        "idqn_learn_on_replay": lambda: lib.idqn_learn_on_replay(h, d, 64, 120, d, ip, 5, 2, 5, 0, q),
        "idqn_learn_on_replay_dev": lambda: lib.idqn_learn_on_replay_dev(h, d, 64, 120, d, d, 5, 2, 5, 0, q),
        "idqn_learn_steps_on_replay_fc": lambda: lib.idqn_learn_steps_on_replay_fc(h, d, 64, 70, d, ip, 2, 5, 2, 5, 0, q),
        "idqn_learn_steps_on_replay_fc_dev": lambda: lib.idqn_learn_steps_on_replay_fc_dev(h, d, 64, 70, d, d, 2, 5, 2, 5, 0, q),
        "idqn_per_learn_steps_on_replay": lambda: lib.idqn_per_learn_steps_on_replay(h, C.byref(pers), d, 64, 70, d, 2, 5, 2, 5, 0, q),
        "idqn_iqn_learn_on_replay": lambda: lib.idqn_iqn_learn_on_replay(h, d, 64, 120, d, ip, d, 5, 2, 0, q),
        "idqn_iqn_learn_on_replay_dev": lambda: lib.idqn_iqn_learn_on_replay_dev(h, d, 64, 120, d, d, d, 5, 2, 0, q),
        "idqn_iqn_act_host_begin": lambda: lib.idqn_iqn_act_host_begin(h, 0, 0, hp, hp, d, ip, q),
        "idqn_export_dense0_factors": lambda: lib.idqn_export_dense0_factors(h, d, d, q),
        "idqn_dense0_factors": lambda: lib.idqn_dense0_factors(h, C.byref(fac), C.byref(n1), C.byref(n2)),
        "idqn_finish_step_factored": lambda: lib.idqn_finish_step_factored(h, d, d, 1, 1, 0, 0, 0, 0, 0, 0, 3, q),
        "idqn_per_learn_on_replay": lambda: lib.idqn_per_learn_on_replay(h, C.byref(per), d, 64, 70, d, 5, 2, 5, 0, q),
        "idqn_iqn_learn_on_batch": lambda: lib.idqn_iqn_learn_on_batch(h, d, d, d, d, d, d, 5, 0, q),
        "idqn_iqn_q_values": lambda: lib.idqn_iqn_q_values(h, 0, 0, d, 1, d, d, None, q),
        "idqn_backward_rest": lambda: lib.idqn_backward_rest(h, q),
        "idqn_act_host_many": lambda: lib.idqn_act_host_many(h, 0, ip, hp, 2, d, ip, q),
        "idqn_act_host_many_fc": lambda: lib.idqn_act_host_many_fc(h, 0, ip, hp, 2, d, ip, q),
        "idqn_iqn_act_host": lambda: lib.idqn_iqn_act_host(h, 0, 0, hp, hp, d, ip, q),
        "idqn_iqn_act_host_many": lambda: lib.idqn_iqn_act_host_many(h, 0, ip, hp, hp, 2, d, ip, q),
        "idqn_group_create": lambda: lib.idqn_group_create(arr, 1, C.byref(g)),
        "idqn_act_group_create": lambda: lib.idqn_act_group_create(arr, 1, C.byref(g)),
    }
    for name, call in calls.items():
        rc = call()
        text = _hip.lib().idqn_last_error().decode(errors="replace")
        assert rc == _hip.E_INVALID, (name, rc)
        assert "impala" in text, (name, text)
    assert g.value is None
    assert torch.cuda.current_stream().query(), "a refused entry left work on the stream"
    for s, want in state.items():
        assert getattr(agent, s).cpu().numpy().tobytes() == want, s
    # the i-IQN agent and the seed / acting groups refuse or fall back cleanly on the Python side
    from slimdqn.networks.group import AgentGroup
    from slimdqn.networks.iiqn import iIQN

    with pytest.raises(AssertionError):
        iIQN(3, obs, A, K, feats, "impala", 1e-3, 0.99, 1, 1, 10**9, 10**9, n_quantiles=4)
    group = AgentGroup([agent, _agent("odd_even")])
    assert not group._stock() and not group._stock_act_cnn()


def test_reference_smoke_flags_run_as_a_script_with_impala(tmp_path):
    """tests/test_atari.py:15-59 of the reference, flag for flag, with ``-at impala``."""
    root = os.path.join(ROOT, "i-dqn_amd")
    argv = ["-en", "_test_dqn_Pong", "-s", "1", "-dw", "-f", "2", "3", "1", "15", "-rbc", "100", "-bs", "3", "-n", "1", "-gamma", "0.99",
            "-lr", "1e-4", "-horizon", "10", "-ne", "1", "-ntspe", "10", "-utd", "3", "-tuf", "3", "-nis", "3", "-ee", "0.01", "-ed", "4",
            "-at", "impala"]
    code = ("import sys; sys.path.insert(0, %r); from experiments.atari.dqn import run; run(%r, save_root=%r)" % (root, argv, str(tmp_path)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
