"""The general-shape cnn path on the device (csrc/gcnn_kernels.h, k_fc_step / k_fc_q behind it, k_gconv_fwd_many + k_fc_act_many)
against the fp64 oracle, row by row of tests/gcnn_shapes.py: every Conv_0 pad class on each axis with an even and an odd Conv_1
input, frames of one row, one column and one pixel, a frame smaller than the 8x8 kernel, channel counts 1..5, conv widths 1, 7, 33,
65, no / one / two hidden dense layers, A = 1, 33, 40, B = 1, 33, 34, K = 1 and 3, flatten and hidden widths of 512 and 513.

Per row: (1) a gradients-only step -- per-head loss and every leaf gradient; (2) the post-ReLU output of every conv of all 2K nets
and the gradient at every conv's pre-activation, read through ``idqn_debug_buffer`` (``g_act0..2``, ``g_dact0..2``; ``g_dact2`` is
k_fc_step's ``din`` with its ReLU mask); (3) one Adam step from a zero state, EVERY element, then a second step against the
oracle re-based on the device's own parameters and moments; (4) Q-values of both parameter sets at n = 1 and n = min(B, 32);
(5) ``idqn_act_host`` against the fp64 argmax, and ``idqn_act_host_many_fc`` at n = 1, 3, 32 byte-equal to it; (6) a weighted
(prioritized) step with |TD| out on three rows; (7) the replay-sourced step on two rows, bytes equal to gather-then-learn.

Bars (the project's existing ones): loss 1e-5 max(1, |loss|); a leaf gradient 2e-5 of the leaf's largest fp64 magnitude; a stage
2e-5 of the stage's largest entry (STAGE_BAR of tests/test_gpu_conv_geometry.py); Q-values 1e-5 max(1, max |q|); parameters after
an Adam step 2e-5 absolute at lr 1e-3 (ADAM_ATOL there); actions where the oracle's top-two gap exceeds 1e-4 max(1, max |q|)
(GAP_RTOL there).  A leaf that misses 2e-5 is held to 4 x the error of the float32 torch_ref run on the same inputs
(gcnn_shapes.f32_errors), computed, not chosen, and is printed.  Measured on MI355X, one run: no row or leaf used the fallback;
the worst leaf is Conv_0/bias of row h13_w7 at 6.1e-6 (float32 oracle 8.6e-6), every other leaf is within 1.1e-6, stages within
8.2e-7, Adam within 3.2e-6, Q-values within 2.1e-7.

The activation buffers are allocated for the handle's ``max_batch`` samples per net, and a step of B samples packs its nets at
the front as [2K][B][OH][OW][CO] (online heads on ``state`` first, then the target heads on ``next_state``) and [K][B][...]:
every handle here is created for more samples than B, the stages are read at stride B, and the rest of each buffer has to be
still zero.

The acting dispatch ``dmax <= FC_MAX_WIDTH`` (k_fc_q1 | k_fc_q, k_fc_act_many1 | k_fc_act_many) is an MLP handle's: a general-shape
handle always runs k_fc_q and k_fc_act_many, whatever its widths (q_values_impl, fc_act_many_chain).  The rows with F or a hidden
width of 512 and 513 therefore straddle that path's workspace sizes (fc_ws, g_infws, the acting block's 2 * dmax floats per
state), not a kernel switch; tests/test_gpu_fc_act_many.py holds the switch itself on MLP handles (fc_limit, fc_wide).

Known hole: ``ggrid()`` caps a launch at 65536 workgroups and the kernels then loop with a grid stride.  The second trip of that
loop needs more than 1.6e7 outputs in one launch; no row here comes near it (the largest launch has under 4e4), and none is added.
"""
from collections import namedtuple

import numpy as np
import pytest

import gcnn_shapes as S

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
NAMES = list(S.ROWS)
LOSS_RTOL = 1e-5   # per-head loss, relative to max(1, |loss|) (tests/test_gpu_general_shapes.py)
GRAD_BAR = 2e-5    # every leaf gradient, relative to the leaf's largest fp64 magnitude (same file)
STAGE_BAR = 2e-5   # every stage, relative to the stage's largest entry (tests/test_gpu_conv_geometry.py)
ADAM_ATOL = 2e-5   # parameters after one Adam step at lr 1e-3, every element (same file)
Q_RTOL = 1e-5      # Q-values, relative to max(1, max |q|)
GAP_RTOL = 1e-4    # actions are compared where the oracle's top-two gap exceeds this (same scale)


def _fresh(name):
    """A new agent with the row's parameters and a handle created for more samples than the row's batch."""
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = iDQN(0, obs, A, K, feats, "cnn", S.LR, S.GAMMA_N, 1, 1, 10**9, 10**9, adam_eps=S.EPS)
    assert agent._gamma_n == S.GAMMA_N
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    agent._ensure_handle(B + 7)
    assert agent._handle_batch > B
    return agent


_SHARED = {}


def _shared(name):
    """The row's agent for the checks that leave parameters and optimizer state alone."""
    if name not in _SHARED:
        _SHARED[name] = _fresh(name)
    return _SHARED[name]


@pytest.fixture(scope="module", autouse=True)
def _release_shared_handles():
    """The rows' handles live for this module only."""
    yield
    for agent in _SHARED.values():
        agent._destroy_handle()
    _SHARED.clear()


def _batch(name):
    return Batch(*[np.array(a) for a in S.case(name)[7]])


def _grad_bar(name, k, leaf):
    return max(GRAD_BAR, 4 * S.f32_errors(name)[k][1][leaf])


def _check_grads(name, k, G, grads, what):
    errs = {leaf: float(np.abs(G[leaf][k] - g).max() / np.abs(g).max()) for leaf, g in grads.items()}
    worst = max(errs, key=errs.get)
    print(f"gcnn {name} head {k} {what}: worst leaf {worst} {errs[worst]:.3e}")
    for leaf, err in errs.items():  # every figure first, then the bars
        if err > GRAD_BAR:
            print(f"gcnn {name} head {k} {what}: FALLBACK {leaf} error {err:.3e}, float32 oracle {S.f32_errors(name)[k][1][leaf]:.3e}, "
                  f"bar {_grad_bar(name, k, leaf):.3e}")
    for leaf, err in errs.items():
        assert err <= _grad_bar(name, k, leaf), (what, leaf, err)


def _stage(agent, nm, nets, B, shape):
    """Buffer ``nm`` of the step just run as [nets, B, OH, OW, CO]; what lies behind the nets * B samples in use is still zero."""
    buf = agent._debug(nm).cpu().numpy()
    per = int(np.prod(shape))
    assert buf.size == nets * agent._handle_batch * per, (nm, buf.size)
    assert not buf[nets * B * per:].any(), f"{nm}: written past the {nets} x {B} samples of the step"
    return buf[: nets * B * per].reshape((nets, B) + tuple(shape))


@pytest.mark.parametrize("name", NAMES)
def test_gradients_and_stages(name):
    from oracle import qnet_ref as Q
    from slimdqn import _hip

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    want = S.oracle(name)
    agent = _shared(name)
    assert [(n, tuple(s)) for n, _, s in agent._leaves] == [(n, tuple(s)) for n, s in Q.leaf_shapes("cnn", obs, A, feats)]
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    G = agent._flat_grad()
    acts = [_stage(agent, f"g_act{i}", 2 * K, B, want[0]["act"][i].shape[1:]) for i in range(3)]
    dacts = [_stage(agent, f"g_dact{i}", K, B, want[0]["dact"][i].shape[1:]) for i in range(3)]
    for k, w in enumerate(want):
        print(f"gcnn {name} head {k} loss {losses[k]:.9f} oracle {w['loss']:.9f} error {abs(losses[k] - w['loss']):.3e}")
        assert abs(losses[k] - w["loss"]) <= LOSS_RTOL * max(1.0, abs(w["loss"])), (k, losses[k], w["loss"])
        _check_grads(name, k, G, w["grads"], "gradients")
        stage_err = {}
        for i in range(3):
            for nm, got, ref in ((f"act{i}", acts[i][k], w["act"][i]), (f"act_next{i}", acts[i][K + k], w["act_next"][i]),
                                 (f"dact{i}", dacts[i][k], w["dact"][i])):
                assert got.shape == ref.shape and np.abs(ref).max() > 0
                stage_err[nm] = float(np.abs(got - ref).max() / np.abs(ref).max())
        worst = max(stage_err, key=stage_err.get)
        print(f"gcnn {name} head {k} stages: worst {worst} {stage_err[worst]:.3e}")
        for nm, err in stage_err.items():
            assert err <= STAGE_BAR, (nm, k, err)


@pytest.mark.parametrize("name", NAMES)
def test_adam_step_every_element_then_a_chained_step(name):
    """One full step from a zero optimizer state: every element of every leaf, and count == 1.  Then a second step against the
    oracle's gradients at the device's own parameters and moments after step 1 (tests/test_gpu_impala.py::test_three_chained_steps:
    a sign flip on a tiny gradient cannot compound), every element again."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = _fresh(name)
    b = _batch(name)
    agent._learn(b)
    got, want = agent._flat(agent._online), S.adam_from_zero(name)
    errs = {leaf: float(np.abs(got[leaf] - want[leaf]).max()) for leaf in want}
    print(f"gcnn {name} adam step 1: worst leaf {max(errs, key=errs.get)} {max(errs.values()):.3e}")
    moved = {leaf: float(np.abs(got[leaf] - p[leaf]).max()) for leaf in want}
    assert min(moved.values()) > 0.5 * S.LR, moved  # every leaf took a step
    for leaf, err in errs.items():
        assert err <= ADAM_ATOL, (leaf, err)
    assert (agent._count.cpu().numpy() == 1).all()
    before = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
    agent._learn(b)
    after = agent._flat(agent._online)
    errs = {}
    for k in range(K):
        _, grads, _ = Q.loss_and_grads(Q.head(before["_online"], k), Q.head(pt, k), batch, "cnn", S.GAMMA_N)
        for leaf, g in grads.items():
            th, _, _ = Q.adam_update(before["_online"][leaf][k].astype(np.float64), g, before["_mu"][leaf][k].astype(np.float64),
                                     before["_nu"][leaf][k].astype(np.float64), 1, S.LR, S.EPS)
            errs[(k, leaf)] = float(np.abs(after[leaf][k] - th).max())
    print(f"gcnn {name} adam step 2: worst {max(errs, key=errs.get)} {max(errs.values()):.3e}")
    for key, err in errs.items():
        assert err <= ADAM_ATOL, (key, err)
    assert (agent._count.cpu().numpy() == 2).all()
    agent._destroy_handle()


@pytest.mark.parametrize("name", NAMES)
def test_q_values_of_both_nets(name):
    obs, feats, A, K, B, p, pt, batch = S.case(name)
    want = S.oracle(name)
    agent = _shared(name)
    worst = 0.0
    for k, w in enumerate(want):
        for n in sorted({1, min(B, 32)}):
            for params, states, ref in ((agent.params, batch[0], w["q"]), (agent.target_params, batch[3], w["q_next"])):
                q = agent.q_values(params, np.array(states[:n]), k).cpu().numpy()
                assert q.shape == (n, A)
                err = float(np.abs(q - ref[:n]).max() / max(1.0, np.abs(ref).max()))
                worst = max(worst, err)
                assert err <= Q_RTOL, (k, n, err)
    print(f"gcnn {name} q-values: worst {worst:.3e}")


def _single(agent, cache, which, k, e, states):
    """(Q row bytes, action) of the single-state route ``idqn_act_host`` for state e on head k of set ``which``."""
    key = (which, k, e)
    if key not in cache:
        act = int(agent._best_action(which, k, np.asarray(states[e])))
        cache[key] = (agent._q_out[0].cpu().numpy().copy(), act)
    return cache[key]


@pytest.mark.parametrize("name", NAMES)
def test_acting_single_state_and_vectorised(name):
    obs, feats, A, K, B, p, pt, batch = S.case(name)
    states, want = S.act_states(name), S.act_oracle(name)
    agent = _shared(name)
    cache = {}
    # idqn_act_host against the oracle: every head, two states, both parameter sets (actions on the online set)
    compared = excused = 0
    worst = 0.0
    for which in (0, 1):
        for k in range(K):
            for e in (0, 1):
                row, act = _single(agent, cache, which, k, e, states)
                ref = want[which][k][e]
                scale = max(1.0, np.abs(ref).max())
                worst = max(worst, float(np.abs(row - ref).max() / scale))
                assert np.abs(row - ref).max() <= Q_RTOL * scale, (which, k, e)
                assert act == int(np.argmax(row))  # first maximum of its own row
                if which == 0 and S.top_two_gap(ref) > GAP_RTOL * scale:
                    compared += 1
                    assert act == int(np.argmax(ref)), (k, e, act, ref)
                elif which == 0:
                    excused += 1
    print(f"gcnn {name} act_host: worst q row {worst:.3e}; actions compared {compared}, excused by the gap rule {excused}")
    # idqn_act_host_many_fc: rows and actions are the single-state route's bytes (csrc/fc_act_many_kernels.h)
    for n, first, heads in ((1, 4, [K - 1]), (3, 5, [(K - 1 - e) % K for e in range(3)]), (32, 0, [e % K for e in range(32)])):
        for which in (0, 1):
            acts = np.asarray(agent._best_actions(which, heads, [np.asarray(states[first + e]) for e in range(n)]))
            assert agent.__dict__.get("_act_many_ok") is False and agent.__dict__.get("_act_many_fc_ok") is True, "this is the loop"
            q = agent._q_out[:n].cpu().numpy().copy()
            for e, k in enumerate(heads):
                row, act = _single(agent, cache, which, k, first + e, states)
                assert q[e].tobytes() == row.tobytes(), (n, which, e, q[e], row)
                assert int(acts[e]) == act, (n, which, e)
    if A > 1 or K > 1:  # the two parameter sets are told apart
        assert cache[(0, 0, 0)][0].tobytes() != cache[(1, 0, 0)][0].tobytes()


@pytest.mark.parametrize("name", S.WEIGHTED)
def test_weighted_step_and_td(name):
    import torch

    from slimdqn import _hip

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    agent = _shared(name)
    w_dev = torch.from_numpy(S.weights(name)).cuda()
    td_dev = torch.zeros(K * B, dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    try:
        losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    G, td = agent._flat_grad(), td_dev.cpu().numpy().reshape(K, B)
    for k, (loss, grads, td_want) in enumerate(S.weighted_oracle(name)):
        td_err = float(np.abs(td[k] - td_want).max() / max(1.0, td_want.max()))
        print(f"gcnn {name} head {k} weighted: loss error {abs(losses[k] - loss):.3e}, |td| error {td_err:.3e}")
        assert abs(losses[k] - loss) <= LOSS_RTOL * max(1.0, abs(loss))
        assert td_err <= Q_RTOL  # a difference of two Q-values: their bar
        _check_grads(name, k, G, grads, "weighted gradients")


@pytest.mark.parametrize("name", S.REPLAY)
def test_replay_sourced_step_is_gather_then_learn(name):
    """``idqn_learn_on_replay_fc`` on a small wrapped ring whose stack is the row's channel count: every byte of the agent's
    state equals gather-then-learn on a fresh handle (buffers, seed choice and comparison of tests/test_gpu_fc_learn_on_replay.py)."""
    import test_gpu_fc_learn_on_replay as R

    obs, feats, A, K, B = S.ROWS[name]
    R.CONFIGS.setdefault("gcnn_row_" + name, ("cnn", tuple(obs[:2]), np.uint8, obs[2], obs, feats, K, A, B, "iDQN"))
    fused = R._identity("gcnn_row_" + name, R._buffer)
    assert fused.__dict__.get("_replay_fused_ok") is False  # the plane entry was asked once and said: not its ring
