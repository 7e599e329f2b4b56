"""GPU: the matrix-core conv path at frame geometries other than 84x84, 20x20 and 36x28.

``cnn_fast_shape()`` (csrc/qnet.hip) sends every cnn with 4 input channels, conv widths 32 / 64 and one hidden dense layer of
128..512 onto the hand-written path for ANY frame of at least 8x8.  The three frame sizes of the other GPU tests are all
multiples of 4 whose quotient is odd: Conv_0 always pads (2, 2), Conv_1 always sees an odd input and pads (1, 2), its data
gradient always has four parity variants of unequal size.  The table below covers the other classes -- H mod 4 = 1, 2, 3
(pads (3, 4), (3, 3), (2, 3)), even Conv_1 inputs, layers that collapse to 1x1, frames one or two output columns wide,
frames larger than Atari's, flatten widths from 32 to 11648 -- and holds every one of them to the fp64 oracle:

* stage by stage (tests/cnn_stages.py), every head and every 32-sample block, at the bars of test_gpu_fp_path.py;
* the zero borders of the padded activation and gradient buffers read directly;
* one Adam step, Q-values, single-state and vectorised acting;
* the replay-sourced step, the i-IQN heads and (tests/test_gpu_handle_history.py) a used handle;
* a sweep of 64 small frames, created, stepped once and destroyed: a planner check that refuses a geometry the dispatcher
  chose the path for shows up as a failed create.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import cnn_stages as S
from test_gpu_fp_path import conv_mode  # noqa: F401  (fixture: both conv arithmetic modes)

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
LOSS_ATOL = 1e-5   # per-head loss (test_gpu_fp_path.py)
STAGE_BAR = 2e-5   # every stage, relative to the stage's largest entry (test_gpu_fp_path.py)
ADAM_ATOL = 2e-5   # parameters after one Adam step (test_ragged_batches_and_shapes_against_oracle)
Q_RTOL = 1e-5      # Q-values, relative to max(1, max |q|) (test_gpu_general_shapes.py)
GAP_RTOL = 1e-4    # actions are compared where the oracle's top-two gap exceeds this (same scale)
GAMMA, N_STEP, LR, EPS = 0.97, 3, 1e-3, 1e-6
GAMMA_N = GAMMA ** N_STEP

TABLE = [
    # obs, features, A, K, B
    ((8, 8, 4), [32, 32, 32, 128], 3, 2, 5),        # smallest legal frame: Conv_1 / Conv_2 are 1x1, F = 32
    ((11, 10, 4), [32, 32, 64, 128], 3, 2, 7),      # H mod 4 = 3, W mod 4 = 2; 2x2 later layers, F = 256
    ((9, 13, 4), [32, 64, 32, 128], 4, 2, 33),      # pad (3, 4) on both axes; Conv_1 input 3x4; F = 128; one sample in block 2
    ((22, 31, 4), [64, 32, 64, 256], 6, 2, 40),     # pad (3, 3) x (2, 3); Conv_1 input 6x8, both even
    ((24, 24, 4), [32, 32, 64, 384], 4, 2, 64),     # multiple of 4 with even quotient; J = 384; two full blocks
    ((23, 40, 4), [64, 64, 64, 256], 5, 2, 33),     # pad (2, 3) rows, Conv_1 input 6x10
    ((45, 50, 4), [32, 64, 64, 512], 18, 2, 33),    # Conv_1 input 12x13 (even x odd), 18 actions
    ((84, 8, 4), [32, 64, 64, 128], 5, 1, 20),      # two output columns, then one: every range of positions spans many rows
    ((8, 84, 4), [64, 64, 32, 256], 5, 1, 20),      # the transpose: one output row
    ((100, 108, 4), [32, 64, 64, 512], 6, 1, 8),    # larger than Atari: 25x27 -> 13x14, F = 11648
]
IDS = ["%dx%d" % row[0][:2] for row in TABLE]
ROW = {row[0][:2]: row for row in TABLE}


def _inputs(obs, feats, A, K, B):
    """Parameters and one batch, built as test_ragged_batches_and_shapes_against_oracle builds them."""
    from oracle import qnet_ref as Q

    p = Q.init_params(3, "cnn", obs, A, feats, K)
    pt = Q.init_params(4, "cnn", obs, A, feats, K)
    rng = np.random.default_rng(5)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = list(Q.synthetic_batch(6, B, obs, A, "cnn"))
    batch[4][B // 2] = True
    return p, pt, tuple(batch)


@functools.lru_cache(maxsize=None)
def _reference(i):
    """Inputs and everything the oracle says about row i: computed once, shared by both conv modes, never modified."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B = TABLE[i]
    p, pt, batch = _inputs(obs, feats, A, K, B)
    heads = S.oracle_heads(p, pt, batch, K, GAMMA_N)
    adam = {}
    for n in p:  # Q.learn_on_batch's update from a zero optimizer state, from the gradients already computed
        adam[n] = np.stack([Q.adam_update(p[n][k].astype(np.float64), heads[k][1][n], 0.0, 0.0, 0, LR, EPS)[0] for k in range(K)])
    return p, pt, batch, heads, adam


def _agent(obs, feats, A, K, p, pt):
    from slimdqn.networks.idqn import iDQN

    agent = iDQN(0, obs, A, K, feats, "cnn", LR, GAMMA, N_STEP, 1, 10**9, 10**9, adam_eps=EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _gap(q):
    top = np.sort(q)[::-1]
    return top[0] - top[1]


@pytest.mark.parametrize("i", range(len(TABLE)), ids=IDS)
def test_geometry_row_against_oracle(i, conv_mode):  # noqa: F811
    """(a) every stage of every head and sample block, (b) zero borders, (d) Q-values and acting, (c) one Adam step."""
    import torch

    from oracle import qnet_ref as Q
    from slimdqn import _hip

    obs, feats, A, K, B = TABLE[i]
    p, pt, batch, heads, adam = _reference(i)
    if i == 0:  # Q.learn_on_batch itself, once: the shared reference above is its update
        zeros = {n: np.zeros(v.shape, np.float64) for n, v in p.items()}
        want, _, _, _, _ = Q.learn_on_batch({n: v.astype(np.float64) for n, v in p.items()}, pt, zeros, zeros,
                                            np.zeros(K, np.int64), batch, "cnn", GAMMA_N, LR, EPS)
        for n in want:
            np.testing.assert_array_equal(want[n], adam[n])
    agent = _agent(obs, feats, A, K, p, pt)
    assert agent._w0 != (0, 0) and len(agent._leaves) == 10, "not the matrix-core path's layout"
    failures = []

    # (a) stage helper
    losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    torch.cuda.synchronize()
    for k in range(K):
        print(f"head {k}: loss {losses[k]:.8f} oracle {heads[k][0]:.8f}")
        if not abs(losses[k] - heads[k][0]) <= LOSS_ATOL:
            failures.append(("loss", k, float(losses[k]), float(heads[k][0])))
    errs = S.stage_errors(agent, p, pt, batch, obs, feats, A, K, B, GAMMA_N, conv_mode, oracle=heads)
    S.print_stage_errors(errs)
    failures += [("stage", n, e) for n, e in errs.items() if not e < STAGE_BAR]

    # (b) borders stay zero, interiors are live
    for name, (outside, inside) in S.border_report(agent, obs, feats, K, B, conv_mode).items():
        print(f"border {name}: max |outside| {outside:.3e}, min over slots of max |interior| {inside:.3e}")
        if not outside == 0.0:
            failures.append(("border not zero", name, outside))
        if not inside > 0.0:
            failures.append(("interior all zero in some slot", name, inside))

    # (d) Q-values and acting (before the Adam step: the oracle's Q-values are those of p)
    n = min(B, 32)
    states = batch[0][:n]
    for k in range(K):
        aux = heads[k][2]
        q = agent.q_values(agent.params, states, k).cpu().numpy()
        if not np.abs(q - aux["q"][:n]).max() <= Q_RTOL * max(1.0, np.abs(aux["q"]).max()):
            failures.append(("q_values online", k, float(np.abs(q - aux["q"][:n]).max())))
        qt = agent.q_values(agent.target_params, batch[3][:2], k).cpu().numpy()
        if not np.abs(qt - aux["q_next"][:2]).max() <= Q_RTOL * max(1.0, np.abs(aux["q_next"]).max()):
            failures.append(("q_values target", k, float(np.abs(qt - aux["q_next"][:2]).max())))
        e = min(1, n - 1)
        want = aux["q"][e]
        act = int(agent._best_action(0, k, np.asarray(states[e])))  # host state: the idqn_act_host route
        row = agent._q_out[0].cpu().numpy()
        scale = max(1.0, np.abs(want).max())
        if not np.abs(row - want).max() <= Q_RTOL * scale:
            failures.append(("act_host q row", k, float(np.abs(row - want).max())))
        if _gap(want) > GAP_RTOL * scale and act != int(np.argmax(want)):
            failures.append(("act_host action", k, act, int(np.argmax(want))))
    hd = [e % K for e in range(n)]
    acts = np.asarray(agent._best_actions(0, hd, [np.asarray(s) for s in states]))  # the idqn_act_host_many route
    rows = agent._q_out[:n].cpu().numpy()
    compared = 0
    for e in range(n):
        want = heads[hd[e]][2]["q"][e]
        scale = max(1.0, np.abs(want).max())
        if _gap(want) > GAP_RTOL * scale:
            compared += 1
            if int(acts[e]) != int(np.argmax(want)):
                failures.append(("act_host_many action", e, int(acts[e]), int(np.argmax(want))))
        elif not np.abs(rows[e] - want).max() <= Q_RTOL * scale:
            failures.append(("act_host_many q row", e, float(np.abs(rows[e] - want).max())))
    assert 2 * compared >= n, f"only {compared} of {n} states have a top-two gap that allows comparing actions"

    # (c) Adam step
    agent._apply_adam()
    got = agent._flat(agent._online)
    for leaf in adam:
        err = float(np.abs(got[leaf] - adam[leaf]).max())
        if not err <= ADAM_ATOL:
            failures.append(("adam", leaf, err))
    assert (agent._count.cpu().numpy() == 1).all()
    agent._destroy_handle()
    assert not failures, failures


# ---- 3(a) the replay-sourced step -----------------------------------------------------------------------------------------
def _replay_pair(obs, feats, A, K, B):
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    def make():
        rb = ReplayBuffer(UniformSamplingDistribution(5), batch_size=B, max_capacity=96, stack_size=4, update_horizon=2, gamma=0.99)
        rng = np.random.default_rng(9)
        for t in range(230):  # more transitions than the ring holds: slots and frames have wrapped
            rb.add(TransitionElement(rng.integers(0, 256, obs[:2], dtype=np.uint8), int(rng.integers(A)), float(rng.normal()),
                                     bool(t % 37 == 36), bool(t % 91 == 90)))
        rb.reuse_sample_buffers = True
        return rb, iDQN(0, obs, A, K, feats, "cnn", 6.25e-5, 0.99, 2, 1, 10**9, 10**9, adam_eps=1.5e-4)

    return make(), make()


def _assert_same_bits(agent_a, agent_b, rb_a, rb_b):
    for name in ("_online", "_mu", "_nu", "_losses", "_cum"):
        np.testing.assert_array_equal(getattr(agent_a, name).cpu().numpy(), getattr(agent_b, name).cpu().numpy(), err_msg=name)
    assert np.isfinite(agent_a._losses.cpu().numpy()).all() and (agent_a._count.cpu().numpy() == 3).all()
    assert rb_a._sampling_distribution._rng_key.bit_generator.state == rb_b._sampling_distribution._rng_key.bit_generator.state


@pytest.mark.parametrize("hw", [(8, 8), (24, 24), (84, 8), (8, 84), (100, 108)], ids=lambda hw: "%dx%d" % hw)
def test_learn_on_replay_is_sample_then_learn(hw, monkeypatch):
    """Frames whose byte count is a multiple of 16: `update_online_params` as one call on the frame ring equals
    `rb.sample()` then `learn_on_batch` bit for bit (as tests/test_gpu_int_path.py has it at 84x84)."""
    import torch

    monkeypatch.delenv("IDQN_CONV", raising=False)
    obs, feats, A, K, B = ROW[hw]
    assert obs[0] * obs[1] % 16 == 0
    (rb_a, agent_a), (rb_b, agent_b) = _replay_pair(obs, feats, A, K, B)
    agent_b.fuse_replay_sampling = False
    for step in range(3):
        agent_a.update_online_params(step, rb_a)
        agent_b.update_online_params(step, rb_b)
    torch.cuda.synchronize()
    assert agent_a.__dict__.get("_replay_fused_ok") is True, "the fused path did not run"
    _assert_same_bits(agent_a, agent_b, rb_a, rb_b)


def test_frame_of_682_bytes_gathers_then_learns(monkeypatch):
    """(22, 31): 682 bytes per frame, no multiple of 16 -- the ring is not fusable, the step still runs and equals
    gather-then-learn bit for bit."""
    import torch

    monkeypatch.delenv("IDQN_CONV", raising=False)
    obs, feats, A, K, B = ROW[(22, 31)]
    (rb_a, agent_a), (rb_b, agent_b) = _replay_pair(obs, feats, A, K, B)
    agent_b.fuse_replay_sampling = False
    for step in range(3):
        agent_a.update_online_params(step, rb_a)
        agent_b.update_online_params(step, rb_b)
    torch.cuda.synchronize()
    assert rb_a.ring_view()[2] == 682 and not agent_a._ring_fusable(rb_a.ring_view())
    assert agent_a.__dict__.get("_replay_fused_ok") is False
    _assert_same_bits(agent_a, agent_b, rb_a, rb_b)


# ---- 3(b) the i-IQN heads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(22, 31), (45, 50)], ids=lambda hw: "%dx%d" % hw)
def test_iqn_step_and_acting_against_oracle(hw, monkeypatch):
    """One i-IQN step (n_quantiles = 8, K = 2, B = 33), a batched Q-value call and one idqn_iqn_act_host call against
    oracle/iqn_ref.py, compared as tests/test_gpu_iqn.py compares its small case (S.check_iqn_step: the same bars)."""
    from oracle import iqn_ref as I
    from oracle import make_golden as G
    from oracle import qnet_ref as Q
    from slimdqn.networks.iiqn import iIQN

    monkeypatch.delenv("IDQN_CONV", raising=False)
    obs, feats, A = ROW[hw][:3]
    K, B, N = 2, 33, 8
    hy = G.FP_HYPER
    p = I.init_params(3, obs, A, feats, K)
    pt = I.init_params(4, obs, A, feats, K)
    rng = np.random.default_rng(5)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(6, B, obs, A, "cnn")
    term[B // 2] = True
    batch = (st, a, r, s2, term)
    taus = I.synthetic_taus(7, K, N, B)
    agent = iIQN(0, obs, A, K, feats, "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"], n_quantiles=N)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    # acting first (the step moves the parameters): a batch of states, then one host state through the graph + mailbox route
    tau = rng.random((N, 7)).astype(np.float32)
    q = agent.q_values(agent.params, st[:7], 1, taus=tau).cpu().numpy()
    for e in range(7):
        _, want = I.greedy_action(Q.head(p, 1), st[e], tau[:, e])
        assert np.abs(q[e] - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (e, q[e], want)
    tau1 = rng.random((N, 1)).astype(np.float32)
    act = int(agent._act_host(1, 0, np.asarray(s2[3]), tau1, None))
    want_act, want = I.greedy_action(Q.head(pt, 0), s2[3], tau1[:, 0])
    row = agent._q_out[0].cpu().numpy()
    assert np.abs(row - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (row, want)
    assert act == int(row.argmax())
    if _gap(want) > GAP_RTOL * max(1.0, np.abs(want).max()):
        assert act == want_act
    # the step
    rec = S.iqn_record(p, pt, batch, taus, hy)
    losses = agent._learn(Batch(*batch), taus=taus).cpu().numpy()
    S.check_iqn_step(agent, losses, rec, A, K, B, N)


# ---- 4. creation-and-one-step sweep -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", range(8, 24))
def test_create_and_step_sweep(H, monkeypatch):
    """Every height 8..23 with four widths: create (a planner check that refuses the geometry fails here, with the library's
    message), one F_GRADS_ONLY step of 40 samples on a handle for 64, the loss (the forward pass) and the gradients of the
    first and the largest leaf (the whole backward) against the oracle, destroy."""
    from slimdqn import _hip

    monkeypatch.delenv("IDQN_CONV", raising=False)
    feats, A, K, B = [32, 64, 64, 128], 4, 2, 40
    failures = []
    for W in (8 + (5 * H) % 16, 12, 17, 30):
        obs = (H, W, 4)
        p, pt, batch = _inputs(obs, feats, A, K, B)
        agent = _agent(obs, feats, A, K, p, pt)
        try:
            agent._ensure_handle(64)
        except Exception as e:  # the message of the C side
            print(f"({H}, {W}): create failed: {e}")
            failures.append((H, W, "create", str(e)))
            continue
        try:
            losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy()
            G = agent._flat_grad()
            heads = S.oracle_heads(p, pt, batch, K, GAMMA_N)
            for k in range(K):
                e0 = S.relerr(G["Conv_0/kernel"][k], heads[k][1]["Conv_0/kernel"])
                ed = S.relerr(G["Dense_0/kernel"][k], heads[k][1]["Dense_0/kernel"])
                print(f"({H}, {W}) head {k}: loss {losses[k]:.8f} oracle {heads[k][0]:.8f}  Conv_0/kernel {e0:.3e}  Dense_0/kernel {ed:.3e}")
                if not abs(losses[k] - heads[k][0]) <= LOSS_ATOL:
                    failures.append((H, W, "loss", k, float(losses[k]), float(heads[k][0])))
                if not e0 < STAGE_BAR:
                    failures.append((H, W, "Conv_0/kernel", k, e0))
                if not ed < STAGE_BAR:
                    failures.append((H, W, "Dense_0/kernel", k, ed))
        finally:
            agent._destroy_handle()
    assert not failures, failures
