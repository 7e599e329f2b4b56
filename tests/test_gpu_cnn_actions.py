"""GPU: the head kernels of the matrix-core cnn path and the i-IQN heads at action counts A = 1 .. 32 (tests/cnn_action_shapes.py).

Every kernel behind the conv trunk branches on A; the other tables reach A = 3, 4, 5, 6, 18.  Each iDQN row here runs in both conv
modes on one agent and is held to the fp64 oracle (oracle/qnet_ref.py):

(a) every stage of an ``F_GRADS_ONLY`` step (tests/cnn_stages.py: loss, q, q_next, dL/dh, every leaf gradient, every head and block);
(b) one weighted step (``is_weight`` / ``td_abs`` set): loss, gradients, |TD| per head and sample;
(c) one Adam step from a zero state;
(d) ``q_values`` of both nets, ``idqn_act_host`` on every head, ``idqn_act_host_many`` with heads e % K, ``idqn_best_action`` on several
    device states (``k_q_out``'s action) and, at A = 17 and 32, ``idqn_act_group_host`` over two members -- also byte for byte
    against ``idqn_act_host``;
(f) +5 on the target net's ``Dense_1/bias[j]`` for j in {0, A - 2, A - 1}: a kernel that leaves action j out of the maximum misses the
    loss by about (5 gamma^n)^2;
(g) a zero ``Dense_1/kernel`` and biases with the maximum planted twice: every acting entry returns the lower index.

(e), the replay-sourced step, and the i-IQN rows have tests of their own below; the last two tests stand on the other side of the
limit (A = 33).  The bars are the project's own, imported through cnn_action_shapes; tests/test_cnn_action_shapes_host.py shows on the
CPU that the fp32 oracle alone uses at most half of each.  The observed maxima are printed per row (``-s``) and set no bar.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import cnn_action_shapes as T
import cnn_stages as S
from test_gpu_fp_path import conv_mode  # noqa: F401  (fixture: both conv arithmetic modes)

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def _agent(row, p, pt):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    feats = T.feats_of(row)
    if row.K == 1:
        agent = DQN(0, T.OBS, row.A, feats, "cnn", T.LR, T.GAMMA, T.N_STEP, 1, 10**9, adam_eps=T.EPS)
    else:
        agent = iDQN(0, T.OBS, row.A, row.K, feats, "cnn", T.LR, T.GAMMA, T.N_STEP, 1, 10**9, 10**9, adam_eps=T.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    assert agent._w0 != (0, 0) and len(agent._leaves) == 10, "not the matrix-core path's layout"
    return agent


def _single(agent, which, head, state):
    act = int(agent._best_action(which, head, np.asarray(state)))  # host state: the idqn_act_host route
    return agent._q_out[0].cpu().numpy().copy(), act


def _k_q_out_actions(agent, which, head, states):
    """``idqn_best_action`` on n > 1 device states: the batched forward, ``k_hidden`` and ``k_q_out`` with its action."""
    import torch

    from slimdqn import _hip

    s = torch.from_numpy(np.ascontiguousarray(states)).cuda()
    n = int(s.shape[0])
    acts = torch.full((32,), -1, dtype=torch.int32, device="cuda")
    agent._ensure_handle(32)
    _hip.check(_hip.lib().idqn_best_action(agent._handle, which, head, _hip.ptr(s), n, _hip.ptr(agent._q_out), _hip.ptr(acts),
                                           _hip.current_stream()), "idqn_best_action")
    return agent._q_out[:n].cpu().numpy().copy(), acts[:n].cpu().numpy()


def _grad_errors(agent, want, K, failures, what, fig):
    G = agent._flat_grad()
    for k in range(K):
        for leaf, g in want[k][1].items():
            e = S.relerr(G[leaf][k], g)
            fig[what + " grad"] = max(fig.get(what + " grad", 0.0), e)
            if not e < T.STAGE_BAR:
                failures.append((what + " grad", k, leaf, e))


@pytest.mark.parametrize("rid", [r.id for r in T.IDQN])
def test_idqn_row_against_oracle(rid, conv_mode):  # noqa: F811
    import torch

    from slimdqn import _hip

    row = T.BY_ID[rid]
    A, K, B = row.A, row.K, row.B
    feats = T.feats_of(row)
    p, pt, batch, w = T.idqn_inputs(rid)
    ref = T.idqn_oracle(rid)
    heads = ref["plain"]
    agent = _agent(row, p, pt)
    lib = _hip.lib()
    failures, fig = [], {}

    # (a) every stage
    losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy().reshape(-1)
    torch.cuda.synchronize()
    for k in range(K):
        fig["loss"] = max(fig.get("loss", 0.0), abs(float(losses[k]) - heads[k][0]))
        if not abs(losses[k] - heads[k][0]) <= T.LOSS_ATOL:
            failures.append(("loss", k, float(losses[k]), float(heads[k][0])))
    errs = S.stage_errors(agent, p, pt, batch, T.OBS, feats, A, K, B, T.GAMMA_N, conv_mode, oracle=heads)
    fig["stage"] = max(errs.values())
    failures += [("stage", n, e) for n, e in errs.items() if not e < T.STAGE_BAR]

    # (d) Q-values and acting (before the Adam step: the oracle's Q-values are those of p)
    n = min(B, 32)
    states = batch[0][:n]
    for k in range(K):
        aux = heads[k][2]
        for name, which, st, want in (("online", 0, states, aux["q"][:n]), ("target", 1, batch[3][:n], aux["q_next"][:n])):
            q = agent._q_values(which, k, st).cpu().numpy()
            e = float(np.abs(q - want).max() / max(1.0, np.abs(want).max()))
            fig["q_values"] = max(fig.get("q_values", 0.0), e)
            if not e <= T.Q_RTOL:
                failures.append(("q_values " + name, k, e))
        picks = sorted({0, min(1, n - 1), n - 1})
        got = [_single(agent, 0, k, states[e]) for e in picks]
        e, _ = T.check_actions([a for _, a in got], np.stack([r for r, _ in got]), aux["q"][picks], failures, f"act_host head {k}")
        fig["act_host q"] = max(fig.get("act_host q", 0.0), e)
        rows, acts = _k_q_out_actions(agent, 0, k, states[:5])
        e, _ = T.check_actions(acts, rows, aux["q"][: len(rows)], failures, f"k_q_out head {k}")
        fig["k_q_out q"] = max(fig.get("k_q_out q", 0.0), e)
    hd = [e % K for e in range(n)]
    acts = np.asarray(agent._best_actions(0, hd, [np.asarray(s) for s in states]))  # the idqn_act_host_many route
    assert agent.__dict__.get("_act_many_ok") is True, "idqn_act_host_many refused the handle: this was the loop"
    want = np.stack([heads[hd[e]][2]["q"][e] for e in range(n)])
    fig["act_many q"], compared = T.check_actions(acts, agent._q_out[:n].cpu().numpy(), want, failures, "act_host_many")
    assert compared >= T.MIN_ACTION_SHARE * n, f"only {compared} of {n} states have a top-two gap that allows comparing actions"
    if rid in T.GROUP_ROWS:
        _group_part(row, agent, p, pt, states, heads, failures)

    # (c) one Adam step from the zero state, on the gradients of (a)
    agent._apply_adam()
    got = agent._flat(agent._online)
    for leaf, wantp in ref["adam"].items():
        e = float(np.abs(got[leaf] - wantp).max())
        fig["adam"] = max(fig.get("adam", 0.0), e)
        if not e <= T.ADAM_ATOL:
            failures.append(("adam", leaf, e))
    assert (agent._count.cpu().numpy() == 1).all()

    # (b) the weighted step, from the row's parameters again
    agent._load_flat(agent._online, p)
    w_dev, td_dev = torch.from_numpy(w).cuda(), torch.zeros((K, B), dtype=torch.float32, device="cuda")
    _hip.check(lib.idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy().reshape(-1)
    td = td_dev.cpu().numpy()
    for k in range(K):
        fig["weighted loss"] = max(fig.get("weighted loss", 0.0), abs(float(losses[k]) - ref["weighted"][k][0]))
        if not abs(losses[k] - ref["weighted"][k][0]) <= T.LOSS_ATOL:
            failures.append(("weighted loss", k, float(losses[k]), float(ref["weighted"][k][0])))
        want_td = np.abs(ref["weighted"][k][2]["td"])
        fig["td"] = max(fig.get("td", 0.0), float(np.abs(td[k] - want_td).max()))
        if not (np.abs(td[k] - want_td) <= T.TD_ATOL + T.TD_RTOL * want_td).all():
            failures.append(("|TD|", k, float(np.abs(td[k] - want_td).max())))
    _grad_errors(agent, ref["weighted"], K, failures, "weighted", fig)

    # (f) the target maximum at action j: plain mean again, |TD| still written
    _hip.check(lib.idqn_set_per_buffers(agent._handle, None, _hip.ptr(td_dev)), "idqn_set_per_buffers")
    for j, want in ref["bumped"].items():
        agent._load_flat(agent._target, T.bumped_target(pt, j))
        td_dev.zero_()
        losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy().reshape(-1)
        td = td_dev.cpu().numpy()
        for k in range(K):
            wl, wtd = want[k]
            # (a loss of ~20: LOSS_ATOL relative to max(1, |loss|), as tests/test_gpu_general_shapes.py has it; one fp32 ulp is 1.9e-6 there)
            e = abs(float(losses[k]) - wl) / max(1.0, wl)
            fig["bump loss"] = max(fig.get("bump loss", 0.0), e)
            if not e <= T.LOSS_ATOL:
                failures.append(("target maximum at action", j, "loss", k, float(losses[k]), float(wl)))
            if not (np.abs(td[k] - wtd) <= T.TD_ATOL + T.TD_RTOL * wtd).all():
                failures.append(("target maximum at action", j, "|TD|", k, float(np.abs(td[k] - wtd).max())))
    _hip.check(lib.idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    agent._load_flat(agent._target, pt)

    # (g) the first maximum wins: q is the bias bit for bit
    flat = {name: v.copy() for name, v in p.items()}
    flat["Dense_1/kernel"][:] = 0.0
    group = _Group()([agent])
    for bias, want in T.tie_biases(A):
        flat["Dense_1/bias"][:] = bias
        agent._load_flat(agent._online, flat)
        for k in range(K):
            row_q, act = _single(agent, 0, k, states[0])
            rows, acts = _k_q_out_actions(agent, 0, k, states[:3])
            if not ((row_q == bias).all() and (rows == bias[None]).all()):
                failures.append(("ties: q is not the bias", want, k))
            if act != want or acts.tolist() != [want] * 3:
                failures.append(("ties: act_host / k_q_out", want, k, act, acts.tolist()))
        m = min(n, 5)
        acts = np.asarray(agent._best_actions(0, hd[:m], [np.asarray(s) for s in states[:m]]))
        _, gacts = group.call(0, [0] * m, hd[:m], [states[e] for e in range(m)])
        if acts.tolist() != [want] * m or gacts.tolist() != [want] * m:
            failures.append(("ties: act_host_many / act_group", want, acts.tolist(), gacts.tolist()))
    group.close()
    print(rid, conv_mode, {k: f"{v:.3g}" for k, v in fig.items()})
    agent._destroy_handle()
    assert not failures, failures


def _Group():
    from test_gpu_act_group import _Group as G

    return G


def _group_part(row, agent, p, pt, states, heads, failures):
    """``idqn_act_group_host`` over two members (member 1 holds the two parameter sets exchanged), as tests/test_gpu_act_group.py: every
    row against the oracle and, byte for byte, against the member's own ``idqn_act_host``."""
    from oracle import qnet_ref as Q

    K = row.K
    other = _agent(row, pt, p)
    agent._ensure_handle(32), other._ensure_handle(32)
    members = [agent, other]
    group = _Group()(members)
    n = 8
    mem, hd = [e % 2 for e in range(n)], [(e // 2) % K for e in range(n)]
    for which in (0, 1):
        q, acts = group.call(which, mem, hd, [states[e] for e in range(n)])
        want = np.stack([Q.forward(Q.head((p, pt)[(which + g) % 2], k), states[e : e + 1], "cnn")[0] for e, (g, k) in enumerate(zip(mem, hd))])
        T.check_actions(acts, q, want, failures, f"act_group which {which}")
        for e, (g, k) in enumerate(zip(mem, hd)):
            q1, a1 = _single(members[g], which, k, states[e])
            if q[e].tobytes() != q1.tobytes() or int(acts[e]) != a1:
                failures.append(("act_group differs from act_host", which, e, q[e].tolist(), q1.tolist(), int(acts[e]), a1))
    group.close()
    other._destroy_handle()


# ---- (e) the replay-sourced step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", T.REPLAY_ROWS)
def test_learn_on_replay_is_sample_then_learn(rid, monkeypatch):
    """``idqn_learn_on_replay`` on the frame ring equals ``rb.sample()`` then ``learn_on_batch`` bit for bit at A = 32 and A = 9."""
    import torch

    from test_gpu_conv_geometry import _assert_same_bits, _replay_pair

    monkeypatch.delenv("IDQN_CONV", raising=False)
    row = T.BY_ID[rid]
    (rb_a, agent_a), (rb_b, agent_b) = _replay_pair(T.OBS, T.feats_of(row), row.A, row.K, row.B)
    agent_b.fuse_replay_sampling = False
    for step in range(3):
        agent_a.update_online_params(step, rb_a)
        agent_b.update_online_params(step, rb_b)
    torch.cuda.synchronize()
    assert agent_a.__dict__.get("_replay_fused_ok") is True, "the fused path did not run"
    _assert_same_bits(agent_a, agent_b, rb_a, rb_b)


# ---- the i-IQN heads ----------------------------------------------------------------------------------------------------------------
def _iqn_agent(row, p, pt):
    from slimdqn.networks.iiqn import iIQN

    hy = T.iqn_hyper()
    agent = iIQN(0, T.OBS, row.A, row.K, T.feats_of(row), "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"],
                 n_quantiles=row.N)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


@pytest.mark.parametrize("rid", [r.id for r in T.IQN])
def test_iqn_row_against_oracle(rid, monkeypatch):
    """Acting first (the step moves the parameters): ``idqn_iqn_q_values``, ``idqn_iqn_act_host`` on every head and
    ``idqn_iqn_act_host_many`` on min(B, 32) states against ``iqn_ref.greedy_action`` with the same fractions; the planted ties; then ONE
    full step through ``iqn_record`` + ``check_iqn_step``."""
    monkeypatch.delenv("IDQN_CONV", raising=False)
    row = T.BY_ID[rid]
    A, K, B, N = row.A, row.K, row.B, row.N
    p, pt, batch, taus, act_taus = T.iqn_inputs(rid)
    want = T.iqn_acting_oracle(rid)
    agent = _iqn_agent(row, p, pt)
    n = min(B, 32)
    states = batch[0][:n]
    failures, fig = [], {}
    for which in (0, 1):
        params = agent.params if which == 0 else agent.target_params
        for k in range(K):
            q = agent.q_values(params, states, k, taus=np.ascontiguousarray(act_taus[:n].T)).cpu().numpy()
            e = float((np.abs(q - want[(which, k)]).max(axis=1) / np.maximum(1.0, np.abs(want[(which, k)]).max(axis=1))).max())
            fig["q_values"] = max(fig.get("q_values", 0.0), e)
            if not e <= T.Q_RTOL:
                failures.append(("idqn_iqn_q_values", which, k, e))
            picks = sorted({0, min(1, n - 1), n - 1})
            got = []
            for e_ in picks:
                act = int(agent._act_host(which, k, np.asarray(states[e_]), act_taus[e_][:, None], None))
                got.append((agent._q_out[0].cpu().numpy().copy(), act))
                if act != int(got[-1][0].argmax()):
                    failures.append(("idqn_iqn_act_host: action is not its own row's first maximum", which, k, e_))
            e, _ = T.check_actions([a for _, a in got], np.stack([r for r, _ in got]), want[(which, k)][picks], failures,
                                   f"idqn_iqn_act_host which {which} head {k}")
            fig["act_host q"] = max(fig.get("act_host q", 0.0), e)
        hd = [e % K for e in range(n)]
        acts = agent._act_host_many(which, hd, [np.asarray(s) for s in states], act_taus[:n])
        assert agent.__dict__.get("_iqn_act_many_ok") is True, "the batched entry was refused: this is the loop"
        w = np.stack([want[(which, hd[e])][e] for e in range(n)])
        e, compared = T.check_actions(acts, agent._q_out[:n].cpu().numpy(), w, failures, f"idqn_iqn_act_host_many which {which}")
        fig["act_many q"] = max(fig.get("act_many q", 0.0), e)
        assert compared >= T.MIN_ACTION_SHARE * n

    # (g) a zero Dense_1/kernel: every quantile value is the bias exactly, and so is their mean over N = 1, 8, 32 fractions
    flat = {name: v.copy() for name, v in p.items()}
    flat["Dense_1/kernel"][:] = 0.0
    m = min(n, 5)
    for bias, want_a in T.tie_biases(A):
        flat["Dense_1/bias"][:] = bias
        agent._load_flat(agent._online, flat)
        for k in range(K):
            act = int(agent._act_host(0, k, np.asarray(states[0]), act_taus[0][:, None], None))
            row_q = agent._q_out[0].cpu().numpy().copy()
            if act != want_a or not (row_q == bias).all():
                failures.append(("ties: idqn_iqn_act_host", want_a, k, act, row_q.tolist()))
            agent._iqn_q(0, k, states[:3], np.ascontiguousarray(act_taus[:3].T), want_action=True)
            acts3 = agent._action_out[:3].cpu().numpy().tolist()
            if acts3 != [want_a] * 3:
                failures.append(("ties: idqn_iqn_q_values", want_a, k, acts3))
        acts = agent._act_host_many(0, hd[:m], [np.asarray(s) for s in states[:m]], act_taus[:m])
        if np.asarray(acts).tolist() != [want_a] * m or not (agent._q_out[:m].cpu().numpy() == bias[None]).all():
            failures.append(("ties: idqn_iqn_act_host_many", want_a, np.asarray(acts).tolist()))
    agent._load_flat(agent._online, p)
    print(rid, {k: f"{v:.3g}" for k, v in fig.items()})
    assert not failures, failures

    # the step
    rec = T.iqn_record(rid)
    losses = agent._learn(Batch(*batch), taus=taus).cpu().numpy()
    S.check_iqn_step(agent, losses, rec, A, K, B, N)
    agent._destroy_handle()


# ---- the other side of the limit ----------------------------------------------------------------------------------------------------
def test_33_actions_on_the_nature_shape_is_the_general_path():
    """A = 33 with the Nature-CNN widths: ``cnn_fast_shape`` sends it to the general-shape kernels.  The create succeeds, the handle is
    a general-shape one (``idqn_act_host_many`` refuses it, ``idqn_act_host_many_fc`` serves it -- the ten leaf names are the same on
    both paths and tell nothing), and the step meets the oracle as every general shape does."""
    from oracle import qnet_ref as Q
    from slimdqn.networks.idqn import iDQN
    from test_gpu_general_shapes import _run_case

    obs, feats, A, K, B = (84, 84, 4), [32, 64, 64, 512], 33, 1, 8
    _run_case(obs, feats, A, K, B)
    agent = iDQN(0, obs, A, K, feats, "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-8)
    states = Q.synthetic_batch(3, 2, obs, A, "cnn")[0]
    acts = agent._best_actions(0, [0, 0], [np.asarray(s) for s in states])
    assert agent._act_many_ok is False and agent._act_many_fc_ok is True, "not a general-shape handle"
    rows = agent._q_out[:2].cpu().numpy()
    assert rows.shape == (2, 33) and acts.tolist() == rows.argmax(1).tolist()
    agent._destroy_handle()


def test_iqn_with_33_actions_is_refused_at_create():
    from slimdqn import _hip
    from slimdqn.networks.iiqn import iIQN

    with pytest.raises(_hip.HipExtensionError, match="n_actions <= 32"):
        iIQN(0, T.OBS, 33, 2, [32, 32, 32, 256], "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9, n_quantiles=8)
    # the library itself, past the Python layout call: idqn_create answers the same, and a legal create afterwards works
    row = T.BY_ID["iqn_A32"]
    p, pt = T.iqn_inputs("iqn_A32")[:2]
    agent = _iqn_agent(row, p, pt)
    agent._ensure_handle(32)
    cfg = agent._config(32)
    cfg.n_actions = 33
    h = C.c_void_p()
    rc = _hip.lib().idqn_create(C.byref(cfg), _hip.ptr(agent._online), _hip.ptr(agent._target), _hip.ptr(agent._mu), _hip.ptr(agent._nu),
                                _hip.ptr(agent._grad), _hip.ptr(agent._count), _hip.ptr(agent._losses), _hip.ptr(agent._cum), C.byref(h))
    assert rc != 0 and h.value is None and "n_actions <= 32" in _hip.lib().idqn_last_error().decode()
    agent._destroy_handle()
