"""GPU: the i-IQN learner step's heads on every route of the Dense_0 layer, at every group size of the fraction count, against the fp64
oracle (tests/iqn_shapes.py holds the table, the restated planner and the oracle records; oracle/iqn_ref.py is the reference).

Per row, on a fresh ``iIQN`` agent loaded with the row's parameters:

1. the ROUTE: the step runs with ``IDQN_F_PROFILE_ALL`` and the Dense_0 launch names of ``idqn_profile_table`` must equal
   ``expected_route(row)`` (the fused launch, the two-split pair and the plain step's update have names of their own; the stream and
   gemm-dgrad routes share theirs, see tests/iqn_shapes.py);
2. that same step, the first from a zero Adam state, through ``cnn_stages.check_iqn_step`` with its bars unchanged;
3. on the chained rows two more steps, each with another batch and other fractions: per-step losses, and parameters, ``mu`` and ``nu`` of
   every leaf after the third step against three oracle steps;
4. where the fused launch ran: every word of the handle's ``iqn_gate`` allocation (arrived, passed, err) is zero after every step;
5. ``IDQN_IQN_ADAM_FUSE=0`` on four fused rows: the route becomes the two-split pair (asserted) and the step meets the same bars.  The
   library reads the switch when a handle is created, and every agent here creates its own;
6. a weighted step (``idqn_set_per_buffers``) on one row per route, the route asserted again, against the checker of
   tests/test_gpu_iqn_per.py;
7. acting at N = 33, 61, 64 (NP = 64 with zero rows behind N): ``idqn_iqn_q_values``, ``idqn_iqn_act_host`` and
   ``idqn_iqn_act_host_many`` against ``iqn_ref.greedy_action``.

Observed figures are printed (``-s``); none sets a bar.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import cnn_stages as S
import iqn_shapes as T

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def _agent(row):
    from slimdqn.networks.iiqn import iIQN

    hy = T.hyper()
    agent = iIQN(0, row.obs, row.A, row.K, row.feats, "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"],
                 n_quantiles=row.N)
    p, pt = T.params(row.id)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _profiled_step(agent, batch, taus):
    """One step with the timeline on: (losses, the names of its launches in launch order)."""
    from slimdqn import _hip

    losses = agent._learn(Batch(*batch), flags=_hip.F_PROFILE_ALL, taus=taus).cpu().numpy().copy()
    buf = C.create_string_buffer(8192)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, 8192), "idqn_profile_table")
    return losses, [ln.split("\t")[0] for ln in buf.value.decode().splitlines()]


def _gate_words(agent):
    import torch

    return agent._debug("iqn_gate").view(torch.int32).cpu().numpy()


def _run_row(rid, fuse_switch):
    row = T.BY_ID[rid]
    want_route = T.expected_route(row, fuse_switch)
    fused = want_route == ["iqn dense0 dgrad + wgrad + adam"]
    o64 = T.oracle(rid)
    rec = T.record(rid)
    agent = _agent(row)
    batch, taus = T.step_inputs(rid, 0)
    losses, names = _profiled_step(agent, batch, taus)
    got_route = T.dense0_launches(names)
    print(rid, "route", T.route(row, fuse_switch), got_route)
    assert got_route == want_route, (rid, got_route, want_route)
    assert (_gate_words(agent) == 0).all(), "the gate words are not as the launch found them (step 0)"
    S.check_iqn_step(agent, losses, rec, row.A, row.K, row.B, row.N)
    if T.chained(row) and fuse_switch:
        all_losses = [losses]
        for t in range(1, T.N_STEPS_CHAIN):
            batch, taus = T.step_inputs(rid, t)
            all_losses.append(agent._learn(Batch(*batch), taus=taus).cpu().numpy().copy())
            if fused:
                assert (_gate_words(agent) == 0).all(), f"the gate words are not as the launch found them (step {t})"
        got = (agent._flat(agent._online), agent._flat(agent._mu), agent._flat(agent._nu))
        fig = T.chain_errors(all_losses, got, o64, row.K, T.hyper()["lr"])
        print(rid, "chained: shares of the loss / parameter bars, relative mu / nu deviation:", {k: f"{v:.3g}" for k, v in fig.items()})
        assert fig["loss"] <= 1.0 and fig["param"] <= 1.0, fig
        assert fig["mu"] <= T.MOMENT_RTOL and fig["nu"] <= T.MOMENT_RTOL, fig
        assert (agent._count.cpu().numpy() == T.N_STEPS_CHAIN).all()
    agent._destroy_handle()


@pytest.mark.parametrize("rid", T.IDS)
def test_row_against_oracle(rid, monkeypatch):
    monkeypatch.delenv("IDQN_CONV", raising=False)
    monkeypatch.delenv("IDQN_IQN_ADAM_FUSE", raising=False)
    _run_row(rid, True)


@pytest.mark.parametrize("rid", T.FUSE_OFF_ROWS)
def test_fused_row_as_two_splits(rid, monkeypatch):
    """IDQN_IQN_ADAM_FUSE=0: the two-split launch + Adam pass at group counts the planner never gives it.  Against the oracle, not
    against the fused run: the number of splits differs, and with it the summation order."""
    monkeypatch.delenv("IDQN_CONV", raising=False)
    monkeypatch.setenv("IDQN_IQN_ADAM_FUSE", "0")
    assert T.route(T.BY_ID[rid]) == "fused" and T.route(T.BY_ID[rid], False) == "two-split"
    _run_row(rid, False)


@pytest.mark.parametrize("rid", T.WEIGHTED_ROWS)
def test_weighted_step(rid, monkeypatch):
    """Importance weights and the priority signal on one row per route: loss, every leaf gradient (read off mu) and td_abs against
    ``test_iqn_per_host.weighted_iqn_loss``, bars as tests/test_gpu_iqn_per.py has them."""
    import torch

    from oracle import qnet_ref as Q
    from slimdqn import _hip
    from test_iqn_per_host import weighted_iqn_loss

    monkeypatch.delenv("IDQN_CONV", raising=False)
    monkeypatch.delenv("IDQN_IQN_ADAM_FUSE", raising=False)
    row = T.BY_ID[rid]
    K, B, hy = row.K, row.B, T.hyper()
    p, pt = T.params(rid)
    batch, taus = T.step_inputs(rid, 0)
    w = np.random.default_rng(3).uniform(0.05, 1.0, B).astype(np.float32)
    agent = _agent(row)
    agent._ensure_handle(B)
    w_dev, td_dev = torch.from_numpy(w).cuda(), torch.zeros((K, B), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    losses, names = _profiled_step(agent, batch, taus)
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    assert T.dense0_launches(names) == T.expected_route(row), (rid, T.dense0_launches(names), T.expected_route(row))
    td = td_dev.cpu().numpy()
    mu = agent._flat(agent._mu)
    want, want_td, grads = np.zeros(K), np.zeros((K, B)), {}
    for k in range(K):
        want[k], g, _, want_td[k] = weighted_iqn_loss(Q.head(p, k), Q.head(pt, k), batch, tuple(taus[k]), hy["gamma"] ** hy["n"], w)
        for leaf in g:
            grads.setdefault(leaf, []).append(g[leaf])
    assert np.abs(losses - want).max() <= T.LOSS_RTOL * max(1.0, np.abs(want).max()), (losses, want)
    np.testing.assert_allclose(td, want_td, rtol=T.TD_RTOL, atol=T.TD_ATOL)
    worst = 0.0
    for leaf in grads:
        wg = np.stack(grads[leaf]).reshape(K, -1)
        g = mu[leaf].reshape(K, -1) / (1.0 - 0.9)
        scale = np.abs(wg).max(1)[:, None]
        worst = max(worst, float((np.abs(g - wg) / scale).max()))
        assert (np.abs(g - wg) <= T.GRAD_RTOL * scale + 1e-12).all(), (leaf, np.abs(g - wg).max(), scale.max())
    print(rid, T.route(row), "weighted: max |td_abs - want|", np.abs(td - want_td).max(), "worst gradient deviation", worst)
    assert (agent._count.cpu().numpy() == 1).all()
    if T.route(row) == "fused":
        assert (_gate_words(agent) == 0).all()
    agent._destroy_handle()


@pytest.mark.parametrize("rid", T.ACT_ROWS)
def test_acting_past_32_fractions(rid, monkeypatch):
    monkeypatch.delenv("IDQN_CONV", raising=False)
    row = T.BY_ID[rid]
    K, N = row.K, row.N
    states, taus = T.act_inputs(rid)
    n = len(states)
    want = T.acting_oracle(rid)
    agent = _agent(row)
    failures, worst = [], 0.0

    def check(q, w, what):
        nonlocal worst
        q, w = np.asarray(q, np.float64).reshape(w.shape), np.asarray(w, np.float64)
        err = np.abs(q - w).max(axis=-1) / np.maximum(1.0, np.abs(w).max(axis=-1))
        worst = max(worst, float(err.max()))
        if not (err <= T.ACT_Q_RTOL).all():
            failures.append((what, float(err.max())))

    for which in (0, 1):
        arena = agent.params if which == 0 else agent.target_params
        for k in range(K):
            w = want[(which, k)]
            check(agent.q_values(arena, states, k, taus=np.ascontiguousarray(taus.T)).cpu().numpy(), w, f"idqn_iqn_q_values {which} {k}")
            agent._iqn_q(which, k, states, np.ascontiguousarray(taus.T), want_action=True)
            acts = agent._action_out[:n].cpu().numpy()
            if not np.array_equal(acts, w.argmax(1)):
                failures.append(("idqn_iqn_q_values action", which, k, acts.tolist(), w.argmax(1).tolist()))
            for e in sorted({0, min(1, n - 1), n - 1}):
                act = int(agent._act_host(which, k, np.asarray(states[e]), taus[e][:, None], None))
                check(agent._q_out[0].cpu().numpy(), w[e], f"idqn_iqn_act_host {which} {k} {e}")
                if act != int(w[e].argmax()):
                    failures.append(("idqn_iqn_act_host action", which, k, e, act, int(w[e].argmax())))
        hd = [e % K for e in range(n)]
        acts = agent._act_host_many(which, hd, [np.asarray(s) for s in states], taus)
        assert agent.__dict__.get("_iqn_act_many_ok") is True, "the batched entry was refused: this is the loop"
        w = np.stack([want[(which, hd[e])][e] for e in range(n)])
        check(agent._q_out[:n].cpu().numpy(), w, f"idqn_iqn_act_host_many {which}")
        if not np.array_equal(np.asarray(acts), w.argmax(1)):
            failures.append(("idqn_iqn_act_host_many action", which, np.asarray(acts).tolist(), w.argmax(1).tolist()))
    print(rid, "acting: largest Q deviation relative to max(1, max |q|):", f"{worst:.3g}")
    agent._destroy_handle()
    assert not failures, failures
