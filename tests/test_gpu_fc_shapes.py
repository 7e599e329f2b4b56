"""GPU: the one-launch MLP step ``k_fc_step_par`` against the fp64 oracle at every boundary of its LDS plan.

Every descendant of fc_step_par, csrc/fc_par_kernels.h (the ring-sourced step, the persistent n-step kernel, seed groups, prioritized seed
groups, grouped acting) is pinned to ``k_fc_step_par<FcBatchSrc>`` byte for byte, so the oracle reaches the family through
this kernel only -- and which kernel a step ran was not observable.  Here every row of tests/fc_shapes.py

* asserts the ROUTE: ``idqn_profile_read`` names the kernel the step launched (``k_fc_step_par`` for the inside rows, the named
  fallback for the nearest shape on the other side of each limit, a refused create for ``features = []``);
* holds losses, every leaf gradient, the weighted loss / gradients / |TD|, three chained Adam steps (losses, ``cum``, counts,
  parameters, both moments), both nets' Q-values and the greedy actions to ``oracle/qnet_ref.py`` in fp64;
* and, for the ragged batches, requires that rows ``B..31`` carry nothing over from an earlier full batch.

The bars are the project's own (tests/fc_shapes.py lists where each comes from); tests/test_fc_shapes_host.py shows on the CPU that
the fp32 oracle alone uses at most half of each for every row.  None is taken from what the GPU gave: the observed errors are
only printed (``-s``).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import fc_shapes as F

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
RUN_IDS = [r.id for r in F.RUNNABLE]
INSIDE_IDS = [r.id for r in F.INSIDE]


def _agent(row, load=True):
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    if row.id == "K1_dqn":
        agent = DQN(0, row.d0, row.A, row.feats, "fc", F.LR, F.GAMMA, F.N_STEP, 1, 10**9, adam_eps=row.eps)
    else:
        agent = iDQN(0, row.d0, row.A, row.K, row.feats, "fc", F.LR, F.GAMMA, F.N_STEP, 1, 10**9, 10**9, adam_eps=row.eps)
    if load:
        p, pt, _, _ = F.inputs(row.id)
        agent._load_flat(agent._online, p)
        agent._load_flat(agent._target, pt)
    return agent


def route(agent):
    """The kernel the handle's last MLP step launched (idqn_profile_read; the event spans it also returns are dropped)."""
    from slimdqn import _hip

    mean_ms, n, name = C.c_double(), C.c_int32(), C.create_string_buffer(64)
    _hip.check(_hip.lib().idqn_profile_read(agent._handle, C.byref(mean_ms), C.byref(n), name), "idqn_profile_read")
    return name.value.decode()


def _check_grads(row, agent, losses, want, what, errs):
    G = agent._flat_grad()
    for k in range(row.K):
        loss, grads, _ = want[k]
        errs[what + " loss"] = max(errs.get(what + " loss", 0.0), abs(float(losses[k]) - loss))
        assert abs(float(losses[k]) - loss) <= F.LOSS_ATOL, (what, k, float(losses[k]), loss)
        for leaf, g in grads.items():
            e = F.rel_to_max(G[leaf][k], g)
            errs[what + " grad"] = max(errs.get(what + " grad", 0.0), e)
            assert e <= F.GRAD_RTOL, (what, k, leaf, e)


@pytest.mark.parametrize("rid", RUN_IDS)
def test_route_and_gradients_plain_and_weighted(rid):
    import torch

    from slimdqn import _hip

    row = F.BY_ID[rid]
    _, _, batches, w = F.inputs(rid)
    ref = F.oracle(rid)
    agent, errs = _agent(row), {}
    batch = Batch(*batches[0])
    losses = agent._learn(batch, flags=_hip.F_GRADS_ONLY | _hip.F_PROFILE).cpu().numpy()
    assert route(agent) == row.route, row.why
    _check_grads(row, agent, losses, ref["plain"], "plain", errs)
    assert agent._count.cpu().numpy().tolist() == [0] * row.K
    # importance weights and |TD| (the prioritized-replay extension), then the plain mean again
    w_dev, td_dev = torch.from_numpy(w).cuda(), torch.zeros((row.K, row.B), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    losses = agent._learn(batch, flags=_hip.F_GRADS_ONLY | _hip.F_PROFILE).cpu().numpy()
    assert route(agent) == row.route
    _check_grads(row, agent, losses, ref["weighted"], "weighted", errs)
    td = td_dev.cpu().numpy()
    for k in range(row.K):
        want = np.abs(ref["weighted"][k][2]["td"])
        errs["td"] = max(errs.get("td", 0.0), float(np.abs(td[k] - want).max()))
        np.testing.assert_allclose(td[k], want, rtol=F.TD_RTOL, atol=F.TD_ATOL)
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    losses = agent._learn(batch, flags=_hip.F_GRADS_ONLY).cpu().numpy()
    _check_grads(row, agent, losses, ref["plain"], "plain again", errs)
    print(rid, {k: f"{v:.3g}" for k, v in errs.items()})


@pytest.mark.parametrize("rid", RUN_IDS)
def test_three_chained_steps(rid):
    """Counts 0, 1, 2 on three different batches: the second and third steps start from non-zero moments."""
    from slimdqn import _hip

    row = F.BY_ID[rid]
    _, _, batches, _ = F.inputs(rid)
    ref = F.oracle(rid)
    agent, errs = _agent(row), {"loss": 0.0, "param": 0.0, "moment": 0.0}
    for i, b in enumerate(batches):
        losses = agent._learn(Batch(*b), flags=_hip.F_PROFILE).cpu().numpy()
        assert route(agent) == row.route, (i, row.why)
        errs["loss"] = max(errs["loss"], float(np.abs(losses - ref["losses"][i]).max()))
        assert np.abs(losses - ref["losses"][i]).max() <= F.LOSS_ATOL, (i, losses, ref["losses"][i])
    cum = agent._cum.cpu().numpy()
    errs["cum"] = float(np.abs(cum - ref["cum"]).max())
    assert errs["cum"] <= F.LOSS_ATOL * F.N_STEPS_CHAIN
    assert agent._count.cpu().numpy().tolist() == [F.N_STEPS_CHAIN] * row.K
    got_p, got_m, got_v = agent._flat(agent._online), agent._flat(agent._mu), agent._flat(agent._nu)
    for leaf in ref["p"]:
        e = float(np.abs(got_p[leaf] - ref["p"][leaf]).max())
        errs["param"] = max(errs["param"], e)
        assert e <= F.PARAM_ATOL, (leaf, e)
        for k in range(row.K):
            for what, got, want in (("mu", got_m, ref["mu"]), ("nu", got_v, ref["nu"])):
                e = F.rel_to_max(got[leaf][k], want[leaf][k])
                errs["moment"] = max(errs["moment"], e)
                assert e <= F.MOMENT_RTOL, (what, leaf, k, e)
    print(rid, {k: f"{v:.3g}" for k, v in errs.items()})


@pytest.mark.parametrize("rid", RUN_IDS)
def test_q_values_and_greedy_actions(rid):
    row = F.BY_ID[rid]
    _, _, batches, _ = F.inputs(rid)
    ref = F.oracle(rid)
    agent = _agent(row)
    states = batches[0][0][: min(row.B, 32)]
    n, worst = len(states), 0.0
    for which, key in ((0, "q"), (1, "qt")):
        for k in range(row.K):
            got = agent._q_values(which, k, states).cpu().numpy()
            want = ref[key][k][:n]
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= F.Q_RTOL * max(1.0, float(np.abs(want).max())), (key, k, err)
    for k in sorted({0, row.K - 1}):
        for i in range(min(n, 4)):
            act = int(agent._best_action(0, k, states[i]).item())
            q64 = ref["q"][k][i]
            top = np.sort(q64)[::-1]
            if row.A == 1 or top[0] - top[1] > F.GAP:
                assert act == int(np.argmax(q64)), (k, i, act, q64)
            else:
                assert q64.max() - q64[act] <= 1e-5, (k, i, act, q64)
    print(rid, f"q err {worst:.3g}")


@pytest.mark.parametrize("rid", F.TIE_ROWS)
def test_ties_take_the_first_maximum(rid):
    """A zero Q-head kernel and biases whose maximum stands at indices 2 and 5: action 2 on every acting entry (A = 1: 0)."""
    row = F.BY_ID[rid]
    p, pt, batches, _ = F.inputs(rid)
    flat = {n: v.copy() for n, v in p.items()}
    last = len(row.feats)
    flat[f"Dense_{last}/kernel"][:] = 0.0
    bias = np.full(row.A, -1.0, np.float32)
    want = 0
    if row.A > 1:
        bias[[2, 5]] = 0.5
        want = 2
    flat[f"Dense_{last}/bias"][:] = bias
    agent = _agent(row)
    agent._load_flat(agent._online, flat)
    states = batches[0][0][:4]
    for k in sorted({0, row.K - 1}):
        assert int(agent._best_action(0, k, states[0]).item()) == want
        q = agent._q_values(0, k, states).cpu().numpy()
        assert (np.argmax(q, axis=1) == want).all() and (q == bias[None]).all()
    heads = [0, row.K - 1, 0, row.K - 1]
    assert agent._best_actions(0, heads, list(states)).tolist() == [want] * 4


STATE = ("_online", "_mu", "_nu", "_losses", "_cum", "_count", "_grad")


def _snapshot(agent):
    import torch

    torch.cuda.synchronize()
    return {n: getattr(agent, n).cpu().numpy().tobytes() for n in STATE}


@pytest.mark.parametrize("rid", F.RAGGED)
def test_pad_rows_carry_nothing_over_from_a_full_batch(rid):
    """A B = 32 step with rewards x 1000 on the same handle, state restored, then the ragged step: byte for byte the fresh
    agent's ragged step (rows B..31 are zero inputs with zero loss weight, whatever ran before)."""
    from oracle import qnet_ref as Q

    row = F.BY_ID[rid]
    _, _, batches, _ = F.inputs(rid)
    ragged = Batch(*batches[0])
    fresh = _agent(row)
    fresh._learn(ragged)
    assert route(fresh) == F.PAR
    want = _snapshot(fresh)
    used = _agent(row)
    keep = {n: getattr(used, n).clone() for n in ("_online", "_mu", "_nu", "_cum", "_count")}
    s, a, r, s2, t = Q.synthetic_batch(99, 32, row.d0, row.A, "fc")
    used._learn(Batch(s, a, (r + 0.5) * 1000.0, s2, t))
    assert route(used) == F.PAR and (used._count.cpu().numpy() == 1).all()
    for n, v in keep.items():
        getattr(used, n).copy_(v)
    used._learn(ragged)
    got = _snapshot(used)
    for n in STATE:
        assert got[n] == want[n], f"{n} differs after a poisoned full batch"


@pytest.mark.parametrize("rid", [r.id for r in F.REFUSED])
def test_refused_shapes_are_refused_with_their_message(rid):
    """``features = []``: the reference's DQNNet accepts it, idqn_create (build_layout) does not -- recorded, not dropped."""
    from slimdqn import _hip

    with pytest.raises(_hip.HipExtensionError, match=F.REFUSAL_NO_HIDDEN):
        _agent(F.BY_ID[rid], load=False)


def test_the_n_step_entry_names_its_route():
    """``idqn_learn_steps_on_replay_fc``: ``k_fc_steps_par`` for a net inside fc_steps_plan, the single step's ring-sourced name
    for the net that fits fc_par_plan only (the entry loops); a single ring-sourced step names ``k_fc_step_par<ring>``."""
    import test_gpu_fc_learn_steps as L

    for rid, want in ((F.DESCENDANT_ROWS[0], "k_fc_steps_par"), (F.DESCENDANT_LOOP_ROW, "k_fc_step_par<ring>")):
        name = "shape_" + rid
        rb = L._buffer(name)
        agent = L._agent(name)
        slots = np.random.default_rng(2).integers(0, L.CAPACITY, (3, L.CONFIGS[name][8])).astype(np.int32)
        L._many(agent, rb, slots)
        assert route(agent) == want
        L._single(agent, rb, slots[0])
        assert route(agent) == "k_fc_step_par<ring>"
        assert (agent._count.cpu().numpy() == 4).all()
