"""GPU: i-IQN with prioritized replay and the replay-sourced i-IQN step (extension, parity unpinned: the reference has no
quantile code and cannot learn from priorities).

* the importance-weighted quantile Huber loss, its gradients and the priority signal td_abs against the fp64 autograd checker
  of ``tests/test_iqn_per_host.py`` (itself pinned to ``oracle/iqn_ref.py`` there).  Bars are the ones of the unweighted step
  (``test_gpu_iqn.py`` / ``test_gpu_iqn_batches.py``): per-head loss within 1e-5 relative to max(1, |loss|), every leaf gradient
  within 3e-5 of its largest entry; td_abs within rtol 2e-5 / atol 2e-6 (``test_gpu_per_extension.py``);
* bit-exact metamorphic relations between the weighted and the plain step;
* ``idqn_iqn_learn_on_replay`` / ``_dev`` bit for bit against ``replay_gather_stacked`` + ``idqn_iqn_learn_on_batch``;
* ``PrioritizedLearner`` with an ``iIQN`` agent, gathered and replay-sourced;
* the refusals of the new entries.
"""
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest

from test_iqn_per_host import weighted_iqn_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ATARI = ((84, 84, 4), 6, [32, 64, 64, 512])


def _golden_tool():
    spec = importlib.util.spec_from_file_location("mk", os.path.join(ROOT, "tools", "make_iqn_batch_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def _iiqn(obs, A, feats, K, N, hy, seed=0):
    from slimdqn.networks.iiqn import iIQN

    return iIQN(seed, obs, A, K, feats, "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"], n_quantiles=N)


def _small_case(B):
    """The small shape of test_gpu_iqn.py (``iqn_small``) at B samples, inputs built the way ``iqn_case_inputs`` builds them and
    conditioned the way tools/make_iqn_batch_golden.py conditions its case: a sample with an online ReLU pre-activation within
    MARGIN of zero (where fp32 and fp64 may take different branches) gets a fresh state and fresh online fractions."""
    from oracle import iqn_ref as I
    from oracle import make_golden as G
    from oracle import qnet_ref as Q

    mk = _golden_tool()
    obs, A, feats, K, _, N = G.IQN_CASES["iqn_small"]
    seed = 4000 + B
    p, pt = I.init_params(seed, obs, A, feats, K), I.init_params(seed + 1, obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(seed + 10, B, obs, A, "cnn")
    term[0] = True
    term[B - 1] = True
    taus = I.synthetic_taus(seed + 20, K, N, B)
    for rnd in range(50):
        bad = np.zeros(B, bool)
        for k in range(K):
            bad |= mk._min_preact(Q.head(p, k), st, taus[k, 0]) < mk.MARGIN
        if not bad.any():
            break
        for b in np.flatnonzero(bad):
            mk._replace(st, taus, seed, rnd, int(b))
    else:
        raise RuntimeError("no well-conditioned inputs found")
    return (obs, A, feats, K, N), p, pt, (st, a, r, s2, term), taus


def _atari_case():
    mk = _golden_tool()
    obs, A, feats, K, B, N = mk.CASES["iqn_atari_k5_b64"]
    p, pt, batch, taus = mk.case_inputs("iqn_atari_k5_b64")  # (the committed golden's conditioned inputs)
    return (obs, A, feats, K, N), p, pt, batch, taus


def _per_step(agent, batch, taus, weights=None, td=None):
    """One ``_learn`` with the given prioritized-replay buffers on the handle (device tensors or None), cleared afterwards."""
    from slimdqn import _hip

    B = int(np.asarray(batch.action).shape[0])
    agent._ensure_handle(B)
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(weights), _hip.ptr(td)), "idqn_set_per_buffers")
    try:
        return agent._learn(batch, taus=taus).cpu().numpy().copy()
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")


@pytest.mark.parametrize("case,B", [("small", 32), ("small", 45), ("atari", 64)])
def test_weighted_loss_priorities_and_gradients_match_the_checker(case, B):
    import torch

    from oracle import make_golden as G
    from oracle import qnet_ref as Q

    (obs, A, feats, K, N), p, pt, batch, taus = _small_case(B) if case == "small" else _atari_case()
    assert batch[0].shape[0] == B
    hy = G.FP_HYPER
    w = np.random.default_rng(3).uniform(0.05, 1.0, B).astype(np.float32)
    agent = _iiqn(obs, A, feats, K, N, hy)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    w_dev, td_dev = torch.from_numpy(w).cuda(), torch.zeros((K, B), dtype=torch.float32, device="cuda")
    losses = _per_step(agent, Batch(*batch), taus, w_dev, td_dev)
    td = td_dev.cpu().numpy()
    mu = agent._flat(agent._mu)  # first step from zero Adam state: mu = (1 - b1) g
    want, want_td, grads = np.zeros(K), np.zeros((K, B)), {}
    for k in range(K):
        want[k], g, _, want_td[k] = weighted_iqn_loss(Q.head(p, k), Q.head(pt, k), batch, tuple(taus[k]), hy["gamma"] ** hy["n"], w)
        for leaf in g:
            grads.setdefault(leaf, []).append(g[leaf])
    print("losses", losses, "want", want, "max |td_abs - want|", np.abs(td - want_td).max(), "td_abs range", want_td.min(), want_td.max())
    assert np.abs(losses - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (losses, want)
    np.testing.assert_allclose(td, want_td, rtol=2e-5, atol=2e-6)
    for leaf in grads:
        wg = np.stack(grads[leaf]).reshape(K, -1)
        g = mu[leaf].reshape(K, -1) / (1.0 - 0.9)
        scale = np.abs(wg).max(1)[:, None]
        print(leaf, "max |g - want| / scale", (np.abs(g - wg) / scale).max())
        assert (np.abs(g - wg) <= 3e-5 * scale + 1e-12).all(), (leaf, np.abs(g - wg).max(), scale.max())
    assert (agent._count.cpu().numpy() == 1).all()


@pytest.mark.parametrize("B", [32, 45])
def test_weighted_step_metamorphic_bit_exact(B):
    """N = 16: every GEMM kernel and every grouped kernel of the heads runs.  Two steps each from the same state."""
    import torch

    from slimdqn import _hip

    rng = np.random.default_rng(30 + B)
    obs, A, K, N, feats = (20, 20, 4), 4, 2, 16, [32, 64, 32, 256]
    hy = {"lr": 2.5e-4, "gamma": 0.99, "n": 1, "eps": 1e-6}
    s = rng.integers(0, 256, size=(B,) + obs, dtype=np.uint8)
    s2 = rng.integers(0, 256, size=(B,) + obs, dtype=np.uint8)
    batch = Batch(s, rng.integers(0, A, size=B).astype(np.int32), rng.standard_normal(B).astype(np.float32), s2, rng.random(B) < 0.1)
    taus = [rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01 for _ in range(2)]
    SENTINEL, PAD = -7.0, 64

    def run(weights, with_td, set_and_clear_first=False):
        agent = _iiqn(obs, A, feats, K, N, hy, seed=11)
        w_dev = None if weights is None else torch.from_numpy(weights).cuda()
        td_dev = torch.full((K * B + PAD,), SENTINEL, dtype=torch.float32, device="cuda") if with_td else None
        if set_and_clear_first:
            scratch = torch.zeros(K * B, dtype=torch.float32, device="cuda")
            agent._ensure_handle(B)
            _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(scratch), _hip.ptr(scratch)), "set")
            _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "clear")
        losses, tds = [], []
        for t in taus:
            losses.append(_per_step(agent, batch, t, w_dev, td_dev))
            tds.append(None if td_dev is None else td_dev.cpu().numpy().copy())
        return losses, agent._flat(agent._online), agent._flat(agent._mu), tds

    def same(a, b):
        for la, lb in zip(a[0], b[0]):
            np.testing.assert_array_equal(la, lb)
        for leaf in a[1]:
            np.testing.assert_array_equal(a[1][leaf], b[1][leaf], err_msg=leaf)
            np.testing.assert_array_equal(a[2][leaf], b[2][leaf], err_msg=leaf)

    plain = run(None, False)
    ones = run(np.ones(B, np.float32), True)
    td_only = run(None, True)
    cleared = run(None, False, set_and_clear_first=True)
    weighted = run(rng.uniform(0.05, 1.0, B).astype(np.float32), True)
    same(plain, ones)      # all-ones weights: the unweighted step
    same(plain, td_only)   # writing priorities changes nothing else
    same(plain, cleared)   # set + clear: the plain launch again
    for a, b in zip(ones[3], td_only[3]):
        np.testing.assert_array_equal(a, b)
    # the priority signal does not depend on the weights (first step: the same parameters)
    np.testing.assert_array_equal(weighted[3][0], td_only[3][0])
    assert not np.array_equal(weighted[0][0], plain[0][0])  # (the weights did act on the loss)
    for tds in (ones[3], td_only[3], weighted[3]):
        for td in tds:
            assert (td[K * B :] == SENTINEL).all(), "td_abs entries past [K][batch] were written"
            assert np.isfinite(td[: K * B]).all() and (td[: K * B] > 0).all()


def _filled_buffer(sampler, B, obs_hw=(84, 84), A=6, capacity=300, n=700, priority=False):
    """More transitions than the ring holds (slots and frames have wrapped), episode ends every 37 transitions."""
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    rb = ReplayBuffer(sampler, batch_size=B, max_capacity=capacity, stack_size=4, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(9)
    for i in range(n):
        tr = TransitionElement(rng.integers(0, 256, obs_hw, dtype=np.uint8), int(rng.integers(A)), float(rng.normal()),
                               bool(i % 37 == 36), False)
        rb.add(tr, **({"priority": float(rng.random() + 0.1)} if priority else {}))
    rb.reuse_sample_buffers = True
    return rb


def _state_arrays(agent):
    return {n: getattr(agent, n).cpu().numpy().copy() for n in ("_online", "_mu", "_nu", "_count", "_losses", "_cum")}


@pytest.mark.parametrize("B", [32, 96])
def test_learn_on_replay_is_gather_then_learn(B):
    import torch

    from slimdqn import _hip
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    obs, A, feats = ATARI
    K, N = 2, 8
    hy = {"lr": 6.25e-5, "gamma": 0.99, "n": 1, "eps": 1.5e-4}
    rb = _filled_buffer(UniformSamplingDistribution(5), B)
    rng = np.random.default_rng(12)
    steps = []
    saw_episode_start = False
    for _ in range(3):
        slots = rb.sample_slots()
        st = np.asarray(rb._gather(slots).state)
        saw_episode_start |= bool((st[..., 0].reshape(B, -1) == 0).all(1).any())  # a zero frame before an episode start
        steps.append((slots, rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01))
    assert saw_episode_start, "no sampled stack holds an episode start"
    assert rb.add_count > rb._max_capacity  # the ring has wrapped
    out = {}
    for form in ("two_calls", "host_slots", "dev_slots"):
        agent = _iiqn(obs, A, feats, K, N, hy, seed=3)
        losses = []
        for slots, taus in steps:
            if form == "two_calls":
                agent._learn(rb._gather(slots), taus=taus)  # replay_gather_stacked, then idqn_iqn_learn_on_batch
            else:
                kw = {"slots_host": slots} if form == "host_slots" else {"slots_dev": torch.from_numpy(slots).cuda()}
                _hip.check(agent._learn_on_replay(rb.ring_view(), taus=taus, **kw), "idqn_iqn_learn_on_replay")
            losses.append(agent._losses.cpu().numpy().copy())
        out[form] = (losses, _state_arrays(agent))
        del agent
    assert np.isfinite(np.asarray(out["two_calls"][0])).all()
    for form in ("host_slots", "dev_slots"):
        for la, lb in zip(out["two_calls"][0], out[form][0]):
            np.testing.assert_array_equal(la, lb, err_msg=form)
        for name, want in out["two_calls"][1].items():
            np.testing.assert_array_equal(out[form][1][name], want, err_msg=f"{form} {name}")
    assert (out["two_calls"][1]["_count"] == 3).all()


def test_update_online_params_fused_and_two_calls(monkeypatch):
    """The switch is read on every call: one process runs both settings, each from the same seeds."""
    import torch

    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    obs, A, feats = ATARI
    K, N, B = 2, 8, 32
    hy = {"lr": 6.25e-5, "gamma": 0.99, "n": 1, "eps": 1.5e-4}
    out = {}
    for setting in ("0", "1"):
        monkeypatch.setenv("IDQN_LEARN_ON_REPLAY", setting)
        rb = _filled_buffer(UniformSamplingDistribution(5), B)
        agent = _iiqn(obs, A, feats, K, N, hy, seed=3)
        for step in range(4):
            agent.update_online_params(step, rb)
        torch.cuda.synchronize()
        assert agent.__dict__.get("_replay_fused_ok") is (True if setting == "1" else None), "the wrong path ran"
        out[setting] = (_state_arrays(agent), rb._sampling_distribution._rng_key.bit_generator.state,
                        agent._tau_rng.bit_generator.state)
        del agent
    for name, want in out["0"][0].items():
        np.testing.assert_array_equal(out["1"][0][name], want, err_msg=name)
    assert np.isfinite(out["1"][0]["_losses"]).all() and (out["1"][0]["_count"] == 4).all()
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]  # the same draws from both generators


def test_prioritized_learner_with_iiqn(monkeypatch):
    """20 prioritized steps, gathered (switch off) and replay-sourced, from the same seeds: identical parameters and an
    identical sum tree; the written priorities are (mean_k td_abs + eps)^alpha of the step's read-back td_abs."""
    import torch

    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler

    obs, A, K, N, B, cap = (20, 20, 4), 5, 2, 8, 32, 64
    hy = {"lr": 1e-3, "gamma": 0.99, "n": 1, "eps": 1e-8}
    out = {}
    for setting in ("0", "1"):
        monkeypatch.setenv("IDQN_LEARN_ON_REPLAY", setting)
        sampler = SlotPrioritizedSampler(0, cap, priority_exponent=0.6)
        rb = _filled_buffer(sampler, B, obs_hw=(20, 20), A=A, capacity=cap, n=150)
        agent = _iiqn(obs, A, [32, 32, 32, 256], K, N, hy, seed=2)
        learner = PrioritizedLearner(agent, rb, beta=0.5, eps=1e-3, reduce="mean")
        assert (learner._replay_sourced() is not None) == (setting == "1")
        tree = sampler._sum_tree
        losses = []
        for _ in range(20):
            losses.append(learner.step().cpu().numpy().copy())
            # the step's priorities, recomputed from its td_abs
            lv = learner._leaves.cpu().numpy()
            td = learner._td_abs.cpu().numpy().astype(np.float64)
            assert np.isfinite(td).all() and (td > 0).all()
            want = (td.mean(0) + 1e-3) ** 0.6
            np.testing.assert_allclose(learner._priorities.cpu().numpy(), want, rtol=1e-12)
            got = tree._nodes[tree._first_leaf_offset + lv]
            first = {}
            for pos, leaf in enumerate(lv):  # duplicates: the first occurrence wins (SumTree.set semantics)
                first.setdefault(int(leaf), pos)
            for leaf, pos in first.items():
                assert abs(got[pos] - want[pos]) <= 1e-12 * want[pos]
        torch.cuda.synchronize()
        assert np.isfinite(np.asarray(losses)).all()
        assert agent.__dict__.get("_replay_fused_ok") is (True if setting == "1" else None), "the wrong path ran"
        out[setting] = (losses, _state_arrays(agent), tree._nodes.copy())
        del learner, agent
    for la, lb in zip(out["0"][0], out["1"][0]):
        np.testing.assert_array_equal(la, lb)
    for name, want in out["0"][1].items():
        np.testing.assert_array_equal(out["1"][1][name], want, err_msg=name)
    np.testing.assert_array_equal(out["0"][2], out["1"][2])
    assert (out["1"][1]["_count"] == 20).all()


def test_replay_entry_refusals():
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    obs, A, K, N, B = (20, 20, 4), 5, 2, 4, 32
    hy = {"lr": 1e-3, "gamma": 0.99, "n": 1, "eps": 1e-8}
    rb = _filled_buffer(UniformSamplingDistribution(1), B, obs_hw=(20, 20), A=A, capacity=64, n=100)
    frames, n_frames, frame_bytes, rows, stack = rb.ring_view()[:5]
    slots = np.ascontiguousarray(rb.sample_slots(), np.int32)
    slots_dev = torch.from_numpy(slots).cuda()
    tau = torch.full((K * 3 * N * 512,), 0.5, dtype=torch.float32, device="cuda")
    agent = _iiqn(obs, A, [32, 32, 32, 256], K, N, hy)
    agent._ensure_handle(B)
    plain = iDQN(0, obs, A, K, [32, 32, 32, 256], "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9)
    plain._ensure_handle(B)
    lib, q = _hip.lib(), _hip.current_stream()

    def call(dev, handle, batch=B, stk=4, flags=0):
        fn = lib.idqn_iqn_learn_on_replay_dev if dev else lib.idqn_iqn_learn_on_replay
        return fn(handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows),
                  _hip.ptr(slots_dev) if dev else slots.ctypes.data, _hip.ptr(tau), batch, stk, flags, q)

    before = _state_arrays(agent)
    for dev in (False, True):
        name = "idqn_iqn_learn_on_replay_dev" if dev else "idqn_iqn_learn_on_replay"
        for kwargs, match in ((dict(handle=plain._handle), "without quantile heads"), (dict(handle=agent._handle, batch=257), "batch 257"),
                              (dict(handle=agent._handle, stk=3), "stack 3"), (dict(handle=agent._handle, flags=_hip.F_GRADS_ONLY), "profile flags")):
            rc = call(dev, **kwargs)
            assert rc == _hip.E_INVALID, (name, kwargs, rc)
            msg = lib.idqn_last_error().decode()
            assert msg.startswith(name + ":") and match in msg, msg
    torch.cuda.synchronize()
    for n, want in before.items():  # a refused call enqueued nothing
        np.testing.assert_array_equal(getattr(agent, n).cpu().numpy(), want, err_msg=n)
    # and the accepted call runs
    _hip.check(call(True, agent._handle), "idqn_iqn_learn_on_replay_dev")
    assert np.isfinite(agent._losses.cpu().numpy()).all() and (agent._count.cpu().numpy() == 1).all()
