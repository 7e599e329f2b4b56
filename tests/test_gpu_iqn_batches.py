"""GPU parity of i-IQN steps on minibatches of more than 32 samples (up to 256): the heads run NB = N x ceil(B / 32) blocks
of 32 rows per virtual net, block s N + q holding fraction q of sample block s.  Bars as in test_gpu_iqn.py: per-head loss
within 1e-5 relative, every leaf gradient (read off mu after one step from zero Adam state) within 3e-5 of its largest
entry, post-Adam parameters within a fraction of lr."""
import json
import os
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
SMALL = ((20, 20, 4), 5, [32, 32, 32, 256], 2)  # obs, A, features, K


def _agent(obs, A, feats, K, N, hy, seed=0):
    from slimdqn.networks.iiqn import iIQN

    return iIQN(seed, obs, A, K, feats, "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"], n_quantiles=N)


def _small_inputs(N, B, seed):
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    obs, A, feats, K = SMALL
    p = I.init_params(seed, obs, A, feats, K)
    pt = I.init_params(seed + 1, obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(seed + 10, B, obs, A, "cnn")
    term[0] = True
    term[B - 1] = True
    return p, pt, (st, a, r, s2, term), I.synthetic_taus(seed + 20, K, N, B)


@pytest.mark.parametrize("N,B", [(16, 64), (16, 256), (5, 100), (8, 33)])
def test_iqn_batch_step_against_oracle(N, B):
    from oracle import iqn_ref as I
    from oracle import make_golden as G

    obs, A, feats, K = SMALL
    hy = G.FP_HYPER
    p, pt, batch, taus = _small_inputs(N, B, 100 + N + B)
    mu0 = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    nu0 = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    p64, _, _, _, want, grads = I.learn_on_batch(p, pt, mu0, nu0, np.zeros(K, np.int64), batch, taus, hy["gamma"] ** hy["n"],
                                                 hy["lr"], hy["eps"], np.float64, return_grads=True)
    agent = _agent(obs, A, feats, K, N, hy)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    losses = agent._learn(Batch(*batch), taus=taus).cpu().numpy()
    assert np.abs(losses - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (losses, want)
    mu, par = agent._flat(agent._mu), agent._flat(agent._online)
    for leaf in grads:
        wg = grads[leaf].reshape(K, -1)
        g = mu[leaf].reshape(K, -1) / (1.0 - 0.9)
        scale = np.abs(wg).max(1)[:, None]
        assert (np.abs(g - wg) <= 3e-5 * scale + 1e-12).all(), (leaf, np.abs(g - wg).max(), scale.max())
        wp, pp = p64[leaf].reshape(K, -1), par[leaf].reshape(K, -1)
        big = np.abs(wg) > 1e-3 * scale
        assert (np.abs(pp - wp)[big] <= 0.02 * hy["lr"] + 2e-7 * np.abs(wp[big])).all(), leaf
    assert (agent._count.cpu().numpy() == 1).all()


def test_iqn_batch_64_against_golden():
    """Full size (BASELINE config 3 with B = 64) against tools/make_iqn_batch_golden.py's fp64 probes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("mk", os.path.join(os.path.dirname(GOLDEN), "..", "tools", "make_iqn_batch_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    name = "iqn_atari_k5_b64"
    obs, A, feats, K, B, N = mk.CASES[name]
    p, pt, batch, taus = mk.case_inputs(name)
    rec = json.load(open(os.path.join(GOLDEN, f"fp_path_{name}.json")))
    hy = rec["hyper"]
    agent = _agent(obs, A, feats, K, N, hy)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    losses = agent._learn(Batch(*batch), taus=taus).cpu().numpy()
    want = np.asarray(rec["losses"])
    assert np.abs(losses - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), (losses, want)
    # the debug rows cover sample block 0
    dbg = agent._debug("iqn_dbg").cpu().numpy().reshape(K, 2 * N + 33, 32)[0]
    z_on, z_tg, a_star = dbg[:N], dbg[N : 2 * N], dbg[2 * N + 32]
    assert np.array_equal(a_star.astype(np.int64), np.asarray(rec["a_star_head0"])[:32])
    for got, key in ((z_on, "z_online_head0"), (z_tg, "z_target_head0")):
        w = np.asarray(rec[key])[:, :32]
        assert np.abs(got - w).max() <= 2e-5 * max(1.0, np.abs(w).max()), key
    mu, par = agent._flat(agent._mu), agent._flat(agent._online)
    for leaf, r in rec["leaves"].items():
        idx = np.asarray(r["idx"])
        g = mu[leaf].reshape(K, -1)[:, idx] / (1.0 - 0.9)
        wg, scale = np.asarray(r["grad"]), np.asarray(r["grad_absmax"])[:, None]
        assert (np.abs(g - wg) <= 3e-5 * scale + 1e-12).all(), (leaf, np.abs(g - wg).max(), scale.max())
        wp = np.asarray(r["param"])
        big = np.abs(wg) > 1e-3 * scale
        assert (np.abs(par[leaf].reshape(K, -1)[:, idx] - wp)[big] <= 0.02 * hy["lr"] + 2e-7 * np.abs(wp[big])).all(), leaf


def _atari_batch(rng, B, A=6):
    obs = (84, 84, 4)
    s = rng.integers(0, 256, size=(B,) + obs, dtype=np.uint8)
    s2 = rng.integers(0, 256, size=(B,) + obs, dtype=np.uint8)
    return Batch(s, rng.integers(0, A, size=B).astype(np.int32), rng.standard_normal(B).astype(np.float32), s2, rng.random(B) < 0.1)


def test_iqn_batch_256_reproducible():
    """B = 256 at full size: four steps twice from the same state end with identical bits (every cross-workgroup sum is in a
    fixed order), finite losses, and Dense_0/kernel's second moments moved."""
    from slimdqn.networks.iiqn import iIQN

    rng = np.random.default_rng(21)
    K, N, B = 5, 32, 256
    batch = _atari_batch(rng, B)
    taus = [rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01 for _ in range(4)]
    runs = []
    for _ in range(2):
        agent = iIQN(5, (84, 84, 4), 6, K, [32, 64, 64, 512], "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
        losses = [agent._learn(batch, taus=t).cpu().numpy().copy() for t in taus]
        runs.append((losses, agent._flat(agent._online), agent._flat(agent._nu)["Dense_0/kernel"]))
        del agent
    for la, lb in zip(runs[0][0], runs[1][0]):
        assert np.isfinite(la).all() and np.array_equal(la, lb)
    for leaf in runs[0][1]:
        assert np.array_equal(runs[0][1][leaf], runs[1][1][leaf]), leaf
    assert np.array_equal(runs[0][2], runs[1][2]) and np.abs(runs[0][2]).max() > 0


def test_iqn_batch_block_order_invariance():
    """Full size, B = 64: swapping the two sample blocks (with their fractions) changes only summation orders."""
    from slimdqn.networks.iiqn import iIQN

    rng = np.random.default_rng(22)
    K, N, B = 5, 32, 64
    batch = _atari_batch(rng, B)
    taus = rng.random((K, 3, N, B)).astype(np.float32) * 0.98 + 0.01
    perm = np.r_[32:64, 0:32]
    swapped = Batch(*(np.ascontiguousarray(x[perm]) for x in batch))
    out = []
    for bt, tt in ((batch, taus), (swapped, np.ascontiguousarray(taus[..., perm]))):
        agent = iIQN(6, (84, 84, 4), 6, K, [32, 64, 64, 512], "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
        out.append((agent._learn(bt, taus=tt).cpu().numpy().copy(), agent._flat(agent._mu)))
        del agent
    la, lb = out[0][0], out[1][0]
    assert (np.abs(la - lb) <= 1e-6 * np.abs(la)).all(), (la, lb)
    for leaf in out[0][1]:
        ga, gb = out[0][1][leaf].reshape(K, -1), out[1][1][leaf].reshape(K, -1)
        scale = np.abs(ga).max(1)[:, None]
        assert (np.abs(ga - gb) <= 1e-5 * scale + 1e-12).all(), (leaf, np.abs(ga - gb).max(), scale.max())


@pytest.mark.parametrize("n", [64, 200])
def test_iqn_q_values_many_states(n):
    from oracle import iqn_ref as I
    from oracle import make_golden as G
    from oracle import qnet_ref as Q

    obs, A, feats, K = SMALL
    N = 8
    p, pt, batch, _ = _small_inputs(N, n, 300 + n)
    agent = _agent(obs, A, feats, K, N, G.FP_HYPER)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    tau = np.random.default_rng(n).random((N, n)).astype(np.float32)
    for which, params, arena in ((0, p, agent.params), (1, pt, agent.target_params)):
        q = agent.q_values(arena, batch[0], 1, taus=tau).cpu().numpy()
        ph = Q.head(params, 1)
        want = I.quantile_values(ph, I.trunk(ph, batch[0]), tau).mean(0)
        assert q.shape == (n, A)
        assert np.abs(q - want).max() <= 2e-6 * max(1.0, np.abs(want).max())
    agent._iqn_q(0, 1, batch[0], taus=tau, want_action=True)
    acts = agent._action_out[:n].cpu().numpy()
    q = agent.q_values(agent.params, batch[0], 1, taus=tau).cpu().numpy()
    assert np.array_equal(acts, q.argmax(1))


def test_iqn_batch_trainer_entry_point(tmp_path):
    from experiments.atari.iiqn import run

    argv = ["-en", "t", "-s", "2", "-ne", "1", "-ntspe", "120", "-nis", "80", "-rbc", "200", "-nn", "2", "-nq", "8", "-at", "cnn",
            "-tuf", "20", "-tsf", "5", "-f", "32", "64", "64", "256", "-horizon", "30", "-bs", "64"]
    p, agent = run(argv, save_root=str(tmp_path))
    logs = [r for r in p["wandb"].records if "loss" in r]
    assert logs and all(np.isfinite(r["loss"]) for r in logs)
    assert int(agent._count[0].item()) >= 1


def test_iqn_batch_refusals():
    import torch

    from oracle import make_golden as G
    from slimdqn import _hip

    obs, A, feats, K = SMALL
    N, B = 4, 64
    p, pt, batch, taus = _small_inputs(N, B, 7)
    agent = _agent(obs, A, feats, K, N, G.FP_HYPER)
    agent._learn(Batch(*batch), taus=taus)
    buf = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    ptr = _hip.ptr(buf)
    with pytest.raises(_hip.HipExtensionError, match="batch 257"):
        _hip.check(_hip.lib().idqn_iqn_learn_on_batch(agent._handle, ptr, ptr, ptr, ptr, ptr, ptr, 257, 0, _hip.current_stream()),
                   "idqn_iqn_learn_on_batch")
    with pytest.raises(_hip.HipExtensionError, match="max_batch"):
        _hip.check(_hip.lib().idqn_iqn_q_values(agent._handle, 0, 0, ptr, agent._handle_batch + 1, ptr, ptr, None,
                                                _hip.current_stream()), "idqn_iqn_q_values")
