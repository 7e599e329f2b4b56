"""GPU parity of the HIP gradient step (through the C ABI) against the oracle and the committed goldens.

Bars (north_star): per-head TD loss within 1e-5 of the fp64 oracle; gradients / parameters to fp32
accumulation accuracy.  fp goldens are NOT reference-captured (oracle/__init__.py: parity unpinned).
"""
import json
import os

import numpy as np
import pytest

import cnn_stages as S
from cnn_stages import relerr as _relerr, unpack_act as _unpack_act, unpack_planes as _unpack_planes  # noqa: F401  (test_gpu_configs.py imports them from here)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOSS_ATOL = 1e-5  # north_star: fp32 loss within 1e-5


def _case(name):
    from oracle import make_golden as G

    arch, obs, A, feats, K, B, steps = G.FP_CASES[name]
    p, pt, batches = G.fp_case_inputs(name)
    rec = json.load(open(os.path.join(GOLDEN, f"fp_path_{name}.json")))
    return arch, obs, A, feats, K, B, steps, p, pt, batches, rec


def _agent(name):
    from collections import namedtuple

    from slimdqn.networks.idqn import iDQN

    arch, obs, A, feats, K, B, steps, p, pt, batches, rec = _case(name)
    h = rec["hyper"]
    agent = iDQN(0, obs, A, K, feats, arch, h["lr"], h["gamma"], h["n"], 1, 10**9, 10**9, adam_eps=h["eps"])
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    bs = [Batch(s, a, r, s2, t) for (s, a, r, s2, t) in batches]
    return agent, bs, rec, (arch, obs, A, feats, K, B, steps, p, pt, batches)


@pytest.fixture(params=["bf16x3", "f32"])
def conv_mode(request, monkeypatch):
    """Conv arithmetic of the agents a test creates: the plane kernels (csrc/convp.h: f32-accurate products on the bf16
    matrix cores, the default) or the f32 MFMA kernels; read by idqn_create from IDQN_CONV."""
    monkeypatch.setenv("IDQN_CONV", request.param)
    return request.param


@pytest.mark.parametrize("name", ["cnn_small", "cnn_atari_k5"])
def test_cnn_every_stage_against_oracle(name, conv_mode):
    """Forward activations, Q-values, every backward intermediate and every leaf gradient, stage by stage
    (tests/cnn_stages.py does the reading and comparing)."""
    import torch

    from slimdqn import _hip

    agent, bs, rec, (arch, obs, A, feats, K, B, steps, p, pt, batches) = _agent(name)
    losses = agent._learn(bs[0], flags=_hip.F_GRADS_ONLY).cpu().numpy()
    torch.cuda.synchronize()
    g_hat = rec["hyper"]["gamma"] ** rec["hyper"]["n"]
    oracle = S.oracle_heads(p, pt, batches[0], K, g_hat)
    for k in range(K):
        assert abs(losses[k] - oracle[k][0]) <= LOSS_ATOL, (k, losses[k], oracle[k][0])
    errs = S.stage_errors(agent, p, pt, batches[0], obs, feats, A, K, B, g_hat, conv_mode, oracle=oracle)
    S.print_stage_errors(errs)
    bad = {n_: e for n_, e in errs.items() if not e < 2e-5}
    assert not bad, bad


@pytest.mark.parametrize("name", ["cnn_small", "cnn_atari_k5", "cnn_atari_a18_b64", "fc_lunar_k3"])
def test_full_steps_against_goldens(name, conv_mode):
    """Fused path (weight gradient + Adam in one kernel): losses and post-Adam parameters of every step."""
    agent, bs, rec, _ = _agent(name)
    K = agent._K
    for s, batch in enumerate(bs):
        losses = agent._learn(batch).cpu().numpy()
        want = np.asarray(rec["steps"][s]["losses"])
        assert np.abs(losses - want).max() <= LOSS_ATOL, (s, losses, want)
        flat = agent._flat(agent._online)
        for leaf, d in rec["steps"][s]["leaves"].items():
            err = np.abs(flat[leaf].reshape(K, -1)[:, d["idx"]] - np.asarray(d["param"]))
            if s == 0:
                assert err.max() <= 3e-7, f"step {s} {leaf}: {err.max()}"
            else:
                # From the second step on a pre-activation within an fp32 ulp of zero can take the other ReLU
                # branch than in the fp64 oracle (the numpy-fp32 oracle shows the same 1.35e-6 outlier on
                # Conv_0 at step 1 of cnn_atari_k5): allow rare outliers bounded by one Adam update each.
                assert (err <= 3e-7).mean() >= 0.98 and err.max() <= 2 * rec["hyper"]["lr"] * (s + 1), \
                    f"step {s} {leaf}: {np.sort(err.ravel())[-5:]}"
    assert agent._count.cpu().numpy().tolist() == [len(bs)] * K
    np.testing.assert_allclose(agent.cumulated_losses, np.sum([r["losses"] for r in rec["steps"]], axis=0), atol=3e-5)


@pytest.mark.parametrize("name", ["cnn_small", "cnn_atari_k5", "fc_lunar_k3"])
def test_two_phase_path_gradients_and_adam(name):
    """Data-parallel split: gradients only (what gets all-reduced), then idqn_apply_adam."""
    from slimdqn import _hip

    agent, bs, rec, _ = _agent(name)
    K = agent._K
    step = rec["steps"][0]
    losses = agent._learn(bs[0], flags=_hip.F_GRADS_ONLY).cpu().numpy()
    assert np.abs(losses - np.asarray(step["losses"])).max() <= LOSS_ATOL
    G = agent._flat_grad()
    for leaf, d in step["leaves"].items():
        flat = G[leaf].reshape(K, -1)
        scale = np.asarray(d["grad_absmax"])[:, None]
        assert (np.abs(flat[:, d["idx"]] - np.asarray(d["grad"])) <= 2e-5 * scale + 1e-12).all(), leaf
        np.testing.assert_allclose(np.sqrt((flat.astype(np.float64) ** 2).sum(1)), d["grad_l2"], rtol=2e-5, err_msg=leaf)
    assert agent._count.cpu().numpy().tolist() == [0] * K  # nothing applied yet
    agent._apply_adam()
    flat = agent._flat(agent._online)
    for leaf, d in step["leaves"].items():
        np.testing.assert_allclose(flat[leaf].reshape(K, -1)[:, d["idx"]], np.asarray(d["param"]), rtol=0, atol=3e-7)
    assert agent._count.cpu().numpy().tolist() == [1] * K


def test_q_values_and_formula_known_answers():
    """tests/test_idqn.py:44-84 restated on the HIP path: target = r + (1-term) * gamma * max Q_target(s'),
    loss = (target - Q(s)[a])^2 for a single sample; best_action = argmax of the head drawn from the key."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn import prng

    agent, bs, rec, (arch, obs, A, feats, K, B, steps, p, pt, batches) = _agent("cnn_small")
    s, a, r, s2, t = batches[0]
    qv = agent.q_values(agent.params, s[:7], 1).cpu().numpy()
    np.testing.assert_allclose(qv, Q.forward(Q.head(p, 1), s[:7], arch), atol=2e-6)
    qt = agent.q_values(agent.target_params, s2[:5], 0).cpu().numpy()
    np.testing.assert_allclose(qt, Q.forward(Q.head(pt, 0), s2[:5], arch), atol=2e-6)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    for term in (False, True):
        one = Batch(s[:1], a[:1], r[:1], s2[:1], np.array([term]))
        losses = agent._learn(one, flags=1).cpu().numpy()  # grads only: parameters stay put
        for k in range(K):
            q_next = Q.forward(Q.head(pt, k), s2[:1], arch)
            target = r[0] + (1 - int(term)) * 0.99 * q_next.max()
            pred = Q.forward(Q.head(p, k), s[:1], arch)[0, a[0]]
            assert abs(losses[k] - (target - pred) ** 2) <= LOSS_ATOL
    key = prng.PRNGKey(123)
    head = prng.randint(key, 0, K)
    best = int(agent.best_action(agent.params, s[0], key).item())
    assert best == int(np.argmax(Q.forward(Q.head(p, head), s[:1], arch)[0]))
    # ties: with a zero output layer every action has the same value and jnp.argmax returns the first
    flat = {n: v.copy() for n, v in p.items()}
    last = max(int(n.split("/")[0].split("_")[1]) for n in flat if n.startswith("Dense_"))
    flat[f"Dense_{last}/kernel"][:] = 0.0
    flat[f"Dense_{last}/bias"][:] = 0.25
    agent._load_flat(agent._online, flat)
    assert int(agent.best_action(agent.params, s[0], key).item()) == 0


def test_shift_sync_and_log_semantics():
    """idqn.py:74-94: T-step = copy then shift, D-step = sync, T-step skips the sync, logs normalised by T/utd."""
    from oracle import qnet_ref as Q
    from slimdqn.networks.idqn import iDQN

    agent = iDQN(7, 8, 4, 4, [16, 16], "fc", 1e-3, 0.99, 1, 1, target_update_frequency=6, target_sync_frequency=2)
    p0 = agent._flat(agent._online)
    t0 = agent._flat(agent._target)
    for n in p0:  # make heads and target distinguishable
        p0[n] = p0[n] + np.arange(4, dtype=np.float32).reshape((4,) + (1,) * (p0[n].ndim - 1))
        t0[n] = t0[n] - 5
    agent._load_flat(agent._online, p0)
    agent._load_flat(agent._target, t0)
    agent.cumulated_losses = np.array([6.0, 12.0, 18.0, 24.0])
    updated, logs = agent.update_target_params(2)  # D-step
    assert not updated and logs == {}
    want_t = Q.sync_target_params(p0, t0)
    got_t = agent._flat(agent._target)
    for n in p0:
        np.testing.assert_array_equal(got_t[n], want_t[n])
        np.testing.assert_array_equal(agent._flat(agent._online)[n], p0[n])
    updated, logs = agent.update_target_params(6)  # T-step (also a multiple of D: sync must be skipped)
    assert updated
    assert logs["loss"] == pytest.approx(15.0 / 6) and logs["networks/2_loss"] == pytest.approx(3.0)
    np.testing.assert_array_equal(agent.cumulated_losses, np.zeros(4))
    got_p, got_t = agent._flat(agent._online), agent._flat(agent._target)
    want_p = Q.shift_params(p0)
    for n in p0:
        np.testing.assert_array_equal(got_t[n], p0[n])  # target <- params BEFORE the shift
        np.testing.assert_array_equal(got_p[n], want_p[n])
    updated, _ = agent.update_target_params(3)
    assert not updated


def test_dqn_is_the_k1_case():
    from collections import namedtuple

    from oracle import make_golden as G
    from oracle import qnet_ref as Q
    from slimdqn.networks.dqn import DQN

    arch, obs, A, feats, K, B, steps = G.FP_CASES["fc_lunar_k3"]
    p, pt, batches = G.fp_case_inputs("fc_lunar_k3")
    agent = DQN(0, obs, A, feats, arch, 6.25e-5, 0.99, 1, 1, 200, adam_eps=1.5e-4)
    p1 = {n: a[:1] for n, a in p.items()}
    pt1 = {n: a[:1] for n, a in pt.items()}
    agent._load_flat(agent._online, p1)
    agent._load_flat(agent._target, pt1)
    assert agent.params["params"]["Dense_0"]["kernel"].shape == (8, 100)  # no leading head axis (dqn.py:29)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    _, _, loss = agent.learn_on_batch(agent.params, agent.target_params, agent.optimizer_state, Batch(*batches[0]))
    want, _, _ = Q.loss_and_grads(Q.head(p, 0), Q.head(pt, 0), batches[0], arch, 0.99)
    assert abs(float(loss.item()) - want) <= LOSS_ATOL
    updated, logs = agent.update_target_params(200)
    assert updated and logs["loss"] == pytest.approx(want / 200, rel=1e-5)
    for n, v in agent._flat(agent._target).items():
        np.testing.assert_array_equal(v, agent._flat(agent._online)[n])


@pytest.mark.parametrize("env_name", ["lunar_lander", "atari"])
def test_entry_points_train_end_to_end(env_name, tmp_path):
    """experiments/{lunar_lander,atari}/idqn.py counterpart: collect -> update_online -> update_target on the HIP path."""
    import pickle

    if env_name == "lunar_lander":
        from experiments.lunar_lander.idqn import run

        argv = ["-en", "t", "-s", "1", "-ne", "1", "-ntspe", "120", "-nis", "40", "-rbc", "200", "-nn", "3",
                "-tuf", "20", "-tsf", "5", "-f", "32", "32", "-horizon", "30"]
    else:
        from experiments.atari.idqn import run

        argv = ["-en", "t", "-s", "1", "-ne", "1", "-ntspe", "80", "-nis", "40", "-rbc", "100", "-nn", "2", "-at", "cnn",
                "-tuf", "20", "-tsf", "5", "-f", "32", "64", "64", "128", "-horizon", "30", "-bs", "32"]
    p, agent = run(argv, save_root=str(tmp_path))
    logs = [r for r in p["wandb"].records if "loss" in r]
    assert logs and all(np.isfinite(r["loss"]) and f"networks/{agent.n_networks - 1}_loss" in r for r in logs)
    assert int(agent._count[0].item()) >= 40
    model = pickle.load(open(os.path.join(p["save_path"], "models", "1"), "rb"))
    assert set(model) == {"params"} and set(model["params"]) == {"params"}  # {"params": flax variables dict}, idqn.py:133
    assert all(np.isfinite(v).all() for m in model["params"]["params"].values() for v in m.values())


@pytest.mark.parametrize("env_name", ["lunar_lander", "atari"])
def test_dqn_entry_points_run_as_scripts(env_name, tmp_path):
    """What the reference's own integration tests do (tests/test_lunar_lander.py, tests/test_atari.py:15-59): run
    `python experiments/<env>/dqn.py` with tiny settings in a subprocess and require exit code 0."""
    import subprocess
    import sys

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "i-dqn_amd")
    argv = ["-en", "_test_script", "-s", "1", "-dw", "-rbc", "100", "-bs", "32", "-n", "1", "-gamma", "0.99", "-lr", "1e-4",
            "-horizon", "10", "-ne", "1", "-ntspe", "60", "-utd", "1", "-nis", "40", "-ee", "0.01", "-ed", "10",
            "-tuf", "10"]
    argv += ["-f", "32", "64", "64", "128", "-at", "cnn"] if env_name == "atari" else ["-f", "25", "25", "-at", "fc"]
    code = ("import sys; sys.path.insert(0, %r); from experiments.%s.dqn import run; run(%r, save_root=%r)"
            % (root, env_name, argv, str(tmp_path)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert os.path.exists(os.path.join(str(tmp_path), "_test_script", "dqn", "models", "1"))


@pytest.mark.parametrize("arch,obs,feats,A,K,B", [
    ("cnn", (20, 20, 4), [32, 32, 32, 128], 5, 2, 20),     # ragged: one partly filled 32-sample block
    ("cnn", (20, 20, 4), [32, 64, 32, 256], 3, 3, 50),     # ragged second block, mixed channel widths, J = 256
    ("cnn", (36, 28, 4), [64, 32, 64, 128], 18, 1, 33),    # non-square frames, 18 actions, one sample in block 2
    ("cnn", (20, 20, 4), [32, 32, 32, 128], 4, 2, 256),    # eight sample blocks (BASELINE config 4's global batch)
    ("fc", 8, [100, 100], 4, 3, 7),
    ("fc", (6, 1), [50], 2, 9, 64),
    ("fc", 8, [200, 200], 4, 2, 40),       # the MFMA kernel with weight operands from global memory, two sample blocks
    ("fc", 9, [255, 131], 5, 2, 70),       # the same with odd widths (k padding, clamped edge tiles), three blocks
    ("fc", 8, [200, 200, 200], 4, 1, 32),  # three hidden layers of that size still fit (activations packed per layer)
    ("fc", 12, [512, 300, 64], 6, 2, 33),  # 8-sample blocks, four layers, widest layer the LDS kernels take
    ("fc", 10, [700, 33], 3, 2, 12),       # wider than that: the generic kernel (any width), acting through k_fc_q
    ("fc", 5, [7, 9], 3, 2, 32),           # odd widths
])
def test_ragged_batches_and_shapes_against_oracle(arch, obs, feats, A, K, B, conv_mode):
    """Edge cases of the batch / shape handling: live oracle comparison of losses, gradients and one Adam step."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    p = Q.init_params(3, arch, obs, A, feats, K)
    pt = Q.init_params(4, arch, obs, A, feats, K)
    rng = np.random.default_rng(5)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = list(Q.synthetic_batch(6, B, obs, A, arch))
    batch[4][B // 2] = True
    agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.97, 3, 1, 10**9, 10**9, adam_eps=1e-6)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    G = agent._flat_grad()
    gamma_n = 0.97 ** 3
    for k in range(K):
        loss, grads, _ = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), tuple(batch), arch, gamma_n)
        assert abs(losses[k] - loss) <= LOSS_ATOL, (k, losses[k], loss)
        for leaf, g in grads.items():
            assert _relerr(G[leaf][k], g) < 2e-5, (k, leaf, _relerr(G[leaf][k], g))
    agent._apply_adam()
    zeros = {n: np.zeros(v.shape, np.float64) for n, v in p.items()}
    want, _, _, _, _ = Q.learn_on_batch({n: v.astype(np.float64) for n, v in p.items()}, pt, zeros, zeros,
                                        np.zeros(K, np.int64), tuple(batch), arch, gamma_n, 1e-3, 1e-6)
    got = agent._flat(agent._online)
    for leaf in want:
        # first Adam step moves every element by ~lr * g / (|g| + eps): elements with |g| ~ eps amplify the fp32
        # gradient error, so compare at 2 % of one update
        assert np.abs(got[leaf] - want[leaf]).max() <= 2e-5, leaf


@pytest.mark.parametrize("feats,K,B", [
    ([32, 64, 64, 256], 2, 100),   # four blocks, the last one ragged: separate data gradient + factored bf16x3 update
    ([32, 64, 64, 512], 2, 250),   # eight blocks, the last one ragged: data gradient as the tiled GEMM + finalize
    ([32, 32, 64, 512], 1, 512),   # sixteen blocks = two groups of eight
])
def test_many_block_step_against_oracle(feats, K, B, conv_mode):
    """The route single-device steps of three or more 32-sample blocks take (block-inner Dense_0 forward, data gradient as its own
    launch -- the tiled GEMM for groups of eight blocks --, factors split once, bf16x3 update with Adam fused): ONE full
    `learn_on_batch` against the fp64 oracle, ragged last blocks included."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn.networks.idqn import iDQN

    arch, obs, A = "cnn", (20, 20, 4), 5
    p = Q.init_params(13, arch, obs, A, feats, K)
    pt = Q.init_params(14, arch, obs, A, feats, K)
    rng = np.random.default_rng(15)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = list(Q.synthetic_batch(16, B, obs, A, arch))
    batch[4][B // 3] = True
    agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.97, 3, 1, 10**9, 10**9, adam_eps=1e-6)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    losses = agent._learn(Batch(*batch)).cpu().numpy()
    gamma_n = 0.97 ** 3
    zeros = {n: np.zeros(v.shape, np.float64) for n, v in p.items()}
    want, _, _, _, want_losses = Q.learn_on_batch({n: v.astype(np.float64) for n, v in p.items()}, pt, zeros, zeros,
                                                  np.zeros(K, np.int64), tuple(batch), arch, gamma_n, 1e-3, 1e-6)
    assert np.abs(losses - np.asarray(want_losses)).max() <= LOSS_ATOL, (losses, want_losses)
    got = agent._flat(agent._online)
    for leaf in want:
        err = np.abs(got[leaf] - want[leaf])
        # (first Adam step: every element moves by ~lr; an element whose gradient is ~eps amplifies the fp32 gradient error)
        assert err.max() <= 2e-5 and (err <= 3e-7).mean() >= 0.98, (leaf, err.max(), (err <= 3e-7).mean())


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_nature_shape_with_fewer_heads_against_oracle(K):
    """The Nature-CNN step at K = 1 (plain DQN, networks/dqn.py:60-73) .. 4 heads: the launch plans (items of one to four tiles per wave,
    the data-gradient | weight-gradient pairs built for those tile counts) differ from the K = 5 goldens' -- losses and every leaf
    gradient against the live oracle."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    arch, obs, feats, A, B = "cnn", (84, 84, 4), [32, 64, 64, 512], 6, 32
    p = Q.init_params(23, arch, obs, A, feats, K)
    pt = Q.init_params(24, arch, obs, A, feats, K)
    batch = list(Q.synthetic_batch(26, B, obs, A, arch))
    batch[4][5] = True
    agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-6)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    G = agent._flat_grad()
    for k in range(K):
        loss, grads, _ = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), tuple(batch), arch, 0.99)
        assert abs(losses[k] - loss) <= LOSS_ATOL, (k, losses[k], loss)
        for leaf, g in grads.items():
            assert _relerr(G[leaf][k], g) < 2e-5, (k, leaf, _relerr(G[leaf][k], g))


def test_dqn_cnn_and_many_heads():
    """K = 1 without the head axis on the cnn, and K = 12 (more nets than the Atari config) in one launch set."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn.networks.dqn import DQN
    from slimdqn.networks.idqn import iDQN

    arch, obs, feats, A, B = "cnn", (20, 20, 4), [32, 32, 32, 128], 4, 32
    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    batch = Q.synthetic_batch(1, B, obs, A, arch)
    for K, cls in ((1, DQN), (12, iDQN)):
        p = Q.init_params(7, arch, obs, A, feats, K)
        pt = Q.init_params(8, arch, obs, A, feats, K)
        if K == 1:
            agent = cls(0, obs, A, feats, arch, 1e-4, 0.99, 1, 1, 200, adam_eps=1e-8)
            assert agent.params["params"]["Conv_0"]["kernel"].shape == (8, 8, 4, 32)
        else:
            agent = cls(0, obs, A, K, feats, arch, 1e-4, 0.99, 1, 1, 200, 10, adam_eps=1e-8)
        agent._load_flat(agent._online, p)
        agent._load_flat(agent._target, pt)
        losses = agent._learn(Batch(*batch)).cpu().numpy()
        want = [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, arch, 0.99)[0] for k in range(K)]
        assert np.abs(losses - np.asarray(want)).max() <= LOSS_ATOL


@pytest.fixture(scope="module")
def rccl_single_rank():
    import torch
    import torch.distributed as dist

    import socket

    with socket.socket() as sock:  # a free port: a fixed one collides when two suites share a box
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def _dp_steps_match_golden(name, **kw):
    from slimdqn.networks.parallel import data_parallel_step

    agent, bs, rec, _ = _agent(name)
    K = agent._K
    for s, batch in enumerate(bs):
        losses = data_parallel_step(agent, batch, len(batch.action), **kw).cpu().numpy()
        assert np.abs(losses - np.asarray(rec["steps"][s]["losses"])).max() <= LOSS_ATOL, (kw, s)
    flat = agent._flat(agent._online)
    last = rec["steps"][len(bs) - 1]["leaves"]
    for leaf, d in last.items():
        err = np.abs(flat[leaf].reshape(K, -1)[:, d["idx"]] - np.asarray(d["param"]))
        if len(bs) == 1:
            assert err.max() <= 3e-7, (kw, leaf)
        assert (err <= 3e-7).mean() >= 0.98 and err.max() <= 2 * rec["hyper"]["lr"] * len(bs), (kw, leaf)
    assert agent._count.cpu().numpy().tolist() == [len(bs)] * K
    cum = agent._cum.cpu().numpy()
    want = np.sum([st["losses"] for st in rec["steps"][: len(bs)]], axis=0)
    assert np.abs(cum - want).max() <= LOSS_ATOL * len(bs)


@pytest.mark.parametrize("overlap", [True, False])
def test_allreduce_data_parallel_step_single_rank(rccl_single_rank, overlap):
    """The all-reduce variants of the RCCL path end to end on one rank (world_size 1): two-call backward with the
    async all-reduce of the Dense_0 region, all-reduce of the small-leaf region, two-phase Adam == the golden steps."""
    _dp_steps_match_golden("cnn_atari_k5", mode="allreduce", overlap=overlap)


@pytest.mark.parametrize("name", ["cnn_small", "cnn_atari_k5", "cnn_atari_a18_b64"])
def test_factored_data_parallel_step_single_rank(rccl_single_rank, name):
    """The factored step (all-gather of the Dense_0 factors a3 / dh through RCCL, fused weight-gradient + Adam over
    the gathered blocks, small leaves all-reduced) on one rank == the golden steps; b64 covers two blocks per rank."""
    _dp_steps_match_golden(name, mode="factored")


def test_factored_step_sums_blocks_of_several_ranks():
    """What N ranks compute, on one GPU: split a 64-sample global batch into two 32-sample shards, run the first
    half of the step on each (mean divisor 64), concatenate the exported factors the way all_gather lays them out
    ([rank][head][block]) and finish from them -- the update must equal the single-device step on the 64 samples."""
    import factored_shapes as FS
    from slimdqn import _hip

    agent, bs, rec, _ = _agent("cnn_atari_a18_b64")
    K = agent._K
    g = FS.emulate_ranks(agent, bs[0], 2)
    assert (g.nb_total, g.nb_inner) == (2, 1)
    _hip.check(_hip.lib().idqn_finish_step_factored(*g.finish_args, _hip.FACTORED_DENSE0 | _hip.FACTORED_REST, _hip.current_stream()),
               "finish")
    st = rec["steps"][0]
    assert np.abs(agent._losses.cpu().numpy() - np.asarray(st["losses"])).max() <= LOSS_ATOL
    flat = agent._flat(agent._online)
    for leaf, d in st["leaves"].items():
        err = np.abs(flat[leaf].reshape(K, -1)[:, d["idx"]] - np.asarray(d["param"]))
        assert err.max() <= 3e-7, (leaf, err.max())
    assert agent._count.cpu().numpy().tolist() == [1] * K


def test_factor_view_is_the_exported_factors():
    """idqn_dense0_factors (zero-copy: dL/dh directly in front of the online nets' a3 inside the library) shows exactly the
    floats idqn_export_dense0_factors copies out, for one and for two sample blocks per rank."""
    import ctypes as C

    import torch

    from slimdqn import _hip

    lib = _hip.lib()
    for name in ("cnn_atari_k5", "cnn_atari_a18_b64"):
        agent, bs, _, _ = _agent(name)
        K = agent._K
        F, J = next(shape for n, _, shape in agent._leaves if n == "Dense_0/kernel")
        nb = -(-len(np.asarray(bs[0].action)) // 32)
        n_a3, n_dh = K * nb * F * 32, K * nb * J * 32
        agent._learn(bs[0], flags=_hip.F_STOP_BEFORE_DENSE0_WGRAD)
        a3 = torch.empty(n_a3, dtype=torch.float32, device="cuda")
        dh = torch.empty(n_dh, dtype=torch.float32, device="cuda")
        _hip.check(lib.idqn_export_dense0_factors(agent._handle, _hip.ptr(a3), _hip.ptr(dh), _hip.current_stream()), "export")
        p, c_dh, c_a3 = C.c_void_p(), C.c_int64(), C.c_int64()
        _hip.check(lib.idqn_dense0_factors(agent._handle, C.byref(p), C.byref(c_dh), C.byref(c_a3)), "idqn_dense0_factors")
        assert (c_dh.value, c_a3.value) == (n_dh, n_a3)
        view = _hip.device_view(p.value, n_dh + n_a3)
        torch.cuda.synchronize()
        assert torch.equal(view[:n_dh], dh) and torch.equal(view[n_dh:], a3)
        assert float(dh.abs().sum()) > 0 and float(a3.abs().sum()) > 0
        _hip.check(lib.idqn_backward_rest(agent._handle, _hip.current_stream()), "rest")  # leave no step half done
        torch.cuda.synchronize()


def test_head_window_agent_equals_rows_of_the_full_agent():
    """Head-parallel mode: an agent holding heads [first, first + count) of a K-head i-DQN
    starts from the same parameters as those rows of the single-device agent and, fed the same minibatches, follows
    them to fp32 accumulation accuracy (the heads are independent inside a step; the split-K chunking of the kernels
    depends on the number of local heads, so sums are re-associated, not bit-identical)."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn.networks.idqn import iDQN

    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    obs, A, feats, K = (20, 20, 4), 5, [32, 32, 32, 128], 6
    args = (obs, A, K, feats, "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9)
    full = iDQN(3, *args)
    windows = [iDQN(3, *args, _local_heads=(first, 2)) for first in (0, 2, 4)]
    for step in range(3):
        batch = Batch(*Q.synthetic_batch(40 + step, 32, obs, A, "cnn"))
        want = full._learn(batch).cpu().numpy().copy()
        for w, first in zip(windows, (0, 2, 4)):
            got = w._learn(batch).cpu().numpy()
            np.testing.assert_allclose(got, want[first : first + 2], rtol=2e-6)
        if step == 0:
            for w, first in zip(windows, (0, 2, 4)):
                np.testing.assert_array_equal(w._target.cpu().numpy(), full._target[first : first + 2].cpu().numpy())
    for w, first in zip(windows, (0, 2, 4)):
        assert w.n_networks == K and w._K == 2
        err = np.abs(w._online.cpu().numpy() - full._online[first : first + 2].cpu().numpy())
        assert (err <= 1e-6).mean() >= 0.999 and err.max() <= 2 * 1e-3 * 3, (first, err.max())


def test_head_sharded_agent_on_one_rank_is_the_plain_agent(rccl_single_rank):
    """HeadShardedIDQN over RCCL with world_size 1: same steps, T-step logs, shift and sync as iDQN."""
    from collections import namedtuple

    from oracle import qnet_ref as Q
    from slimdqn.networks.head_parallel import HeadShardedIDQN
    from slimdqn.networks.idqn import iDQN
    from slimdqn import prng

    Batch = namedtuple("Batch", "state action reward next_state is_terminal")
    obs, A, feats, K = (20, 20, 4), 5, [32, 32, 32, 128], 4
    args = (obs, A, K, feats, "cnn", 1e-3, 0.99, 1, 1, 4, 2)  # T = 4, D = 2

    class OneBatch:
        def __init__(self):
            self.i = 0

        def sample(self):
            self.i += 1
            return Batch(*Q.synthetic_batch(70 + self.i, 32, obs, A, "cnn"))

    a, b, ra, rb = iDQN(9, *args), HeadShardedIDQN(9, *args), OneBatch(), OneBatch()
    for step in range(1, 10):
        a.update_online_params(step, ra)
        b.update_online_params(step, rb)
        la, lb = a.update_target_params(step), b.update_target_params(step)
        assert la[0] == lb[0] and la[1].keys() == lb[1].keys()
        for k in la[1]:
            assert la[1][k] == lb[1][k], (step, k)
    np.testing.assert_array_equal(a._online.cpu().numpy(), b._online.cpu().numpy())
    np.testing.assert_array_equal(a._target.cpu().numpy(), b._target.cpu().numpy())
    state = Q.synthetic_batch(1, 1, obs, A, "cnn")[0][0]
    key = prng.PRNGKey(4)
    assert int(a.best_action(a.params, state, key)) == int(b.best_action(b.params, state, key))
    assert b.get_model()["heads"] == (0, K, K)
