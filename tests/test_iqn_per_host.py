"""Host-side checks of i-IQN with prioritized replay (extension, parity unpinned: the reference has no quantile code).

* the replay-sourced i-IQN entries are declared in the header, exported by the built library and bound in ``_hip``;
* ``weighted_iqn_loss`` below -- the checker ``tests/test_gpu_iqn_per.py`` holds the device path to -- restates the
  importance-weighted quantile Huber loss through torch autograd on ``oracle.torch_ref.forward_head`` /
  ``iqn_quantile_values``: ``L = (1 / Bdiv) sum_b w_b l_b`` with ``l_b = (1 / N') sum_ij rho_ij``, and the priority signal
  ``td_abs_b = (1 / (N' N)) sum_ij |delta_ij|``.  With all weights 1 it must be ``oracle.iqn_ref.loss_and_grads`` (fp64,
  < 1e-9 relative: the bar ``test_oracle_fp.py`` holds the two oracles to), and its |delta| mean must be the one computed
  from the oracle's ``aux["target"]`` and ``aux["z_a"]``.  No GPU needed.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("idqn_iqn_learn_on_replay", "idqn_iqn_learn_on_replay_dev")


def weighted_iqn_loss(p_online, p_target, batch, taus, gamma_n, weights=None, bdiv=None, kappa=1.0):
    """One head, fp64.  Returns (loss, grads {leaf: array}, per_sample [B], td_abs [B])."""
    import torch

    from oracle import torch_ref as T

    dtype = torch.float64
    state, action, reward, next_state, terminal = batch
    tau_on, tau_sel, tau_tg = taus
    bsz = state.shape[0]
    w = torch.ones(bsz, dtype=dtype) if weights is None else T._t(weights, dtype)
    po = {n: T._t(a, dtype).requires_grad_(True) for n, a in p_online.items()}
    pt = {n: T._t(a, dtype) for n, a in p_target.items()}
    conv = lambda p: {n: a for n, a in p.items() if n.startswith("Conv_")}  # noqa: E731
    ar = torch.arange(bsz)
    z = T.iqn_quantile_values(po, T.forward_head(conv(po), torch.as_tensor(state), "cnn", dtype), tau_on, dtype)
    with torch.no_grad():
        psi_t = T.forward_head(conv(pt), torch.as_tensor(next_state), "cnn", dtype)
        a_star = T.iqn_quantile_values(pt, psi_t, tau_sel, dtype).mean(0).argmax(1)
        z_t = T.iqn_quantile_values(pt, psi_t, tau_tg, dtype)[:, ar, a_star]
        tgt = T._t(reward, dtype)[None] + (1 - T._t(terminal.astype(np.int64), dtype))[None] * gamma_n * z_t
    z_a = z[:, ar, torch.as_tensor(action.astype(np.int64))]
    delta = tgt[:, None, :] - z_a[None, :, :]  # [N', N, B]
    hub = torch.where(delta.abs() <= kappa, 0.5 * delta**2, kappa * (delta.abs() - 0.5 * kappa))
    wgt = (torch.as_tensor(tau_on).to(dtype)[None] - (delta.detach() < 0).to(dtype)).abs()
    per_sample = (wgt * hub / kappa).sum(1).mean(0)  # sum over the online fractions, mean over the target ones
    loss = (w * per_sample).sum() / float(bdiv or bsz)
    loss.backward()
    td_abs = delta.detach().abs().mean((0, 1))
    return (float(loss.detach()), {n: t.grad.numpy() for n, t in po.items()}, per_sample.detach().numpy(), td_abs.numpy())


def _small_case():
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    obs, A, feats, K, B, N = (20, 20, 4), 5, [32, 32, 32, 128], 2, 8, 4
    p, pt = I.init_params(0, obs, A, feats, K), I.init_params(1, obs, A, feats, K)
    batch = Q.synthetic_batch(2, B, obs, A, "cnn")
    batch[4][0] = True
    return K, B, p, pt, batch, I.synthetic_taus(3, K, N, B)


def test_replay_entries_are_declared_exported_and_bound():
    import subprocess

    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
    assert len(_hip.SYMBOLS["idqn_iqn_learn_on_replay"][1]) == 11
    assert lib.idqn_abi_version() == 4  # entries added only


def test_unit_weights_are_the_oracle():
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    K, B, p, pt, batch, taus = _small_case()
    for k in range(K):
        want, g, aux = I.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, tuple(taus[k]), 0.99)
        for weights in (None, np.ones(B, np.float32)):
            loss, grads, per_sample, td_abs = weighted_iqn_loss(Q.head(p, k), Q.head(pt, k), batch, tuple(taus[k]), 0.99, weights)
            assert abs(loss - want) <= 1e-9 * abs(want)
            for n in g:
                assert np.abs(grads[n] - g[n]).max() <= 1e-9 * (np.abs(g[n]).max() + 1e-30), n
            assert np.abs(per_sample - aux["per_sample"]).max() <= 1e-9 * np.abs(aux["per_sample"]).max()
            delta = aux["target"][:, None, :] - aux["z_a"][None, :, :]
            assert np.abs(td_abs - np.abs(delta).mean((0, 1))).max() <= 1e-9 * np.abs(delta).max()


def test_weights_scale_the_per_sample_terms():
    """L = (1 / Bdiv) sum_b w_b l_b: linear in the weights, so the gradient under weights w is the w-weighted sum of the
    gradients of the single-sample losses -- checked against one-hot weights; td_abs does not depend on the weights."""
    from oracle import qnet_ref as Q

    K, B, p, pt, batch, taus = _small_case()
    w = np.random.default_rng(4).uniform(0.05, 1.0, B).astype(np.float32)
    args = (Q.head(p, 0), Q.head(pt, 0), batch, tuple(taus[0]), 0.99)
    loss, grads, per_sample, td_abs = weighted_iqn_loss(*args, w)
    _, _, per_sample_1, td_abs_1 = weighted_iqn_loss(*args, None)
    assert np.array_equal(per_sample, per_sample_1) and np.array_equal(td_abs, td_abs_1)
    assert abs(loss - float((w.astype(np.float64) * per_sample).sum() / B)) <= 1e-12 * abs(loss)
    acc = {n: np.zeros_like(g) for n, g in grads.items()}
    for b in range(B):
        onehot = np.zeros(B)
        onehot[b] = 1.0
        _, g_b, _, _ = weighted_iqn_loss(*args, onehot)
        for n in acc:
            acc[n] += float(w[b]) * g_b[n]
    for n in grads:
        assert np.abs(grads[n] - acc[n]).max() <= 1e-9 * (np.abs(grads[n]).max() + 1e-30), n
    # a sharded divisor only rescales
    loss2, grads2, _, _ = weighted_iqn_loss(*args, w, bdiv=2 * B)
    assert abs(loss2 - loss / 2) <= 1e-12 * abs(loss)
    assert np.abs(grads2["Dense_1/kernel"] - grads["Dense_1/kernel"] / 2).max() <= 1e-12 * np.abs(grads["Dense_1/kernel"]).max()
