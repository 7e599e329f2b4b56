"""Probe golden of an i-IQN step on a minibatch of more than 32 samples: K = 5, N = 32, A = 6, [32, 64, 64, 512], B = 64.

Same record format as ``oracle/make_golden.py --iqn`` (``capture_iqn``), from the fp64 oracle ``oracle/iqn_ref.py``, with the
inputs built the way ``iqn_case_inputs`` builds them.  Writes ``tests/golden/fp_path_iqn_atari_k5_b64.json``; ``oracle/`` is
only imported.  Usage: ``python tools/make_iqn_batch_golden.py``.

Conditioning.  A step is compared leaf by leaf against fp64 at 3e-5 of each leaf's largest gradient entry.  That bar assumes
every ReLU of the backward pass takes the same branch in fp32 as in fp64.  With 64 samples x 32 fractions x 5 heads there are
~10^7 online pre-activations, and a few of them land within the fp32 rounding of a 7744-term sum of zero (seen: a Dense_0
pre-activation of 7e-9 and a Conv_2 pre-activation of 3e-8).  One flipped mask moves that sample's whole dL/dpsi, and with it
the conv gradients, by ~1e-3 of their scale.  So the case is made well conditioned: every sample whose online pre-activations
(Conv_0..2, Embed_0, Dense_0, all heads) come within MARGIN of zero gets a fresh state and fresh online fractions, until none
does.  The replacements are recorded in the golden (``replaced``) and ``case_inputs`` replays them.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import iqn_ref as I  # noqa: E402
from oracle import make_golden as G  # noqa: E402
from oracle import qnet_ref as Q  # noqa: E402

MARGIN = 2e-7  # ~7x the largest pre-activation seen to take the other branch in fp32

CASES = {"iqn_atari_k5_b64": ((84, 84, 4), 6, [32, 64, 64, 512], 5, 64, 32)}  # name: (obs, A, features, K, B, N)


def case_inputs(name, replaced=None):
    """Inputs of the case; `replaced` ([[round, sample], ...], default: the committed golden's list) replays the conditioning."""
    obs, A, feats, K, B, N = CASES[name]
    seed = sum(name.encode())
    p = I.init_params(seed, obs, A, feats, K)
    pt = I.init_params(seed + 1, obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(seed + 10, B, obs, A, "cnn")
    term[0] = True
    term[40] = True  # (one terminal transition in the second sample block too)
    taus = I.synthetic_taus(seed + 20, K, N, B)
    if replaced is None:
        replaced = json.load(open(os.path.join(ROOT, "tests", "golden", f"fp_path_{name}.json")))["replaced"]
    for rnd, b in replaced:
        _replace(st, taus, seed, rnd, b)
    return p, pt, (st, a, r, s2, term), taus


def _replace(st, taus, seed, rnd, b):
    g = np.random.default_rng([seed, 1000 + rnd, b])
    st[b] = g.integers(0, 256, size=st.shape[1:], dtype=np.uint8)
    taus[:, 0, :, b] = g.random(taus[:, 0, :, b].shape).astype(np.float32)


def _min_preact(p, state, tau_on):
    """Per sample: the smallest |pre-activation| of every ReLU on the online side of one head (fp64)."""
    a = state.astype(np.float64) / 255.0
    m = np.full(state.shape[0], np.inf)
    for li, (k, s) in enumerate(Q.CNN_GEOM):
        y, _ = Q.conv_fwd(a, p[f"Conv_{li}/kernel"].astype(np.float64), p[f"Conv_{li}/bias"].astype(np.float64), s)
        m = np.minimum(m, np.abs(y).reshape(y.shape[0], -1).min(1))
        a = np.maximum(y, 0)
    psi = a.reshape(a.shape[0], -1)
    e = I.cos_features(tau_on) @ p["Embed_0/kernel"].astype(np.float64) + p["Embed_0/bias"].astype(np.float64)
    m = np.minimum(m, np.abs(e).min(axis=(0, 2)))
    pre = (psi[None] * np.maximum(e, 0)) @ p["Dense_0/kernel"].astype(np.float64) + p["Dense_0/bias"].astype(np.float64)
    return np.minimum(m, np.abs(pre).min(axis=(0, 2)))


def condition(name):
    """The replacement list that leaves no online pre-activation within MARGIN of zero."""
    obs, A, feats, K, B, N = CASES[name]
    seed = sum(name.encode())
    replaced = []
    p, _, (st, *_), taus = case_inputs(name, replaced)
    for rnd in range(50):
        bad = np.zeros(B, bool)
        for k in range(K):
            bad |= _min_preact(Q.head(p, k), st, taus[k, 0]) < MARGIN
        print("round", rnd, "samples near a ReLU kink:", np.flatnonzero(bad).tolist())
        if not bad.any():
            return replaced
        for b in np.flatnonzero(bad):
            replaced.append([rnd, int(b)])
            _replace(st, taus, seed, rnd, int(b))
    raise RuntimeError("no well-conditioned inputs found")


def capture(name):
    obs, A, feats, K, B, N = CASES[name]
    replaced = condition(name)
    p, pt, batch, taus = case_inputs(name, replaced)
    hy = G.FP_HYPER
    gamma_n = hy["gamma"] ** hy["n"]
    mu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    nu = {n: np.zeros_like(a, dtype=np.float64) for n, a in p.items()}
    _, _, aux0 = I.loss_and_grads(Q.head(p, 0), Q.head(pt, 0), batch, tuple(taus[0]), gamma_n)
    p64, mu, nu, count, losses, grads = I.learn_on_batch(p, pt, mu, nu, np.zeros(K, np.int64), batch, taus, gamma_n, hy["lr"],
                                                         hy["eps"], np.float64, return_grads=True)
    rec = {"case": name, "hyper": hy, "losses": losses.tolist(), "z_online_head0": aux0["z_a"].tolist(),
           "z_target_head0": aux0["z_t"].tolist(), "a_star_head0": aux0["a_star"].tolist(),
           "q_select_head0": aux0["q_sel"].tolist(), "leaves": {},
           "replaced": replaced, "margin": MARGIN}
    for leaf in p64:
        flat_g, flat_p = grads[leaf].reshape(K, -1), p64[leaf].reshape(K, -1)
        idx = G.probe_indices(name, leaf, flat_g.shape[1])
        rec["leaves"][leaf] = {"idx": idx.tolist(), "grad": flat_g[:, idx].tolist(), "param": flat_p[:, idx].tolist(),
                               "grad_l2": np.sqrt((flat_g**2).sum(1)).tolist(), "grad_absmax": np.abs(flat_g).max(1).tolist()}
    out = os.path.join(ROOT, "tests", "golden", f"fp_path_{name}.json")
    with open(out, "w") as f:
        json.dump(rec, f)
    print("wrote", out, rec["losses"])


if __name__ == "__main__":
    for name in CASES:
        capture(name)
