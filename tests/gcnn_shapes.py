"""Shape table and oracle composition of the general-shape cnn path's tests (tests/test_gcnn_shapes_host.py on the CPU,
tests/test_gpu_gcnn_shapes.py on the device).  Not a test module.

Every row is a cnn configuration ``cnn_fast_shape()`` (csrc/qnet.hip) refuses, so its handle runs csrc/gcnn_kernels.h: one thread
per output element, index arithmetic of its own over the reference's SAME padding (architectures/dqn.py:39-53).  What can go
wrong there is geometry, so the rows are chosen by geometry: Conv_0 (8x8 / 4) pads (2, 2), (3, 4), (3, 3), (2, 3) for an extent
= 0, 1, 2, 3 mod 4, Conv_1 (4x4 / 2) pads (1, 1) on an even input and (1, 2) on an odd one, Conv_2 (3x3 / 1) always (1, 1).

Per head, in fp64: loss, every leaf gradient, the post-ReLU output of each conv (``aux["tape"]``), the gradient at each conv's
pre-activation (``aux["trace"]["d_conv{i}"]``), Q-values of both nets from ``oracle.qnet_ref.loss_and_grads(..., "cnn", gamma_n)``;
Adam from ``oracle.qnet_ref.adam_update``.  Batches are ``synthetic_batch(..., "cnn")`` with one terminal sample forced (not at
B = 1: the only sample has to reach the target net); biases are drawn as tests/test_gpu_general_shapes.py draws them.
"""
import functools

import numpy as np

GAMMA_N = 0.99
LR, EPS = 1e-3, 1e-6  # (the Adam constants of tests/test_gpu_conv_geometry.py, whose every-element bar the device test applies)
FC_MAX_WIDTH = 512    # csrc/fc_kernels.h

# name: (obs, features, A, K, B)                              Conv_0 pad class of H, W (extent mod 4) and the Conv_1 input's parity
ROWS = {
    "unit": ((1, 1, 1), [1, 1, 1], 1, 1, 1),                  # 1x1x1 frame, every width 1, A = K = B = 1, F = 1, no hidden layer
    "one_row": ((1, 5, 1), [2, 3, 2, 4], 3, 2, 4),            # a one-row frame; W = 5: class 1 (3, 4), Conv_1 input 2 (even)
    "one_col": ((7, 1, 3), [3, 2, 2, 5], 3, 1, 2),            # a one-column frame, obs_c = 3; H = 7: class 3 (2, 3), Conv_1 input 2
    "sub_kernel": ((5, 6, 2), [4, 3, 5, 6], 4, 2, 5),         # smaller than the 8x8 kernel on both axes: classes 1 and 2, inputs 2 x 2
    "h9_w14": ((9, 14, 5), [7, 5, 3, 9], 5, 3, 7),            # H class 1 / odd input 3, W class 2 / even input 4; obs_c = 5, width 7, K = 3
    "h11_w6": ((11, 6, 3), [5, 7, 4, 8, 6], 6, 2, 6),         # H class 3 / odd input 3, W class 2 / even input 2; two hidden layers
    "nature_96": ((10, 14, 4), [32, 64, 64, 96], 4, 2, 8),    # Nature widths, 4 channels, a dense width the plane path refuses; class 2 x 2
    "h13_w7": ((13, 7, 1), [1, 33, 2, 10], 2, 1, 3),          # H class 1 / even input 4, W class 3 / even input 2; conv widths 1 and 33
    "h12_w11": ((12, 11, 2), [65, 4, 3, 7], 33, 1, 33),       # H class 0 / odd input 3, W class 3 / odd input 3; width 65, A = 33, B = 33
    "no_hidden": ((8, 9, 3), [3, 4, 5], 40, 1, 34),           # H class 0 / even input 2, W class 1 / odd input 3; no hidden layer, A = 40, B = 34
    "f512": ((16, 32, 2), [4, 6, 64, 20], 5, 1, 3),           # F = 2 * 4 * 64 = 512 = dmax exactly; class 0 with even inputs 4 x 8
    "f513": ((20, 20, 1), [3, 5, 57, 16], 3, 2, 2),           # F = 3 * 3 * 57 = 513 = dmax; class 0 with odd inputs 5 x 5
    "hid512": ((6, 10, 1), [2, 3, 4, 512], 3, 1, 2),          # a hidden width of 512 behind F = 8; W = 10: class 2 / odd input 3
    "hid513": ((10, 7, 2), [2, 3, 4, 513], 2, 1, 2),          # a hidden width of 513 behind F = 8; H = 10: class 2 / odd input 3
}
# init_params draws Conv_0 of these frames so that some head's ReLUs are all dead (5 to 7 leaves with an all-zero gradient): their
# biases are made positive, abs(b) + 0.05, and the seed is chosen so that every leaf of every head has a gradient
POSITIVE_BIAS = ("unit", "one_row", "one_col")
SEEDS = {"unit": 1}  # (seed 0 leaves Conv_1's one unit dead on the one pixel)
# rows of the weighted (prioritized) step: one tiny, one pad-class row, one with more than 32 actions
WEIGHTED = ("one_row", "h9_w14", "h12_w11")
# rows of the replay-sourced step: an odd extent and obs_c != 4 (the ring's stack = obs_c)
REPLAY = ("h11_w6", "h9_w14")
N_ACT_STATES = 32


def geometry(obs, feats):
    """[(IH, IW, OH, OW, (pad lo, hi) rows, (pad lo, hi) columns)] of Conv_0..2, and the flatten width F."""
    from oracle.qnet_ref import CNN_GEOM, same_pad

    h, w = obs[:2]
    out = []
    for k, s in CNN_GEOM:
        oh, lo_h, hi_h = same_pad(h, k, s)
        ow, lo_w, hi_w = same_pad(w, k, s)
        out.append((h, w, oh, ow, (lo_h, hi_h), (lo_w, hi_w)))
        h, w = oh, ow
    return out, h * w * feats[2]


def dmax(obs, feats, A):
    """The widest row of the dense head, the flatten width included (gcnn_setup: FcNet::dmax)."""
    return max([geometry(obs, feats)[1]] + list(feats[3:]) + [A])


def case(name):
    """(obs, feats, A, K, B, online, target, batch) of a row: float32 parameters [K, ...], numpy batch."""
    return _case(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import qnet_ref as Q

    obs, feats, A, K, B = ROWS[name]
    seed = SEEDS.get(name, 0)
    p = Q.init_params(seed, "cnn", obs, A, feats, K)
    pt = Q.init_params(seed + 1, "cnn", obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            if name in POSITIVE_BIAS:
                p[n], pt[n] = np.abs(p[n]) + np.float32(0.05), np.abs(pt[n]) + np.float32(0.05)
    batch = Q.synthetic_batch(seed + 3, B, obs, A, "cnn")
    if B > 1:
        batch[4][0] = True
    for a in list(p.values()) + list(pt.values()) + list(batch):
        a.setflags(write=False)
    return obs, feats, A, K, B, p, pt, batch


@functools.lru_cache(maxsize=None)
def act_states(name):
    """32 states for the acting checks (uint8 [32, H, W, C])."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B = ROWS[name]
    s = Q.synthetic_batch(SEEDS.get(name, 0) + 9, N_ACT_STATES, obs, A, "cnn")[0]
    s.setflags(write=False)
    return s


def _head_record(loss, grads, aux, target_tape):
    return {"loss": loss, "grads": grads, "q": aux["q"], "q_next": aux["q_next"], "td": aux["td"],
            "act": [t[4] for t in aux["tape"] if t[0] == "conv"],          # [B, OH, OW, CO] after the ReLU, online net on state
            "act_next": [t[4] for t in target_tape if t[0] == "conv"],     # target net on next_state
            "dact": [aux["trace"][f"d_conv{i}"] for i in range(3)]}        # gradient at each conv's pre-activation


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per head k: dict(loss, grads {leaf: fp64}, q, q_next [B, A], td [B], act, act_next, dact: three stages each) -- fp64,
    computed once per row."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    out = []
    for k in range(K):
        loss, grads, aux = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N)
        out.append(_head_record(loss, grads, aux, Q.forward(Q.head(pt, k), batch[3], "cnn", keep=True)[1]))
    return out


@functools.lru_cache(maxsize=None)
def adam_from_zero(name):
    """{leaf: [K, ...]} fp64 parameters after one Adam step from a zero optimizer state, from the gradients of ``oracle``."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    want = oracle(name)
    return {n: np.stack([Q.adam_update(p[n][k].astype(np.float64), want[k]["grads"][n], 0.0, 0.0, 0, LR, EPS)[0] for k in range(K)])
            for n in p}


@functools.lru_cache(maxsize=None)
def f32_errors(name):
    """The float32 run of torch_ref against the fp64 oracle on the same inputs, per head: (|loss error|, {leaf: max |error| /
    max |gradient|}).  4 x the leaf's figure is the fallback bar of a leaf that misses 2e-5 on the device."""
    import torch

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = _case(name)
    out = []
    for k, want in enumerate(oracle(name)):
        loss, grads = T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N, dtype=torch.float32)
        out.append((abs(loss - want["loss"]),
                    {n: float(np.abs(grads[n] - g).max() / (np.abs(g).max() + 1e-300)) for n, g in want["grads"].items()}))
    return out


def weights(name):
    """The importance weights of the row's weighted step."""
    return np.random.default_rng(5).uniform(0.2, 1.0, ROWS[name][4]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def weighted_oracle(name):
    """Per head: (loss, grads, |td|) of the prioritized-replay extension's loss  mean_b w_b td_b^2  (fp64)."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    out = []
    for k in range(K):
        loss, grads, aux = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N, weights=weights(name))
        out.append((loss, grads, np.abs(aux["td"])))
    return out


@functools.lru_cache(maxsize=None)
def act_oracle(name):
    """fp64 Q-values [2 sets][K][32, A] of ``act_states``: online (0) and target (1) parameters."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    return [[Q.forward(Q.head(ps, k), act_states(name), "cnn") for k in range(K)] for ps in (p, pt)]


def top_two_gap(q):
    """The gap between a row's two largest Q-values (infinite for a single action: there is nothing to confuse)."""
    if q.size < 2:
        return np.inf
    top = np.sort(q)[::-1]
    return top[0] - top[1]
