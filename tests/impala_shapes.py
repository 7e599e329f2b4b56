"""Shape table and oracle composition of the impala architecture's tests (tests/test_impala_shapes_host.py on the CPU,
tests/test_gpu_impala.py on the device).  Not a test module.

Per head: loss and every leaf gradient from ``oracle.torch_ref.loss_and_grads(..., "impala", gamma_n)`` in fp64 (autograd;
torch's CPU max_pool2d backward sends a window's gradient to its FIRST maximum in (row, column) order), Q-values from
``oracle.qnet_ref.forward``, Adam from ``oracle.qnet_ref.adam_update``.  Batches are ``synthetic_batch(..., "cnn")`` with one
terminal sample forced; biases are drawn as tests/test_gpu_general_shapes.py draws them.

Compile-time bounds of csrc/impala_kernels.h the rows straddle: tile 8 x 16 positions (IMP_TH, IMP_TW), 8 output channels
per lane (IMP_CB), 32 per workgroup (IMP_COB), 8 input channels per LDS pass (IMP_CIC; 4 for the uint8 conv), 16 tiles per
weight-gradient chunk (IMP_WG_TILES); Dense_0 of a head with a hidden layer: 64 features / hidden units per LDS pass and 64 hidden
units per workgroup (IMP_D0_IC, IMP_D0_OC), 32 features per gradient workgroup (IMP_D0_R), 32 samples per block (IMP_D0_SB).
"""
import functools

import numpy as np

GAMMA_N = 0.99
LR, EPS = 1e-3, 1e-8

# name: (obs, features, A, K, B)
ROWS = {
    "odd_even": ((7, 10, 2), [3, 5, 4, 12], 5, 2, 5),         # 7 -> 4 -> 2 -> 1 and 10 -> 5 -> 3 -> 2: both pad classes, an extent of 1
    "no_hidden": ((12, 9, 4), [8, 6, 8], 40, 1, 33),          # no hidden dense layer, A > 32, B > 32; 66 tiles = 5 chunks, the last ragged
    "mid": ((16, 16, 4), [16, 32, 32, 64], 6, 2, 8),          # exactly one tile per image, exactly one chunk (16 tiles)
    "one_row": ((1, 5, 1), [2, 2, 2], 3, 1, 4),               # a one-row frame
    "workload": ((84, 84, 4), [32, 64, 64, 512], 6, 2, 2),    # the workload's geometry: 66 tiles per image, 9 chunks
    "tile_plus": ((9, 17, 3), [7, 9, 33, 6], 3, 1, 2),        # tile height / width + 1 (ragged 1-row, 1-column edge tiles); channels 8 - 1, 8 + 1, 32 + 1
    "tile_minus": ((7, 15, 2), [31, 8, 9], 4, 2, 3),          # tile height / width - 1; channels 32 - 1, exactly 8, 8 + 1; one chunk (3 tiles)
    "chunks_17": ((8, 16, 1), [4, 4, 4, 5], 2, 1, 17),        # exactly the tile; 17 tiles = one full chunk + one tile
    "reference_test": ((84, 84, 4), [3, 7, 5, 9], 4, 2, 2),   # the reference's own unit-test configuration (widths, A, K drawn in 1..9)
    "u8_tail": ((9, 6, 5), [4, 3, 5, 7], 3, 1, 3),            # 5 frame channels: the uint8 conv's second LDS pass (4 per pass) is ragged
    "d0_blocks": ((20, 28, 1), [2, 2, 5, 65], 2, 1, 33),      # Dense_0 kernels: 60 features (32 + 28, under 64), 64 + 1 hidden units, 2 sample blocks
    "tie": ((7, 10, 2), [3, 5, 4, 12], 5, 2, 5),              # head 0: Stack_0/Conv_0 = 0 * x + 0.5 -> every Stack-0 pool window is an exact tie
}
SEEDS = {"one_row": 3}


def case(name):
    """(obs, feats, A, K, B, online, target, batch) of a row: float32 parameters [K, ...], numpy batch."""
    return _case(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    from oracle import qnet_ref as Q

    obs, feats, A, K, B = ROWS[name]
    seed = SEEDS.get(name, 0)
    p = Q.init_params(seed, "impala", obs, A, feats, K)
    pt = Q.init_params(seed + 1, "impala", obs, A, feats, K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    if name == "one_row":  # a 1 x 1 feature map of two channels: positive biases keep the final ReLU alive
        for n in p:
            if n.endswith("bias"):
                p[n] = np.abs(p[n]) + np.float32(0.05)
    if name == "tie":
        p["Stack_0/Conv_0/kernel"][0] = 0.0
        p["Stack_0/Conv_0/bias"][0] = 0.5
    batch = Q.synthetic_batch(seed + 3, B, obs, A, "cnn")
    batch[4][0] = True
    for a in list(p.values()) + list(pt.values()) + list(batch):
        a.setflags(write=False)
    return obs, feats, A, K, B, p, pt, batch


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per head k: dict(loss, grads {leaf: fp64}, q [B, A], q_next [B, A]) -- fp64, computed once per row."""
    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = _case(name)
    out = []
    for k in range(K):
        loss, grads = T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "impala", GAMMA_N)
        out.append({"loss": loss, "grads": grads, "q": Q.forward(Q.head(p, k), batch[0], "impala"),
                    "q_next": Q.forward(Q.head(pt, k), batch[3], "impala")})
    return out


@functools.lru_cache(maxsize=None)
def f32_errors(name):
    """The float32 run of torch_ref against the fp64 one on the same inputs, per head: (|loss error|, {leaf: max |error| /
    max |gradient|}).  4 x the leaf's figure is the fallback bar of a leaf that misses 2e-5 on the device."""
    import torch

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = _case(name)
    out = []
    for k, want in enumerate(oracle(name)):
        loss, grads = T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "impala", GAMMA_N, dtype=torch.float32)
        out.append((abs(loss - want["loss"]),
                    {n: float(np.abs(grads[n] - g).max() / (np.abs(g).max() + 1e-300)) for n, g in want["grads"].items()}))
    return out


def weighted_oracle(name, k, weights):
    """(loss, grads, |td|) of head k for the prioritized-replay extension's loss  mean_b w_b td_b^2  (fp64 autograd)."""
    import torch

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = _case(name)
    dt = torch.float64
    po = {n: T._t(a[k], dt).requires_grad_(True) for n, a in p.items()}
    ptt = {n: T._t(a[k], dt) for n, a in pt.items()}
    q = T.forward_head(po, torch.as_tensor(batch[0]), "impala", dt)
    with torch.no_grad():
        qn = T.forward_head(ptt, torch.as_tensor(batch[3]), "impala", dt)
    tgt = T._t(batch[2], dt) + (1 - T._t(batch[4].astype(np.int64), dt)) * GAMMA_N * qn.max(1).values
    td = q.gather(1, torch.as_tensor(batch[1].astype(np.int64))[:, None])[:, 0] - tgt
    loss = (T._t(weights, dt) * td**2).mean()
    loss.backward()
    return float(loss.detach()), {n: t.grad.numpy() for n, t in po.items()}, td.detach().abs().numpy()


def stack_outputs(name, k, which=0):
    """fp64 (pool outputs, Stack outputs) of head k's online (0) / target (1) net on state / next_state; the third Stack's
    output is given after the final ReLU, as the device keeps it."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    ph = Q.head(pt if which else p, k)
    a = batch[3 if which else 0].astype(np.float64) / 255.0
    pools, stacks = [], []
    for si in range(3):
        ps = {n[len(f"Stack_{si}/"):]: v for n, v in ph.items() if n.startswith(f"Stack_{si}/")}
        c0 = Q.conv_fwd(a, ps["Conv_0/kernel"].astype(np.float64), ps["Conv_0/bias"].astype(np.float64), 1)[0]
        pools.append(Q.max_pool_same(c0))
        a = Q.impala_stack(ps, a)
        stacks.append(np.maximum(a, 0) if si == 2 else a)
    return pools, stacks


def last_max_pool_conv0_grad(name, k):
    """Head k's Stack_0/Conv_0/kernel gradient under a "LAST maximum of the window wins" pool backward (fp64): the model the
    tie row tells apart from the oracle's first-maximum rule.  Stack 0's pool is replaced by a hand-written autograd function."""
    import torch
    import torch.nn.functional as F

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = _case(name)

    class LastMaxPool(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):  # x: padded with -inf, [B, C, Hp, Wp]
            win = x.unfold(2, 3, 2).unfold(3, 3, 2)  # B, C, PH, PW, 3, 3
            flat = win.reshape(*win.shape[:4], 9)
            m = flat.max(-1).values
            idx = 8 - torch.flip(flat == m[..., None], [-1]).to(torch.int8).argmax(-1)  # the last position of the maximum
            ctx.save_for_backward(idx)
            ctx.shape = x.shape
            return m

        @staticmethod
        def backward(ctx, g):
            (idx,) = ctx.saved_tensors
            dx = torch.zeros(ctx.shape, dtype=g.dtype)
            b, c, ph, pw = g.shape
            for i in range(ph):
                for j in range(pw):
                    kh, kw = idx[:, :, i, j] // 3, idx[:, :, i, j] % 3
                    bi, ci = torch.meshgrid(torch.arange(b), torch.arange(c), indexing="ij")
                    dx.index_put_((bi, ci, 2 * i + kh, 2 * j + kw), g[:, :, i, j], accumulate=True)
            return dx

    dt = torch.float64
    po = {n: T._t(a[k], dt).requires_grad_(True) for n, a in p.items()}
    ptt = {n: T._t(a[k], dt) for n, a in pt.items()}
    orig = F.max_pool2d
    calls = {"n": 0}

    def pool(x, *args, **kw):
        calls["n"] += 1
        return LastMaxPool.apply(x) if calls["n"] == 1 else orig(x, *args, **kw)

    F.max_pool2d = pool
    try:
        q = T.forward_head(po, torch.as_tensor(batch[0]), "impala", dt)
    finally:
        F.max_pool2d = orig
    with torch.no_grad():
        qn = T.forward_head(ptt, torch.as_tensor(batch[3]), "impala", dt)
    tgt = T._t(batch[2], dt) + (1 - T._t(batch[4].astype(np.int64), dt)) * GAMMA_N * qn.max(1).values
    qa = q.gather(1, torch.as_tensor(batch[1].astype(np.int64))[:, None])[:, 0]
    ((qa - tgt) ** 2).mean().backward()
    return po["Stack_0/Conv_0/kernel"].grad.numpy()
