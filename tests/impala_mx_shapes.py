"""Shape table, oracle composition and arithmetic restatements of the impala matrix-core conv mode's tests
(IDQN_IMP_CONV=bf16x3, csrc/impala_mx_kernels.h; tests/test_impala_mx_shapes_host.py on the CPU, tests/test_gpu_impala_mx.py on
the device).  Not a test module.

The oracle is composed as tests/impala_shapes.py composes it (fp64 ``oracle.torch_ref.loss_and_grads``, ``oracle.qnet_ref``),
on this file's own rows.

Compile-time bounds of csrc/imp_mx_args.h the rows straddle: a workgroup tile of 16 x 16 positions (TH, TW; a wave owns four
rows, an MFMA M tile two), 16 input channels per k-step and LDS pass (KC), 32 output channels per workgroup (NB).  The grid is
(tiles, N tiles, nets x samples): images are never folded into a workgroup, so no B or K makes a workgroup ragged.
The rule: a layer whose leaf is ci -> co runs on the matrix cores when ci % 16 == 0 and co % 32 == 0 (``eligible``); the
uint8 conv never does.
"""
import functools

import numpy as np

GAMMA_N = 0.99
LR, EPS = 1e-3, 1e-8
TH, TW, KC, NB = 16, 16, 16, 32

# name: (obs, features, A, K, B)
ROWS = {
    "all_mx": ((32, 32, 4), [32, 64, 64, 16], 5, 2, 2),        # every conv but the uint8 one; Stack 0 pooled = exactly one tile; CI 32, 64; CO 1, 2 N tiles; even extents
    "tile_plus": ((33, 33, 3), [32, 32, 32], 4, 1, 2),         # pooled 17 x 17: one row and one column more than the tile; odd extents at every Stack (33 -> 17 -> 9 -> 5)
    "tile_minus": ((30, 29, 2), [16, 32, 32, 8], 3, 2, 1),     # pooled 15 x 15: one less; CI of exactly one k-step (Stack_1/Conv_0, 16 -> 32); Stack 0's 16 -> 16 stay
    "mixed_valu_mx": ((18, 20, 4), [16, 32, 32], 6, 2, 3),     # Stack 0 wholly on the vector ALUs, then eligible layers; the 16 -> 32 data gradient fills half an N tile
    "mixed_mx_valu": ((14, 11, 1), [32, 33, 32, 12], 3, 1, 5), # eligible (Stack 0 inner), then 32 -> 33, 33 -> 33, 33 -> 32 on the vector ALUs, then eligible again; width 32 + 1
    "one_row": ((1, 20, 2), [32, 32, 32], 3, 1, 4),            # a one-row frame: 1 x 10, 1 x 5, 1 x 3 under the matrix-core kernel
    "workload": ((84, 84, 4), [32, 64, 64, 512], 6, 2, 2),     # the workload's geometry (tests/impala_shapes.py): the near-tied pool windows of DESIGN.md 3.6
}
SEEDS = {"one_row": 3}


def eligible(ci, co):
    return ci > 0 and co > 0 and ci % KC == 0 and co % NB == 0


def conv_layers(obs, feats):
    """[(stack, conv, leaf ci, leaf co, H, W)] of the 15 convs: the frame each runs on."""
    from oracle import qnet_ref as Q

    out, h, w, ci = [], obs[0], obs[1], obs[2]
    for s in range(3):
        co = feats[s]
        ph, pw = Q.same_pad(h, 3, 2)[0], Q.same_pad(w, 3, 2)[0]
        out.append((s, 0, ci, co, h, w))
        out += [(s, i, co, co, ph, pw) for i in range(1, 5)]
        h, w, ci = ph, pw, co
    return out


def mx_layers(obs, feats):
    """the (stack, conv) pairs that run on the matrix-core kernel under the mode"""
    return [(s, i) for s, i, ci, co, _, _ in conv_layers(obs, feats) if not (s == 0 and i == 0) and eligible(ci, co)]


def expected_launches(obs, feats):
    """conv launch names of one learner step, in order, under the mode: forward of the trunk, then the data gradients"""
    mx = set(mx_layers(obs, feats))
    nm = lambda s, i, tag: ("k_imp_conv_mx<%s>" if (s, i) in mx else "k_imp_conv<%s>") % tag  # noqa: E731
    fwd = []
    for s in range(3):
        fwd.append("k_imp_conv<u8>" if s == 0 else nm(s, 0, "conv0"))
        for blk in range(2):
            fwd += [nm(s, 1 + 2 * blk, "inner"), nm(s, 2 + 2 * blk, "res")]
    bwd = []
    for s in (2, 1, 0):
        for blk in (1, 0):
            bwd += [nm(s, 2 + 2 * blk, "dgrad mask"), nm(s, 1 + 2 * blk, "dgrad mask skip")]
        if s > 0:
            bwd.append(nm(s, 0, "dgrad"))
    return fwd, bwd


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
    if name == "one_row":  # a 1 x 3 feature map: positive biases keep the final ReLU alive
        for n in p:
            if n.endswith("bias"):
                p[n] = np.abs(p[n]) + np.float32(0.05)
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
    """The float32 run of torch_ref against the fp64 one, per head: (|loss error|, {leaf: max |error| / max |gradient|})."""
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
    """(loss, grads, |td|) of head k for the loss  mean_b w_b td_b^2  (fp64 autograd), as impala_shapes.weighted_oracle."""
    import torch

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


def stage_outputs(name, k, which=0):
    """fp64 (Conv_0 outputs, pool outputs, Stack outputs) of head k's online (0) / target (1) net on state / next_state; the
    third Stack's output after the final ReLU, as the device keeps it."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    return stage_outputs_of(Q.head(pt if which else p, k), batch[3 if which else 0])


def stage_outputs_of(ph, states):
    """stage_outputs for one head's parameters ``ph`` on uint8 ``states``"""
    from oracle import qnet_ref as Q

    a = states.astype(np.float64) / 255.0
    c0s, pools, stacks = [], [], []
    for si in range(3):
        ps = {n[len(f"Stack_{si}/"):]: v for n, v in ph.items() if n.startswith(f"Stack_{si}/")}
        c0 = Q.conv_fwd(a, ps["Conv_0/kernel"].astype(np.float64), ps["Conv_0/bias"].astype(np.float64), 1)[0]
        c0s.append(c0)
        pools.append(Q.max_pool_same(c0))
        a = Q.impala_stack(ps, a)
        stacks.append(np.maximum(a, 0) if si == 2 else a)
    return c0s, pools, stacks


# ---- float32 restatements of the two conv kernels' arithmetic ------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32; a NaN stays a NaN (v_cvt_pk_bf16_f32)"""
    x = np.asarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float32)


def split3(x):
    """split3_pk (csrc/convp.h): x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), the differences in float32"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = bf16_rne(x)
        r = (x - x0).astype(np.float32)
        x1 = bf16_rne(r)
        r = (r - x1).astype(np.float32)
        x2 = bf16_rne(r)
    return x0, x1, x2


def _taps(x):
    """x [B, H, W, C] -> the nine SAME-padded shifted views [9][B, H, W, C], tap = kh * 3 + kw"""
    b, h, w, c = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return [xp[:, kh : kh + h, kw : kw + w, :] for kh in range(3) for kw in range(3)]


def conv_valu(x, w, bias, cic=8):
    """k_imp_conv: passes of ``cic`` input channels; inside a pass one float32 fma chain over (channel, kh, kw) from zero; the
    pass is then added to the total, which starts at the bias.  (The fma is restated as one float64 multiply-add rounded to
    float32: the product is exact in float64, the sum is rounded twice, which differs from a fused one on rare half-way cases.)"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    b, h, wd, ci = x.shape
    co = w.shape[-1]
    taps = _taps(x)
    acc = np.broadcast_to(np.asarray(bias, np.float32), (b, h, wd, co)).copy()
    for c0 in range(0, ci, cic):
        pa = np.zeros((b, h, wd, co), np.float32)
        for c in range(c0, min(c0 + cic, ci)):
            for t in range(9):
                pa = (taps[t][..., c : c + 1].astype(np.float64) * w[t // 3, t % 3, c].astype(np.float64) + pa).astype(np.float32)
        acc = (acc + pa).astype(np.float32)
    return acc


ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # (term of x, term of w): smallest first (csrc/convp.h)


def conv_mx(x, w, bias):
    """k_imp_conv_mx: passes of 16 input channels ascending; inside a pass the taps ascending; inside a tap the six partial
    products of ORDER, each one MFMA -- its 16 bf16 x bf16 products are exact, and their sum with the accumulator is restated
    as exact (float64) and rounded to float32 once, where the matrix core writes its float32 result.  The first five chain
    into the pass's small accumulator, x0 w0 into its main accumulator, both from zero; small + main is then added to the
    total, which starts at the bias."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    b, h, wd, ci = x.shape
    co = w.shape[-1]
    assert ci % KC == 0
    xs = [[t.astype(np.float64) for t in _taps(term)] for term in split3(x)]
    ws = [term.astype(np.float64) for term in split3(w)]
    acc = np.broadcast_to(np.asarray(bias, np.float32), (b, h, wd, co)).copy()
    for c0 in range(0, ci, KC):
        ps, pm = np.zeros((b, h, wd, co), np.float32), np.zeros((b, h, wd, co), np.float32)
        for t in range(9):
            for i, j in ORDER:
                prod = xs[i][t][..., c0 : c0 + KC] @ ws[j][t // 3, t % 3, c0 : c0 + KC, :]
                if (i, j) == (0, 0):
                    pm = (prod + pm).astype(np.float32)
                else:
                    ps = (prod + ps).astype(np.float32)
        acc = (acc + (ps + pm).astype(np.float32)).astype(np.float32)
    return acc


def conv0_outputs_f32(name, k, mode):
    """float32 Conv_0 outputs [3] of head k's online net on the row's states, under ``mode``: "valu" = every conv as
    k_imp_conv sums it, "bf16x3" = the eligible layers as k_imp_conv_mx sums them, the rest as k_imp_conv."""
    from oracle import qnet_ref as Q

    obs, feats, A, K, B, p, pt, batch = _case(name)
    ph = Q.head(p, k)
    mx = set(mx_layers(obs, feats)) if mode == "bf16x3" else set()
    a = (batch[0].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    out = []
    for s in range(3):
        conv = lambda i, v: (conv_mx if (s, i) in mx else functools.partial(conv_valu, cic=4 if (s, i) == (0, 0) else 8))(  # noqa: E731
            v, ph[f"Stack_{s}/Conv_{i}/kernel"], ph[f"Stack_{s}/Conv_{i}/bias"])
        c0 = conv(0, a)
        out.append(c0)
        x = Q.max_pool_same(c0).astype(np.float32)
        for blk in range(2):
            y = np.maximum(conv(1 + 2 * blk, np.maximum(x, 0)), 0)
            x = (conv(2 + 2 * blk, y) + x).astype(np.float32)
        a = x
    return out


def pool_selection(c0):
    """index (0..8, first maximum in (row, column) order; padding is -inf) of every 3 x 3 / 2 SAME window of c0 [B, H, W, C]"""
    from oracle import qnet_ref as Q

    b, h, w, c = c0.shape
    oh, lo_h, hi_h = Q.same_pad(h, 3, 2)
    ow, lo_w, hi_w = Q.same_pad(w, 3, 2)
    xp = np.pad(c0, ((0, 0), (lo_h, hi_h), (lo_w, hi_w), (0, 0)), constant_values=-np.inf)
    win = np.lib.stride_tricks.sliding_window_view(xp, (3, 3), axis=(1, 2))[:, ::2, ::2][:, :oh, :ow]
    return win.reshape(*win.shape[:4], 9).argmax(-1)
