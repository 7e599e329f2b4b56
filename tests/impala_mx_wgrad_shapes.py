"""Shape table, plan and arithmetic restatement of the impala matrix-core weight gradient's tests (IDQN_IMP_WGRAD=bf16x3,
csrc/impala_mx_wgrad_kernels.h; tests/test_impala_mx_wgrad_host.py on the CPU, tests/test_gpu_impala_mx_wgrad.py on the device).
Not a test module.

The rows of tests/impala_mx_shapes.py, with its ``case``, ``oracle``, ``f32_errors``, ``weighted_oracle`` and ``stage_outputs``
(evaluated on this file's table), ``split3`` and ``ORDER``, plus rows for what only the weight gradient can get wrong: its sum
runs over positions and samples, so the batch and the frame decide how many chunks a launch has and how full the last one is.

Compile-time bounds of csrc/imp_mx_wgrad_args.h: a tile of 8 x 16 output positions (TH, TW; a tile row is one k-step of the
MFMA), 8 tiles per chunk (TILES; tiles are numbered image major, then tile row, then tile column), 32 input channels (MB) and 32
output channels (NB) per workgroup.  The eligibility rule is the forward's (``M.eligible``); the uint8 conv never is eligible.
"""
import functools

import numpy as np

import impala_mx_shapes as M

GAMMA_N, LR, EPS = M.GAMMA_N, M.LR, M.EPS
TH, TW, MB, NB, TILES = 8, 16, 32, 32, 8
split3, ORDER, eligible, conv_layers, mx_layers, pool_selection, stage_outputs_of = (
    M.split3, M.ORDER, M.eligible, M.conv_layers, M.mx_layers, M.pool_selection, M.stage_outputs_of)

# name: (obs, features, A, K, B)
OWN_ROWS = {
    "one_chunk": ((32, 33, 3), [32, 32, 32], 3, 1, 2),        # Stack 0 pooled 16 x 17: 2 x 2 tiles x 2 samples = exactly one chunk
    "chunk_plus_tile": ((33, 32, 2), [32, 64, 32], 3, 2, 3),  # pooled 17 x 16: 3 tiles x 3 samples = one chunk and one tile; 32 -> 64 there too
    "many_chunks": ((33, 33, 1), [32, 32, 32], 2, 1, 6),      # pooled 17 x 17: 6 tiles x 6 samples = four chunks and a half; chunks cut inside images
    "small_after_large": ((20, 18, 2), [32, 32, 32], 3, 2, 5),  # the handle-history row: B = 5 (10 tiles, two chunks), then B = 2 (one)
}
ROWS = {**M.ROWS, **OWN_ROWS}
SEEDS = dict(M.SEEDS)


def _on_this_table(fn):
    """``fn`` of impala_mx_shapes, reading this file's rows (its caches are keyed by the row's name; the names are distinct)"""
    @functools.wraps(fn)
    def call(*args):
        rows, seeds = M.ROWS, M.SEEDS
        M.ROWS, M.SEEDS = ROWS, SEEDS
        try:
            return fn(*args)
        finally:
            M.ROWS, M.SEEDS = rows, seeds
    return call


case, oracle, f32_errors = _on_this_table(M.case), _on_this_table(M.oracle), _on_this_table(M.f32_errors)
weighted_oracle, stage_outputs = _on_this_table(M.weighted_oracle), _on_this_table(M.stage_outputs)


def leaf_name(s, i):
    return "Stack_%d/Conv_%d" % (s, i)


def plan(B, H, W, ci, co):
    """imxw_plan (csrc/imp_mx_wgrad_args.h): (tiles_h, tiles_w, n_tiles, n_chunks, m_blocks, n_blocks, part_len)"""
    th, tw = -(-H // TH), -(-W // TW)
    n_tiles = B * th * tw
    return th, tw, n_tiles, -(-n_tiles // TILES), -(-ci // MB), -(-co // NB), 9 * ci * co + co


def valu_chunks(B, H, W):
    """k_imp_wgrad's chunk count (8 x 16 tiles, 16 per chunk): ``wpart`` is sized for the larger plan"""
    return -(-(B * -(-H // 8) * -(-W // 16)) // 16)


def expected_wgrad_launches(obs, feats):
    """(k_imp_wgrad_mx launches, k_imp_wgrad launches) of one learner step under the mode"""
    mx = len(mx_layers(obs, feats))
    return mx, 15 - mx


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def wgrad_mx(x, dy, mirror=False, col_off=0, drop_ragged=False):
    """k_imp_wgrad_mx and k_imp_wreduce: x [B, H, W, CI] (after the ReLU, where the layer has one), dy [B, H, W, CO], float32
    -> (dW [3, 3, CI, CO], db [CO]) float32.

    Per chunk and output element two float32 accumulators from zero run over the chunk's tiles ascending, inside a tile over its
    eight rows ascending; a row is the six partial products of ORDER, each one MFMA -- its 16 bf16 x bf16 products (the row's
    columns) are exact and their sum with the accumulator is restated as exact (float64) and rounded to float32 once.  The
    first five chain into the small accumulator, x0 dy0 into the main one; the chunk's partial is small + main, and the
    partials are added in chunk order.  A row or tile past the frame adds zeros, which changes no float32 sum.  The bias:
    eight lanes per channel, lane j the columns 2 j, 2 j + 1 of every row in the same order, the lanes then added ascending.

    The three keywords restate the kernel WRONGLY, for tests/test_impala_mx_wgrad_host.py: taps mirrored, x one column off,
    the last ragged chunk dropped."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    B, H, W, CI = x.shape
    CO = dy.shape[-1]
    th, tw, n_tiles, n_chunks, *_ = plan(B, H, W, CI, CO)
    Hp, Wp = th * TH, tw * TW
    xp = np.zeros((B, Hp + 2, Wp + 3, CI), np.float32)
    xp[:, 1 : H + 1, 1 : W + 1] = x
    dp = np.zeros((B, Hp, Wp, CO), np.float32)
    dp[:, :H, :W] = dy
    nt = n_chunks * TILES

    def tiles(a, r0, c0):  # [B, ., ., C] -> [n_chunks, TILES, TH, TW, C] of the windows at (r0, c0) of every tile
        v = a[:, r0 : r0 + Hp, c0 : c0 + Wp].reshape(B, th, TH, tw, TW, -1).transpose(0, 1, 3, 2, 4, 5).reshape(n_tiles, TH, TW, -1)
        v = np.concatenate([v, np.zeros((nt - n_tiles,) + v.shape[1:], v.dtype)])
        return v.reshape(n_chunks, TILES, TH, TW, -1)

    xs = [np.stack([tiles(t, kh, kw + col_off) for kh in range(3) for kw in range(3)], 2).astype(np.float64) for t in split3(xp)]
    ds = [tiles(t, 0, 0).astype(np.float64) for t in split3(dp)]  # xs[term]: [chunk, tile, tap, row, col, CI]
    ps, pm = np.zeros((n_chunks, 9, CI, CO), np.float32), np.zeros((n_chunks, 9, CI, CO), np.float32)
    dt = tiles(dp, 0, 0)
    bs = np.zeros((n_chunks, TW // 2, CO), np.float32)
    for j in range(TILES):
        for row in range(TH):
            for i, jj in ORDER:
                prod = np.einsum("ntkc,nko->ntco", xs[i][:, j, :, row], ds[jj][:, j, row])
                if (i, jj) == (0, 0):
                    pm = (prod + pm).astype(np.float32)
                else:
                    ps = (prod + ps).astype(np.float32)
            bs = (bs + dt[:, j, row, 0::2]).astype(np.float32)
            bs = (bs + dt[:, j, row, 1::2]).astype(np.float32)
    part = (ps + pm).astype(np.float32)
    bpart = bs[:, 0]
    for j in range(1, TW // 2):
        bpart = (bpart + bs[:, j]).astype(np.float32)
    last = n_chunks - 1 if drop_ragged and n_tiles % TILES and n_chunks > 1 else n_chunks
    g, b = part[0], bpart[0]
    for c in range(1, last):
        g, b = (g + part[c]).astype(np.float32), (b + bpart[c]).astype(np.float32)
    if mirror:
        g = g[::-1]
    return g.reshape(3, 3, CI, CO), b


@functools.lru_cache(maxsize=None)
def conv_io(name, k):
    """fp64 {(stack, conv): (x [B, H, W, CI] as the conv reads it -- after the ReLU for the inner convs --, dy [B, H, W, CO])} of
    head k's online net in the oracle's loss: the tensors ImpWgradArgs describes, taken from torch_ref's own forward by
    recording its conv calls."""
    import torch

    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = case(name)
    rec = []
    real = T.F.conv2d

    def conv2d(inp, w, b=None, **kw):
        out = real(inp, w, b, **kw)
        if out.requires_grad:
            out.retain_grad()
            rec.append((inp, out))
        return out

    T.F.conv2d = conv2d
    try:
        T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "impala", GAMMA_N)
    finally:
        T.F.conv2d = real
    assert len(rec) == 15, len(rec)
    out = {}
    for n, (inp, o) in enumerate(rec):
        x = inp.detach()[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1).numpy()
        out[(n // 5, n % 5)] = (np.ascontiguousarray(x), np.ascontiguousarray(o.grad.permute(0, 2, 3, 1).numpy()))
    return out
