"""Case table of vectorised impala acting (``idqn_act_host_many_impala``, csrc/imp_act_many_kernels.h), shared by
tests/test_impala_act_many_host.py (CPU: the table against its coverage conditions) and tests/test_gpu_impala_act_many.py (device:
one call against the loop of ``idqn_act_host``, byte for byte).  Not a test module.

A case is (row, n, head assignment, which).  ``row`` names a shape of tests/impala_shapes.py, or ``five_heads`` below (that
table has no row with more than two heads, and the grouping needs more to permute).  The states are the row's batch, ``state``
then ``next_state``, repeated up to n.

The Dense_0 plan of csrc/imp_act_many_args.h, restated (``d0_plan``): F features are cut into passes of 64 (the last one ragged),
a workgroup owns 64 hidden units x 4 passes, one pass per wave, so the grid is (ceil(D / 64), ceil(passes / 4), groups); the
states are grouped by head, heads ascending, call order within a group, and a lane holds 8 states of its group at a time (a group of
more walks its weights again).  Every (state, pass, unit) sum is stored, [n][passes][D] floats, and the tail adds them to the
bias in pass order.  A head without a hidden layer has no Dense_0 launch.
"""
import functools

import numpy as np

import impala_shapes as S

MAX, SC, PASS, OC, PPW = 32, 8, 64, 64, 4  # states per call / per register chunk, features per pass, units and passes per workgroup

EXTRA_ROWS = {
    "five_heads": ((7, 10, 2), [3, 5, 4, 12], 5, 5, 4),  # odd_even's geometry with K = 5: five groups, a permuted order, an unused head
}
ASSIGNMENTS = ("one", "last", "rot", "desc", "skip")

# (row, n, assignment, which)
CASES = [
    # the rows: the smallest shapes at which each kernel can go wrong
    ("odd_even", 3, "rot", 0),         # both pool pad classes, an extent of 1, K = 2; F = 8 (one ragged pass), D = 12
    ("no_hidden", 3, "one", 1),        # no Dense_0 launch: the tail runs F x 40 on the features; A = 40 > 32, K = 1
    ("tile_plus", 2, "one", 0),        # ragged edge tiles, channels 7 / 9 / 33; F = 198: 4 passes = one full range, the last pass 6 features
    ("tile_minus", 3, "desc", 0),      # tile - 1, channels 31 / 8 / 9; no hidden layer, K = 2
    ("u8_tail", 2, "one", 1),          # 5 frame channels: the uint8 conv's ragged second pass, per-net image addressing
    ("d0_blocks", 2, "one", 0),        # F = 60 < 64: one ragged pass; D = 65: a second column block of one unit
    ("mid", 3, "rot", 1),              # F = 128: two full passes; D = 64: exactly one column block
    ("tie", 4, "rot", 0),              # exact ties in the pools of head 0
    ("one_row", 2, "one", 0),          # a one-row frame, F = 2, no hidden layer
    ("workload", 3, "rot", 0),         # F = 7744: 121 full passes, 31 ranges, the last holds ONE pass; D = 512: 8 column blocks
    ("reference_test", 2, "desc", 1),  # F = 605: 10 passes (the last 29 features), 3 ranges, the last holds two; D = 9
    # n at the edges of the register chunk and of the call, all on one head (one group: 1 .. 4 chunks)
    ("odd_even", 1, "one", 0),
    ("odd_even", 2, "one", 1),
    ("odd_even", SC, "one", 0),
    ("odd_even", SC + 1, "last", 0),
    ("odd_even", 31, "one", 1),
    ("odd_even", 32, "last", 0),
    # the same n spread over both heads
    ("odd_even", SC + 1, "rot", 1),
    ("odd_even", 31, "desc", 0),
    ("odd_even", 32, "rot", 0),
    # five heads: the grouping permutes the states
    ("five_heads", 1, "last", 0),
    ("five_heads", 5, "desc", 0),
    ("five_heads", 7, "rot", 1),
    ("five_heads", 13, "skip", 0),
    ("five_heads", 32, "desc", 1),
    ("five_heads", 32, "skip", 0),
]


def shape(row):
    """(obs, feats, A, K, B) of a row of either table."""
    return (EXTRA_ROWS.get(row) or S.ROWS[row])[:5]


@functools.lru_cache(maxsize=None)
def case(row):
    """(obs, feats, A, K, B, online, target, batch), as ``impala_shapes.case``."""
    if row in S.ROWS:
        return S.case(row)
    from oracle import qnet_ref as Q

    obs, feats, A, K, B = EXTRA_ROWS[row]
    p, pt = Q.init_params(10, "impala", obs, A, feats, K), Q.init_params(11, "impala", obs, A, feats, K)
    rng = np.random.default_rng(12)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = Q.synthetic_batch(13, B, obs, A, "cnn")
    return obs, feats, A, K, B, p, pt, batch


def states(row, n):
    batch = case(row)[7]
    pool = [np.asarray(s) for s in list(batch[0]) + list(batch[3])]
    return [pool[e % len(pool)] for e in range(n)]


def heads(assignment, n, K):
    """The head of each of the n states: all on head 0 / on the last head / e mod K / descending / head 0 unused."""
    if assignment == "one":
        return [0] * n
    if assignment == "last":
        return [K - 1] * n
    if assignment == "rot":
        return [e % K for e in range(n)]
    if assignment == "desc":
        return [K - 1 - e % K for e in range(n)]
    if assignment == "skip":
        return [1 + e % (K - 1) for e in range(n)] if K > 1 else [0] * n
    raise KeyError(assignment)


def geometry(row):
    """(F, D): flattened features of the third Stack and hidden units of Dense_0 (D = None: no hidden layer)."""
    obs, feats, A, K, B = shape(row)
    h, w = obs[0], obs[1]
    for _ in range(3):
        h, w = -(-h // 2), -(-w // 2)  # 3 x 3 / 2 max-pool, SAME
    return h * w * feats[2], (feats[3] if len(feats) > 3 else None)


def d0_plan(F, D):
    """dict(n_pass, ranges, col_blocks, last_pass_features, last_range_passes, last_block_units, part_floats)."""
    n_pass = -(-F // PASS)
    ranges = -(-n_pass // PPW)
    col_blocks = -(-D // OC)
    return dict(n_pass=n_pass, ranges=ranges, col_blocks=col_blocks, last_pass_features=F - (n_pass - 1) * PASS,
                last_range_passes=n_pass - (ranges - 1) * PPW, last_block_units=D - (col_blocks - 1) * OC, part_floats=MAX * n_pass * D)


def grouped(head_list, K):
    """(n_groups, order, g_head, g_start, g_count): states sorted (stable) by head, one group per head in use."""
    h = np.asarray(head_list)
    order = np.argsort(h, kind="stable")
    used = sorted(set(h.tolist()))
    counts = [int((h == k).sum()) for k in used]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int).tolist()
    assert all(0 <= k < K for k in used)
    return len(used), order.tolist(), used, starts, counts


def chunks(count):
    """(register chunks of a group of ``count`` states, states of its last chunk)."""
    c = -(-count // SC)
    return c, count - (c - 1) * SC
