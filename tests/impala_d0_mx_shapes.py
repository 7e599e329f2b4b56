"""Shape table and plan restatement of the impala f32 matrix-core Dense_0 forward's tests (IDQN_IMP_D0=mfma,
csrc/impala_d0_mx_kernels.h; tests/test_impala_d0_mx_host.py on the CPU, tests/test_gpu_impala_d0_mx.py on the device).
Not a test module.

The helpers of tests/impala_shapes.py (``case``, ``oracle``, ``f32_errors``, ``weighted_oracle``) evaluated on this file's rows.
On an 8 x 8 observation the three pools leave 1 x 1, so the head's input has F = the third Stack's width and every row costs
milliseconds; what the kernel can get wrong is decided by F (passes of 64 features, rounds of four passes), D (tiles of 32 hidden
units; the default kernel's blocks of 64) and B (blocks of 32 samples).

Compile-time bounds of csrc/imp_d0_mx_args.h: PASS = 64 features, TILE = 32 samples x 32 units, WAVES = 4 passes per round,
XP = 33 floats of LDS pitch.
"""
import functools

import impala_shapes as S

GAMMA_N, LR, EPS = S.GAMMA_N, S.LR, S.EPS
PASS, TILE, WAVES, XP = 64, 32, 4, 33
LDS_BYTES = 4 * (WAVES * PASS * XP + WAVES * TILE * TILE)

# name: (obs, features, A, K, B)
ROWS = {
    "f63": ((8, 8, 1), [2, 3, 63, 33], 3, 1, 2),           # one ragged pass; D = 32 + 1
    "f64": ((8, 8, 1), [2, 3, 64, 32], 3, 1, 1),           # exactly one pass; D = exactly one tile; B = 1
    "f65": ((8, 8, 2), [2, 3, 65, 31], 3, 1, 3),           # a second pass of one feature, odd: its one MFMA is half padding; D = 32 - 1
    "f256": ((8, 8, 1), [2, 2, 256, 64], 3, 2, 2),         # exactly one round; D = two tiles = one block of the default kernel; K = 2
    "f257": ((8, 8, 1), [2, 2, 257, 65], 2, 1, 2),         # a second round of one pass of one feature; D = 64 + 1
    "f320": ((8, 8, 1), [2, 2, 320, 1], 3, 1, 2),          # five passes: a full round and one pass; D = 1
    "f448": ((8, 8, 1), [2, 2, 448, 8], 3, 1, 2),          # seven passes: the last round holds three
    "positions": ((16, 12, 2), [3, 4, 40, 12], 4, 2, 3),   # pooled 2 x 2 x 40: F = 160 from four positions; K = 2
    "b31": ((8, 8, 1), [2, 2, 65, 33], 3, 1, 31),          # B = 32 - 1
    "b32": ((8, 8, 1), [2, 2, 65, 33], 3, 1, 32),          # B = exactly one sample block
    "b33": ((8, 8, 1), [2, 2, 65, 33], 3, 2, 33),          # two sample blocks, one sample in the second; the history row
    "two_hidden": ((8, 8, 1), [2, 2, 70, 33, 17], 3, 2, 3),  # a second hidden layer behind Dense_0
    "mx_convs": ((16, 12, 2), [16, 32, 32, 33], 3, 2, 3),  # F = 128; Stack 1 and 2 eligible for the matrix-core conv modes: the three switches together
    "no_hid": ((8, 8, 1), [2, 2, 65], 3, 1, 3),            # no hidden dense layer: no Dense_0 launch of its own, the mode is a no-op
    "workload": ((84, 84, 4), [32, 64, 64, 512], 6, 2, 2),  # the workload's widths: F = 7744 (121 passes, 31 rounds, the last holds one), D = 512
}
SEEDS = {}
ORACLE_ROW = "positions"
HISTORY_ROW = "b33"
CROSS_MODES_ROW = "mx_convs"  # repeated with IDQN_IMP_CONV and IDQN_IMP_WGRAD also on


def _on_this_table(fn):
    """``fn`` of impala_shapes, reading this file's rows (its caches are keyed by the row's name; the names are distinct)"""
    @functools.wraps(fn)
    def call(*args):
        rows, seeds = S.ROWS, S.SEEDS
        S.ROWS, S.SEEDS = ROWS, SEEDS
        try:
            return fn(*args)
        finally:
            S.ROWS, S.SEEDS = rows, seeds
    return call


case, oracle, f32_errors, weighted_oracle = (_on_this_table(f) for f in (S.case, S.oracle, S.f32_errors, S.weighted_oracle))
assert set(ROWS) & set(S.ROWS) == {"workload"} and ROWS["workload"] == S.ROWS["workload"]  # (the caches are keyed by name)


def pooled(n):
    """extent of a frame side behind the three stride-2 SAME pools"""
    for _ in range(3):
        n = -(-n // 2)
    return n


def dense0(name):
    """(F, D, n_dense) of a row: Dense_0's features and hidden units (None without a hidden layer), dense layers of the head"""
    obs, feats, A, K, B = ROWS[name]
    F = pooled(obs[0]) * pooled(obs[1]) * feats[2]
    return F, (feats[3] if len(feats) > 3 else None), len(feats) - 3 + 1


def applies(name):
    """impd0x_applies: the handle launches a Dense_0 forward of its own"""
    return dense0(name)[2] >= 2


def plan(B, F, D, nets):
    """impd0x_plan (csrc/imp_d0_mx_args.h): (passes, rounds, last_round, grid_x, grid_y, grid_z, lds_bytes)"""
    passes = -(-F // PASS)
    rounds = -(-passes // WAVES)
    return passes, rounds, passes - (rounds - 1) * WAVES, -(-D // TILE), -(-B // TILE), nets, LDS_BYTES


def shape_ok(B, F, D, nets):
    """impd0x_shape_ok"""
    return int(min(B, F, D, nets) >= 1 and nets <= 65535 and -(-B // TILE) <= 65535 and F * D <= 1 << 29 and B * F <= 1 << 29)


def mode_of(v):
    """impd0_mode_of: 0 = valu, 1 = mfma, -1 = refused"""
    return 0 if v is None or v == "valu" else 1 if v == "mfma" else -1
