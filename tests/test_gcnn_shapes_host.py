"""CPU (no GPU): the general-shape cnn path's shape table (tests/gcnn_shapes.py) is worth running on the device.

Every row is one ``cnn_fast_shape()`` refuses and ``build_layout`` accepts, with the reference's leaves; the table's coverage
claims -- every Conv_0 pad class on each axis with an even and an odd Conv_1 input, extents of 1, frames below the kernel size,
flatten and hidden widths on both sides of 512 -- are computed from ``oracle.qnet_ref.same_pad``, not assumed; no leaf of any
head has an all-zero fp64 gradient (a kernel that wrote nothing would pass such a leaf); the two oracles, hand-derived
im2col / col2im and torch autograd over explicit ``F.pad``, agree to 1e-12 at every row, frames below the kernel size included;
float32 autograd meets the device bars, so the fallback bar (4 x its error) is not expected to be used.
"""
import os

import numpy as np
import pytest

import gcnn_shapes as S

NAMES = list(S.ROWS)


def _fast_shape(obs, feats, A):
    """``cnn_fast_shape`` (csrc/qnet.hip) for a handle without quantile heads and without IDQN_CNN_GENERAL."""
    if len(feats) != 4 or obs[2] != 4 or obs[0] < 8 or obs[1] < 8 or A > 32:
        return False
    if any(f not in (32, 64) for f in feats[:3]):
        return False
    return feats[3] % 128 == 0 and 128 <= feats[3] <= 512


def test_the_rule_restated_here_accepts_the_plane_path_shapes():
    assert _fast_shape((84, 84, 4), [32, 64, 64, 512], 6) and _fast_shape((8, 8, 4), [32, 32, 32, 128], 32)
    assert not _fast_shape((84, 84, 4), [32, 64, 64, 512], 33) and not _fast_shape((84, 84, 4), [32, 64, 64, 640], 6)


@pytest.mark.parametrize("name", NAMES)
def test_row_takes_the_general_path_and_has_the_reference_leaves(name):
    from oracle import qnet_ref as Q
    from slimdqn import _hip

    obs, feats, A, K, B = S.ROWS[name]
    assert not _fast_shape(obs, feats, A)
    leaves, stride = _hip.layout(_hip.make_config("cnn", K, A, obs, feats, max(B, 32), S.LR, S.EPS, S.GAMMA_N))
    assert [(n, tuple(s)) for n, _, s in leaves] == [(n, tuple(s)) for n, s in Q.leaf_shapes("cnn", obs, A, feats)]
    assert stride % 64 == 0 and all(off % 64 == 0 for _, off, _ in leaves)
    ends = [off + int(np.prod(s)) for _, off, s in leaves]
    assert all(e <= nxt for e, nxt in zip(ends, [off for _, off, _ in leaves][1:] + [stride]))
    # small: no row has more than about 1e6 conv outputs in a step (2K nets of B samples)
    geo, F = S.geometry(obs, feats)
    assert sum(2 * K * B * g[2] * g[3] * f for g, f in zip(geo, feats)) <= 1_000_000
    assert leaves[6][2][0] == F


def test_table_covers_the_pad_classes_and_parities():
    pads = {(li, ax): set() for li in range(3) for ax in (0, 1)}
    combos = {0: set(), 1: set()}  # axis -> {(Conv_0 pad, Conv_1 input parity)}
    mixed = []
    for name, (obs, feats, A, K, B) in S.ROWS.items():
        geo, _ = S.geometry(obs, feats)
        for li, g in enumerate(geo):
            pads[(li, 0)].add(g[4])
            pads[(li, 1)].add(g[5])
        combos[0].add((geo[0][4], geo[1][0] % 2))
        combos[1].add((geo[0][5], geo[1][1] % 2))
        if obs[0] != obs[1] and geo[0][4] != geo[0][5] and min(obs[:2]) > 1:
            mixed.append(name)
    conv0 = {(2, 2), (3, 4), (3, 3), (2, 3)}
    for ax in (0, 1):
        assert pads[(0, ax)] == conv0                      # extent = 0, 1, 2, 3 mod 4
        assert pads[(1, ax)] == {(1, 1), (1, 2)}           # an even and an odd Conv_1 input
        assert pads[(2, ax)] == {(1, 1)}
        assert combos[ax] == {(p, par) for p in conv0 for par in (0, 1)}, (ax, sorted(combos[ax]))
    # H != W with the classes differing per axis: a transposed pad cannot cancel
    assert {"h9_w14", "h11_w6", "h13_w7", "h12_w11", "no_hidden", "hid513"} <= set(mixed)
    # the rule applies below the kernel size too: extents 1, 5, 6, 7 pad Conv_0 by 7, 7, 6, 5 in all
    assert S.geometry((1, 5, 1), [2, 3, 2])[0][0][4:] == ((3, 4), (3, 4))
    assert S.geometry((7, 6, 1), [2, 3, 2])[0][0][4:] == ((2, 3), (3, 3))


def test_table_covers_the_edges_it_names():
    rows = S.ROWS
    assert rows["unit"] == ((1, 1, 1), [1, 1, 1], 1, 1, 1)
    assert [n for n, r in rows.items() if r[0][0] == 1] == ["unit", "one_row"]
    assert [n for n, r in rows.items() if r[0][1] == 1] == ["unit", "one_col"]
    below = [n for n, r in rows.items() if r[0][0] < 8 and r[0][1] < 8 and min(r[0][:2]) > 1]
    assert below == ["sub_kernel"] and rows["sub_kernel"][0][0] != rows["sub_kernel"][0][1]
    assert {r[0][2] for r in rows.values()} >= {1, 3, 4, 5}
    assert {f for r in rows.values() for f in r[1][:3]} >= {1, 7, 33, 65, 32, 64}
    assert {len(r[1]) - 3 for r in rows.values()} == {0, 1, 2}         # hidden dense layers
    assert {r[2] for r in rows.values()} >= {1, 33, 40}                # actions
    assert {r[4] for r in rows.values()} >= {1, 33, 34}                # batch sizes
    assert {r[3] for r in rows.values()} >= {1, 3}                     # heads
    assert rows["nature_96"][:2] == ((10, 14, 4), [32, 64, 64, 96])
    for name in S.WEIGHTED + S.REPLAY:
        assert name in rows
    assert any(rows[n][2] > 32 for n in S.WEIGHTED)
    for name in S.REPLAY:
        obs = rows[name][0]
        assert obs[2] != 4 and (obs[0] % 2 or obs[1] % 2)


def test_flatten_and_hidden_widths_straddle_512():
    """F and dmax as gcnn_setup computes them (dmax includes the flatten width): 512 exactly and 513 through the frame, 512 and
    513 through a hidden layer behind a small F, and F = 1."""
    fd = {n: (S.geometry(obs, feats)[1], S.dmax(obs, feats, A)) for n, (obs, feats, A, K, B) in S.ROWS.items()}
    assert fd["f512"] == (512, 512) and max(S.ROWS["f512"][1][3:] + [S.ROWS["f512"][2]]) <= 512
    assert fd["f513"] == (513, 513) and max(S.ROWS["f513"][1][3:] + [S.ROWS["f513"][2]]) <= 512
    assert fd["hid512"] == (8, 512) and fd["hid513"] == (8, 513)
    assert fd["unit"] == (1, 1)
    assert S.FC_MAX_WIDTH == 512
    assert sorted(n for n, (F, d) in fd.items() if d > S.FC_MAX_WIDTH) == ["f513", "hid513"]
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "i-dqn_amd", "csrc", "fc_kernels.h")).read()
    assert "#define FC_MAX_WIDTH 512" in src


@pytest.mark.parametrize("name", NAMES)
def test_every_leaf_has_a_gradient_and_float32_meets_the_bars(name):
    obs, feats, A, K, B, p, pt, batch = S.case(name)
    for k, (want, (loss_err, leaf_err)) in enumerate(zip(S.oracle(name), S.f32_errors(name))):
        assert set(want["grads"]) == set(p)
        for leaf, g in want["grads"].items():
            assert np.abs(g).max() > 0, (name, k, leaf)
        assert ((~batch[4]) & (np.abs(want["td"]) > 0)).any(), (name, k, "no non-terminal sample with a TD error")
        for i in range(3):  # every stage the device test reads is live on both nets
            assert want["act"][i].max() > 0 and want["act_next"][i].max() > 0 and np.abs(want["dact"][i]).max() > 0, (name, k, i)
        print(name, k, "f32 loss error", loss_err, "worst leaf", max(leaf_err.values()))
        assert loss_err <= 1e-5 * max(1.0, abs(want["loss"]))
        assert max(leaf_err.values()) <= 2e-5, (name, k, max(leaf_err, key=leaf_err.get))
    if B > 1:
        assert batch[4][0]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_oracles_agree(name):
    """qnet_ref (im2col over np.pad) and torch_ref (autograd over F.pad) in fp64: two independent statements of SAME padding."""
    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    obs, feats, A, K, B, p, pt, batch = S.case(name)
    for k, want in enumerate(S.oracle(name)):
        loss, grads = T.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", S.GAMMA_N)
        assert abs(loss - want["loss"]) <= 1e-12 * max(1.0, abs(want["loss"]))
        for leaf, g in want["grads"].items():
            assert np.abs(grads[leaf] - g).max() <= 1e-12 * np.abs(g).max(), (name, k, leaf)


@pytest.mark.parametrize("name", S.WEIGHTED)
def test_weighted_oracle_is_the_weighted_loss(name):
    obs, feats, A, K, B, p, pt, batch = S.case(name)
    w = S.weights(name).astype(np.float64)
    for k, (loss, grads, td) in enumerate(S.weighted_oracle(name)):
        assert np.array_equal(td, np.abs(S.oracle(name)[k]["td"]))
        assert abs(loss - (w * td * td).mean()) <= 1e-15 * max(1.0, loss)
        assert all(np.abs(g).max() > 0 for g in grads.values())


def test_the_gap_rule_excuses_few_actions():
    """The device test compares an action with the fp64 argmax where the oracle's top-two gap exceeds 1e-4 max(1, max |q|): on
    the oracle alone, fewer than one in four of all (row, head, state) triples fall under that."""
    excused = total = 0
    for name, (obs, feats, A, K, B) in S.ROWS.items():
        for k in range(K):
            for e in (0, 1):
                q = S.act_oracle(name)[0][k][e]
                total += 1
                excused += not S.top_two_gap(q) > 1e-4 * max(1.0, np.abs(q).max())
    print("excused", excused, "of", total)
    assert 4 * excused < total
