"""CPU side of the i-IQN shape table (tests/iqn_shapes.py): what the table covers is asserted from its rows and from the restated
planner, every row's inputs meet the two conditions the GPU test relies on at the row's seed shift and at no smaller one, the inputs are
conditioned (no ReLU pre-activation within RELU_MARGIN of zero), and the oracle's own numpy-fp32 restatement stays within HALF of every
bar the GPU test applies.  A row that breaks the half rule gets a seed shift, never a wider bar.  Figures are printed (``-s``); the only one that
sets a bar is MOMENT_FP32_DEV.
"""
import numpy as np
import pytest

import iqn_shapes as T

ROUTES = ("stream", "gemm-dgrad", "two-split", "fused")


def test_table_covers_every_branch():
    rows = T.TABLE
    assert all(r.why for r in rows) and len({r.why for r in rows}) == len(rows), "one reason per row"
    assert all(1 <= r.N <= 64 and 1 <= r.B <= 256 and r.feats[3] % 256 == 0 for r in rows)
    per, qg, hg = ({T.groups(r)[i] for r in rows} for i in range(3))
    assert per == set(range(1, 9)), per
    assert qg == {1, 2, 3, 4}, qg
    assert hg >= {1, 2, 3, 6, 7, 8}, hg
    assert any(r.N > 8 and T.groups(r) == (1, 1, 1) for r in rows), "a prime N above 8"
    by_route = {}
    for r in rows:
        by_route.setdefault((T.route(r), r.feats[3]), []).append(r)
    for route in ROUTES:
        assert (route, 256) in by_route and (route, 512) in by_route, route
    fused = [T.plan(r) for r in rows if T.route(r) == "fused"]
    assert {p["n_jh"] for p in fused} == {1, 2}
    items = {T.plan(r)["items"]: T.route(r) for r in rows if T.dims(r)[3] % 16 == 0 and T.dims(r)[2] == 1}
    assert items[256] == "two-split" and items[264] == "fused", "both sides of the nb = 1 threshold"
    F = {T.dims(r)[0] for r in rows}
    assert {32, 64, 288, 576} <= F and min(F) < 256
    assert len({T.route(r) for r in rows if r.N >= 33}) >= 3
    many = {T.route(r) for r in rows if T.dims(r)[2] > 1 and T.dims(r)[3] % 16 == 0}
    assert many == {"fused", "two-split"}, "among nb > 1 rows both planner outcomes occur"
    assert {T.dims(r)[2] for r in rows} >= {1, 2, 4, 8} and {r.B for r in rows} >= {1, 20, 31, 32, 33, 64, 100, 256}
    # the subsets
    assert all(T.route(T.BY_ID[i]) == "fused" for i in T.FUSE_OFF_ROWS) and any(T.dims(T.BY_ID[i])[2] > 1 for i in T.FUSE_OFF_ROWS)
    assert sum(T.dims(T.BY_ID[i])[2] == 1 for i in T.FUSE_OFF_ROWS) == 3
    assert sorted(T.route(T.BY_ID[i]) for i in T.WEIGHTED_ROWS) == sorted(ROUTES)
    assert [T.BY_ID[i].N for i in T.ACT_ROWS] == [33, 61, 64]
    chained = {T.route(T.BY_ID[i]) for i in T.CHAIN_IDS}
    assert chained == set(ROUTES) and "K32_N16_J512" in T.CHAIN_IDS
    assert all(T.chained(r) for r in rows if T.route(r) == "fused")


def test_expected_route_names():
    by = T.BY_ID
    assert T.expected_route(by["N7"]) == ["iqn dense0 dgrad", "factor planes", "dense0 wgrad + adam"]
    assert T.expected_route(by["N8"]) == ["iqn dense0 dgrad", "factor planes", "dense0 wgrad + adam"]
    assert T.expected_route(by["N16"]) == ["iqn dense0 dgrad + wgrad", "iqn dense0 adam"]
    assert T.expected_route(by["K33_N16_J512"]) == ["iqn dense0 dgrad + wgrad + adam"]
    assert T.expected_route(by["K32_N16_J512"]) == ["iqn dense0 dgrad + wgrad", "iqn dense0 adam"]
    assert T.expected_route(by["K33_N16_J512"], fuse_switch=False) == ["iqn dense0 dgrad + wgrad", "iqn dense0 adam"]
    names = ["iqn hidden", "iqn dense0 fwd", "iqn dense0 dgrad + wgrad", "da3 finalize (sum, mask, planes)", "iqn dense0 adam", "conv2 wgrad"]
    assert T.dense0_launches(names) == ["iqn dense0 dgrad + wgrad", "iqn dense0 adam"]
    # the planner's model at nb > 1: the margin of each decision (a restated double comparison must not sit on a tie)
    for r in T.TABLE:
        if T.dims(r)[2] > 1 and T.dims(r)[3] % 16 == 0:
            fused, split = T.plan(r)["spans"]
            assert abs(fused - split) > 1e-3 * split, (r.id, fused, split)
    # the list scheduler on hand-made sequences
    assert T._makespan([0, 0, 1], 2.0, 2) == 3.0 and T._makespan([1, 1, 0, 0], 2.0, 2) == 3.0 and T._makespan([0] * 5, 9.0, 4) == 2.0
    assert T._seq(3, 1, 2, 1) == [0, 0, 1, 0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("rid", T.IDS)
def test_row_inputs_are_admissible_at_the_smallest_shift(rid):
    """At the row's seed shift: the fp64 oracle's q_sel top-two gap of step 0 exceeds A_STAR_GAP for every head and live sample, the
    fp32 oracle uses at most half of every bar and has the fp64 oracle's a* on every step; no smaller shift meets both."""
    row = T.BY_ID[rid]
    batch, taus = T.step_inputs(rid)
    assert batch[4][0] and batch[4][row.B - 1] and taus.shape == (row.K, 3, row.N, row.B)
    p, pt = T.params(rid)
    assert all(np.abs(a).max() > 0 for n, a in list(p.items()) + list(pt.items()) if n.endswith("bias"))
    gap = T.min_gap(rid)
    assert gap > T.A_STAR_GAP, gap
    # conditioned: no online pre-activation of any head within RELU_MARGIN of zero, at the fp64 oracle's parameters of every step
    from oracle import qnet_ref as Q

    o64 = T.oracle(rid)
    raw = T.raw_inputs(rid)
    assert np.array_equal(raw[0][3], batch[3]) and np.array_equal(raw[1][:, 1:], taus[:, 1:]), "only states and online fractions are replaced"
    same = [b for b in range(row.B) if np.array_equal(raw[0][0][b], batch[0][b])]
    assert sorted(set(range(row.B)) - set(same)) == sorted({b for _, b in o64["replaced"][0]})
    for k in range(row.K):
        assert T.min_preact(Q.head(p, k), batch[0], taus[k, 0]).min() >= T.RELU_MARGIN
    fig, same_a_star = T.fp32_shares(rid)
    pl = T.plan(row) if T.dims(row)[3] % 16 == 0 else {}
    print(rid, T.route(row), "per / QG / HG = %d / %d / %d" % T.groups(row), "items", pl.get("items", "-"), "shift", T.seed_shift(row),
          "gap %.3g" % gap, "samples replaced per step", [len(x) for x in o64["replaced"]], "fp32 oracle's shares of the bars:", {k: f"{v:.3g}" for k, v in fig.items()})
    assert same_a_star, "the fp32 oracle's a* differs from the fp64 oracle's"
    assert max(v for k, v in fig.items() if k not in ("mu", "nu")) <= T.HALF, fig
    if "mu" in fig:
        assert max(fig["mu"], fig["nu"]) <= T.MOMENT_FP32_DEV and 4 * T.MOMENT_FP32_DEV <= T.MOMENT_RTOL <= 1.1 * 4 * T.MOMENT_FP32_DEV, fig
    for s in range(T.seed_shift(row)):
        if T.min_gap(rid, s) > T.A_STAR_GAP:
            assert not T.admissible(rid, s), (s, "a smaller shift would do")
    if rid in T.CHAIN_IDS:
        for t in range(1, T.N_STEPS_CHAIN):  # a different batch and different fractions each
            b, tt = T.step_inputs(rid, t)
            assert not np.array_equal(b[0], batch[0]) and not np.array_equal(tt, taus) and b[4][0] and b[4][row.B - 1]
    T._oracle.cache_clear()  # (the records of the largest rows are hundreds of MB)


@pytest.mark.parametrize("rid", T.ACT_ROWS)
def test_acting_inputs(rid):
    """The acting check compares the action itself.  Two Q entries each within the Q bar of the oracle's cannot change order when they
    lie more than two bars apart: the oracle's top-two gap is at least 10 bars on every state (observed: 78 and more), and the fp32
    oracle uses at most half of the bar."""
    a64, a32 = T.acting_oracle(rid), T.acting_oracle(rid, "float32")
    share, gap = 0.0, np.inf
    for key, w in a64.items():
        scale = np.maximum(1.0, np.abs(w).max(axis=1))
        share = max(share, float((np.abs(a32[key] - w).max(axis=1) / scale).max() / T.ACT_Q_RTOL))
        gap = min(gap, float((T.top_gap(w) / scale).min()))
    print(rid, "fp32 oracle's share of the acting Q bar: %.3g, smallest top-two gap %.3g" % (share, gap))
    assert share <= T.HALF and gap >= 10 * T.ACT_Q_RTOL, (share, gap)
