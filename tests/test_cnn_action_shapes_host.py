"""CPU side of the action-count table (tests/cnn_action_shapes.py): what the table covers is asserted from its rows, the inputs meet the
requirements the GPU test relies on, and the oracle's own numpy-fp32 restatement stays within HALF of every bar the GPU test applies
(a bar the fp32 oracle alone half uses leaves the kernel the other half).  A row that breaks the half rule gets a seed shift,
never a wider bar.  Figures are printed (``-s``); none of them sets a bar.
"""
import math

import numpy as np
import pytest

import cnn_action_shapes as T
import cnn_stages as S

IDQN_IDS = [r.id for r in T.IDQN]
IQN_IDS = [r.id for r in T.IQN]
HALF = 0.5


def _base(rows, **kw):
    return [r for r in rows if all(getattr(r, k) == v for k, v in kw.items())]


def test_table_covers_every_class():
    base = _base(T.IDQN, J=128, K=2, B=33)
    assert tuple(sorted(r.A for r in base)) == T.IDQN_BASE_A == (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32)
    for nr in (1, 2, 3, 4):  # both ends of every q_reduce instance
        inside = [r.A for r in base if math.ceil(r.A / 8) == nr]
        assert 8 * nr in inside and min(inside) == 8 * (nr - 1) + 1, (nr, inside)
    assert {r.A % 2 for r in base} == {0, 1}                                # odd and even half-wave folding
    assert {math.ceil(r.A / 16) for r in base} == {1, 2} and {15, 16, 17} <= {r.A for r in base}  # the 16-stride loops
    have = {(r.A, r.J, r.K, r.B) for r in T.IDQN}
    for want in ((32, 512, 2, 33), (9, 512, 2, 33), (17, 384, 2, 33), (16, 128, 2, 20), (32, 128, 2, 20), (32, 128, 2, 70),
                 (32, 256, 2, 70), (32, 128, 1, 33)):
        assert want in have, want
    assert all(r.N == 0 and r.shift == 0 for r in T.IDQN)
    iqn = _base(T.IQN, J=256, K=2, B=33, N=8)
    assert tuple(sorted(r.A for r in iqn)) == T.IQN_BASE_A == (1, 2, 8, 9, 16, 17, 31, 32)
    assert {(r.A, r.N) for r in T.IQN} >= {(32, 32), (17, 1)} and all(r.J == 256 and r.K == 2 and r.B == 33 for r in T.IQN)
    assert all(r.why for r in T.TABLE) and len({r.why for r in T.TABLE}) == len(T.TABLE), "one reason per row"
    assert all(1 <= r.A <= 32 for r in T.TABLE)
    assert {T.BY_ID[i].A for i in T.GROUP_ROWS} == {17, 32} and {T.BY_ID[i].A for i in T.REPLAY_ROWS} == {32, 9}
    # the planted ties: every pair exists at A = 32, (0, A - 1) everywhere, and the lower index is the expected action
    assert [int(a) for _, a in T.tie_biases(32)] == [0, 7, 15, 16]
    assert [int(a) for _, a in T.tie_biases(17)] == [0, 7, 15] and [int(a) for _, a in T.tie_biases(9)] == [0, 7]
    assert [int(a) for _, a in T.tie_biases(1)] == [0] and [int(a) for _, a in T.tie_biases(2)] == [0]
    for A in (1, 2, 9, 17, 32):
        for bias, want in T.tie_biases(A):
            assert bias.shape == (A,) and int(np.argmax(bias)) == want and (bias == bias.max()).sum() == min(A, 2)
    assert T.target_bump_indices(1) == [0] and T.target_bump_indices(2) == [0, 1] and T.target_bump_indices(32) == [0, 30, 31]


@pytest.mark.parametrize("rid", IDQN_IDS + IQN_IDS)
def test_batch_holds_both_ends_of_the_action_range(rid):
    row = T.BY_ID[rid]
    batch = (T.idqn_inputs if row.N == 0 else T.iqn_inputs)(rid)[2]
    a = batch[1]
    assert a.shape == (row.B,) and a.dtype == np.int32 and a.min() == 0 and a.max() == row.A - 1
    assert 0 in a and row.A - 1 in a
    if row.A >= 16:
        assert set(range(row.A)) - set(a.tolist()), "an action index must be absent: its gradient column is all zero"
    assert batch[4][row.B // 2] and not batch[4].all()


def _rel(got, want):
    return S.relerr(np.asarray(got, np.float64), np.asarray(want, np.float64))


@pytest.mark.parametrize("rid", IDQN_IDS)
def test_fp32_oracle_uses_at_most_half_of_every_idqn_bar(rid):
    row = T.BY_ID[rid]
    p, pt, batch, w = T.idqn_inputs(rid)
    o64, o32 = T.idqn_oracle(rid), T.idqn_oracle(rid, np.float32)
    fig = dict(loss=0.0, stage=0.0, wloss=0.0, wgrad=0.0, td=0.0, adam=0.0, q=0.0, bump_loss=0.0, bump_td=0.0)
    for k in range(row.K):
        for what, lk, gk in (("plain", "loss", "stage"), ("weighted", "wloss", "wgrad")):
            l64, g64, a64 = o64[what][k]
            l32, g32, a32 = o32[what][k]
            fig[lk] = max(fig[lk], abs(float(l32) - l64))
            for leaf in g64:
                fig[gk] = max(fig[gk], _rel(g32[leaf], g64[leaf]))
        a64, a32 = o64["plain"][k][2], o32["plain"][k][2]
        for key in ("q", "q_next"):
            fig["stage"] = max(fig["stage"], _rel(a32[key], a64[key]))
            fig["q"] = max(fig["q"], float(np.abs(a32[key] - a64[key]).max() / max(1.0, np.abs(a64[key]).max())))
        fig["stage"] = max(fig["stage"], _rel(a32["trace"]["d_dense0"], a64["trace"]["d_dense0"]))
        td64, td32 = np.abs(o64["weighted"][k][2]["td"]), np.abs(o32["weighted"][k][2]["td"])
        fig["td"] = max(fig["td"], float((np.abs(td32 - td64) / (T.TD_ATOL + T.TD_RTOL * td64)).max()))  # share of the |TD| bar
        for j, res in o64["bumped"].items():
            # (a bumped loss is ~20, where one fp32 ulp is 1.9e-6: its bar is LOSS_ATOL relative to max(1, |loss|), the form of
            # tests/test_gpu_general_shapes.py and check_iqn_step; leaving action j out misses it by (5 gamma^n)^2 ~ 20)
            fig["bump_loss"] = max(fig["bump_loss"], abs(float(o32["bumped"][j][k][0]) - res[k][0]) / max(1.0, res[k][0]))
            fig["bump_td"] = max(fig["bump_td"], float((np.abs(o32["bumped"][j][k][1] - res[k][1]) / (T.TD_ATOL + T.TD_RTOL * res[k][1])).max()))
            # the point of the bump: action j is the target maximum of every non-terminal sample, and leaving it out moves the loss
            assert res[k][0] > o64["plain"][k][0] + 1.0, (j, k, res[k][0], o64["plain"][k][0])
    for leaf in o64["adam"]:
        fig["adam"] = max(fig["adam"], float(np.abs(o32["adam"][leaf] - o64["adam"][leaf]).max()))
    print(rid, {k: f"{v:.3g}" for k, v in fig.items()})
    assert fig["loss"] <= HALF * T.LOSS_ATOL and fig["wloss"] <= HALF * T.LOSS_ATOL and fig["bump_loss"] <= HALF * T.LOSS_ATOL, fig
    assert fig["stage"] <= HALF * T.STAGE_BAR and fig["wgrad"] <= HALF * T.STAGE_BAR, fig
    assert fig["td"] <= HALF and fig["bump_td"] <= HALF, fig
    assert fig["adam"] <= HALF * T.ADAM_ATOL and fig["q"] <= HALF * T.Q_RTOL, fig


@pytest.mark.parametrize("rid", IDQN_IDS)
def test_most_idqn_states_are_compared_by_action(rid):
    row = T.BY_ID[rid]
    heads = T.idqn_oracle(rid)["plain"]
    n = min(row.B, 32)
    for k in range(row.K):
        share = float(T.comparable(heads[k][2]["q"][:n]).mean())
        assert share >= T.MIN_ACTION_SHARE, (k, share)
    many = np.stack([heads[e % row.K][2]["q"][e] for e in range(n)])
    assert T.comparable(many).mean() >= T.MIN_ACTION_SHARE
    if row.A == 1:
        assert T.comparable(many).all()


def _iqn_step_shares(rid, shift=None):
    """The fp32 oracle's deviation from the fp64 record as shares of the bars of cnn_stages.check_iqn_step: loss 1e-5 of max(1, |loss|),
    quantile values 2e-5 of max(1, max |z|), gradients 3e-5 of the leaf's largest entry, parameters 0.02 lr + 2e-7 |p| where the
    gradient is not negligible."""
    row = T.BY_ID[rid]
    rec, f32 = T.iqn_record(rid, shift), T.iqn_step_fp32(rid, shift)
    lr = rec["hyper"]["lr"]
    want = np.asarray(rec["losses"])
    fig = dict(loss=float(np.abs(f32["losses"] - want).max() / max(1.0, np.abs(want).max()) / 1e-5), z=0.0, grad=0.0, param=0.0)
    for key in ("z_online_head0", "z_target_head0", "q_select_head0"):
        w = np.asarray(rec[key])
        fig["z"] = max(fig["z"], float(np.abs(f32[key] - w).max() / max(1.0, np.abs(w).max()) / 2e-5))
    for leaf, r in rec["leaves"].items():
        wg, scale, wp = np.asarray(r["grad"]), np.asarray(r["grad_absmax"])[:, None], np.asarray(r["param"])
        g = f32["grads"][leaf].reshape(row.K, -1)
        fig["grad"] = max(fig["grad"], float((np.abs(g - wg) / (3e-5 * scale + 1e-12)).max()))
        big = np.abs(wg) > 1e-3 * scale
        err = np.abs(f32["params"][leaf].reshape(row.K, -1) - wp)
        fig["param"] = max(fig["param"], float((err[big] / (0.02 * lr + 2e-7 * np.abs(wp[big]))).max()))
    return fig


@pytest.mark.parametrize("rid", IQN_IDS)
def test_iqn_seed_shift_is_the_smallest_with_an_exact_a_star(rid):
    """check_iqn_step asserts a* EQUAL: it holds because the oracle's q_sel top-two gap of head 0 exceeds IQN_A_STAR_GAP on every one
    of the first 32 samples at the row's seed shift.  No smaller shift has that gap AND keeps the fp32 oracle within half of the bars."""
    row = T.BY_ID[rid]
    assert T.iqn_a_star_gap(rid) > T.IQN_A_STAR_GAP, T.iqn_a_star_gap(rid)
    for s in range(row.shift):
        gap = T.iqn_a_star_gap(rid, s)
        assert not (gap > T.IQN_A_STAR_GAP and max(_iqn_step_shares(rid, s).values()) <= HALF), (s, "a smaller shift would do")
    rec, f32 = T.iqn_record(rid), T.iqn_step_fp32(rid)
    n = min(row.B, 32)
    assert np.array_equal(np.asarray(f32["a_star_head0"])[:n], np.asarray(rec["a_star_head0"])[:n])


@pytest.mark.parametrize("rid", IQN_IDS)
def test_fp32_oracle_uses_at_most_half_of_every_iqn_bar(rid):
    """The bars of cnn_stages.check_iqn_step and Q_RTOL for the acting rows, each halved."""
    fig = _iqn_step_shares(rid)
    fig["q"] = 0.0
    a64, a32 = T.iqn_acting_oracle(rid), T.iqn_acting_oracle(rid, "float32")
    share = 1.0
    for key, w in a64.items():
        fig["q"] = max(fig["q"], float((np.abs(a32[key] - w).max(axis=1) / np.maximum(1.0, np.abs(w).max(axis=1))).max() / T.Q_RTOL))
        share = min(share, float(T.comparable(w).mean()))
    print(rid, "shares of the bars:", {k: f"{v:.3g}" for k, v in fig.items()}, f"compared by action: {share:.2f}")
    assert max(fig.values()) <= HALF, fig
    assert share >= T.MIN_ACTION_SHARE, share


def test_helpers_at_one_and_at_thirty_two_actions():
    """top_gap / comparable / check_actions on numpy stand-ins: A = 1 has no second-largest value and must still compare."""
    one = np.array([[0.3], [-2.0]])
    assert np.isinf(T.top_gap(one)).all() and T.comparable(one).all()
    failures = []
    worst, n = T.check_actions([0, 0], one.astype(np.float32), one, failures, "A1")
    assert not failures and n == 2 and worst <= 1e-7
    T.check_actions([1, 0], one, one, failures, "A1")
    assert failures == [("A1 action", 0, 1, 0)]
    rng = np.random.default_rng(0)
    q = rng.standard_normal((5, 32))
    q[3, 7] = q[3].max() + 0.5e-4                      # a gap below GAP_RTOL: compared by its Q row only
    q[4] *= 1e3
    q[4, 9] = q[4].max() + 0.05                        # ... and relative to max |q| where that exceeds 1
    ok = T.comparable(q)
    assert ok.tolist() == [True, True, True, False, False]
    assert np.allclose(T.top_gap(q), [np.sort(r)[-1] - np.sort(r)[-2] for r in q])
    failures = []
    acts = np.argmax(q, axis=1)
    acts[3] = 0                                         # inside the gap: not a failure
    worst, n = T.check_actions(acts, q, q, failures, "A32")
    assert not failures and n == 3 and worst == 0.0
    bad = q.copy()
    bad[1, 31] += 2e-5 * max(1.0, np.abs(q[1]).max())   # the last action's value off by more than Q_RTOL
    acts[0] = (acts[0] + 1) % 32
    T.check_actions(acts, bad, q, failures, "A32")
    assert [f[:2] for f in failures] == [("A32 action", 0), ("A32 q row", 1)]
    assert T._actions(np.zeros(33, np.int32), 1, 33).tolist() == [0] * 33
    a = T._actions(np.full(33, 16, np.int32), 32, 33)
    assert a[0] == 31 and a[32] == 0 and 16 not in a and (a[1:32] == 15).all()


def test_iqn_with_33_actions_is_refused_by_the_layout():
    """The quantile heads exist on the matrix-core path only: A = 33 is refused with the library's message (no GPU needed: idqn_layout)."""
    from slimdqn import _hip

    cfg = _hip.make_config("cnn", 2, 33, T.OBS, [32, 32, 32, 256], 32, 1e-3, 1e-6, 0.99, n_quantiles=8)
    with pytest.raises(_hip.HipExtensionError, match="n_actions <= 32"):
        _hip.layout(cfg)
    cfg = _hip.make_config("cnn", 2, 33, (84, 84, 4), [32, 64, 64, 512], 32, 1e-3, 1e-6, 0.99)
    leaves, _ = _hip.layout(cfg)  # without quantile heads the same A is the general-shape layout: accepted
    assert [n for n, _, _ in leaves][-1] == "Dense_1/bias" and leaves[-1][2] == (33,)
