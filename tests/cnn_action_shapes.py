"""The action-count table of the matrix-core cnn path's head kernels and of the i-IQN heads: one row per branch on ``A``.

Every kernel behind the conv trunk branches on the number of actions ``A`` (legal range 1 .. 32: ``cnn_fast_shape`` / ``build_layout``,
csrc/qnet.hip): ``td_dh_body`` (csrc/cnn_kernels.h) picks one of four ``q_reduce`` instances by ``NR = ceil(A / 8)``, stages W1 in four
rounds of 256 elements, folds the target maximum over two half-waves; ``k_hidden`` strides the actions by 8, the acting heads by 16, the
i-IQN kernels by 8 and by rounds of 256, the i-IQN acting heads take the actions as the rows of a 32 x 32 MFMA tile.  The other tables
(``FP_CASES``, the geometry table, ``conv_pp_shapes.py``) reach A = 3, 4, 5, 6, 18 only.  This one runs both sides of every step of those
branches on the smallest frame that keeps every layer, ``(20, 20, 4)``; tests/test_gpu_cnn_actions.py holds each row to the fp64 oracle,
tests/test_cnn_action_shapes_host.py checks on the CPU that the rows cover the classes named here and that the oracle's own fp32
restatement uses at most half of every bar.

The ROUTE of a row is not observable (``idqn_profile_read`` names ``k_dense0_wgrad`` for every cnn step): it follows from the number of
32-sample blocks ``nb`` and the conv mode as ``cnn_backward`` (csrc/qnet.hip) states it --

* nb = 1 (B <= 32), both modes: one workgroup per (chunk, head) loops over the blocks (``bb_only < 0``); ``k_td_dh`` in the bf16x3 mode,
  ``k_td_dh_wt`` in the f32 mode;
* nb >= 2, bf16x3: ``k_td_dh`` with one workgroup per (chunk, head, block), the last to arrive sums the blocks' partials (``TD_BPART``);
* nb >= 2, f32: ``k_td_dh_wt``, the loop form over nb blocks;
* nb >= 3, bf16x3 and J a multiple of 256: the many-block schedule behind it (the Dense_0 data gradient as its own launch).  At J = 128
  nb = 3 stays on the fused update, so the B = 70 row stands twice: at J = 128 as the per-block sum over three blocks, at J = 256 on
  the many-block schedule.
"""
import functools
from collections import namedtuple

import numpy as np

import cnn_stages as S
from fc_shapes import TD_ATOL, TD_RTOL  # noqa: F401  (|TD|: the bars of tests/test_gpu_fc_shapes.py)
from test_gpu_conv_geometry import (ADAM_ATOL, EPS, GAMMA, GAMMA_N, GAP_RTOL, LOSS_ATOL, LR, N_STEP, Q_RTOL,  # noqa: F401
                                    STAGE_BAR)

OBS = (20, 20, 4)
IQN_A_STAR_GAP = 1e-3  # check_iqn_step compares a* exactly: the oracle's q_sel top-two gap of head 0, relative to max(1, max |q_sel|)
MIN_ACTION_SHARE = 0.9  # of a row's states have a top-two gap that allows comparing the greedy action itself

Row = namedtuple("Row", "id A J K B N shift why")


def _r(id, A, why, J=128, K=2, B=33, N=0, shift=0):
    return Row(id, A, J, K, B, N, shift, why)


# ---- iDQN / DQN rows: features [32, 32, 32, J].  B = 33 is nb = 2 with one sample in the second block -------------------------------
IDQN = [
    _r("A1", 1, "NR = 1; half-wave 1 of the maximum folds nothing (-inf); one W1 round of 32 elements; argmax over one action"),
    _r("A2", 2, "NR = 1; each half-wave folds exactly one action"),
    _r("A7", 7, "NR = 1; odd fold (4 + 3); the 8-stride loops one action short of a full pass"),
    _r("A8", 8, "NR = 1 exactly full (256 elements): the last A of the first q_reduce instance; one full 8-stride pass"),
    _r("A9", 9, "NR = 2, first A: a second round of 32 elements; second 8-stride pass of one action"),
    _r("A15", 15, "NR = 2; odd fold; the 16-stride acting loop one action short of a full pass"),
    _r("A16", 16, "NR = 2 exactly full (512 elements); one full 16-stride pass, two full 8-stride passes"),
    _r("A17", 17, "NR = 3, first A; second 16-stride pass of one action; third 8-stride pass of one action"),
    _r("A24", 24, "NR = 3 exactly full (768 elements); three full 8-stride passes"),
    _r("A25", 25, "NR = 4, first A: the fourth round of W1 / q elements; fourth 8-stride pass of one action"),
    _r("A31", 31, "NR = 4; odd fold; every loop one action short of the largest legal pass"),
    _r("A32", 32, "NR = 4 exactly full: w1s[32 * 32] and TD_BPART's 1024 kernel slots are full; the largest legal A"),
    # further rows, each changing one thing
    _r("A32_J512", 32, "NJC = 16 chunk partials in q_reduce / k_q_out at the largest A", J=512),
    _r("A9_J512", 9, "NJC = 16 chunk partials at NR = 2", J=512),
    _r("A17_J384", 17, "NJC = 12 chunk partials at NR = 3", J=384),
    _r("A16_B20", 16, "nb = 1: the loop form (bb_only < 0) at NR = 2, ragged block", B=20),
    _r("A32_B20", 32, "nb = 1: the loop form (bb_only < 0) at NR = 4, ragged block", B=20),
    _r("A32_B70", 32, "nb = 3: the per-block sum over three blocks (J = 128: the fused update, see the module text)", B=70),
    _r("A32_B70_J256", 32, "nb = 3 and J % 256 == 0: the many-block schedule with the separate data gradient", B=70, J=256),
    _r("A32_K1", 32, "K = 1: the DQN agent, leaves without a head axis", K=1),
]
IDQN_BASE_A = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32)
GROUP_ROWS = ("A17", "A32")        # idqn_act_group_host over two members
REPLAY_ROWS = ("A32", "A9")        # idqn_learn_on_replay against gather-then-learn
TIE_PAIRS = ((0, -1), (7, 8), (15, 16), (16, 31))  # (lower, upper) index of the planted maximum; -1: A - 1

# ---- i-IQN rows: features [32, 32, 32, 256], K = 2, B = 33.  ``shift``: the smallest seed shift at which the oracle's q_sel top-two gap
# of head 0 exceeds IQN_A_STAR_GAP on every one of the first 32 samples AND the fp32 oracle stays within half of every bar
# (tests/test_cnn_action_shapes_host.py asserts both, and that no smaller shift does) ------------------------------------------------
IQN = [
    _r("iqn_A1", 1, "one action: a* is always 0, the 8-stride loops run once for one action", J=256, N=8),
    _r("iqn_A2", 2, "two actions", J=256, N=8),
    _r("iqn_A8", 8, "one full 8-stride pass; 256 elements: one full round", J=256, N=8, shift=2),
    _r("iqn_A9", 9, "second 8-stride pass of one action; second round of 32 elements", J=256, N=8),
    _r("iqn_A16", 16, "two full passes; rows 0 .. 15 of the acting MFMA tile", J=256, N=8, shift=1),
    _r("iqn_A17", 17, "third pass of one action; row 16 of the tile: the first of its second half", J=256, N=8, shift=2),
    _r("iqn_A31", 31, "one action short of the full tile", J=256, N=8),
    _r("iqn_A32", 32, "every row of the 32 x 32 tile, four full rounds", J=256, N=8),
    # (shift 0 has the gap, and a near-tie of a* on head 1 that the fp32 oracle resolves the other way: gradients off by 95 bars)
    _r("iqn_A32_N32", 32, "the largest A at 32 fractions", J=256, N=32, shift=2),
    _r("iqn_A17_N1", 17, "one fraction: |TD| for N = 1, the mean over one value", J=256, N=1),
]
IQN_BASE_A = (1, 2, 8, 9, 16, 17, 31, 32)
TABLE = IDQN + IQN
BY_ID = {r.id: r for r in TABLE}
assert len(BY_ID) == len(TABLE)


def feats_of(row):
    return [32, 32, 32, row.J]


def top_gap(q):
    """Gap between the largest and the second largest entry along the last axis; +inf where there is one action only."""
    q = np.asarray(q, np.float64)
    if q.shape[-1] < 2:
        return np.full(q.shape[:-1], np.inf)
    top = np.sort(q, axis=-1)
    return top[..., -1] - top[..., -2]


def comparable(q):
    """Where the greedy action itself is compared: the oracle's top-two gap exceeds GAP_RTOL * max(1, max |q|) of the row."""
    q = np.asarray(q, np.float64)
    return top_gap(q) > GAP_RTOL * np.maximum(1.0, np.abs(q).max(axis=-1))


def check_actions(acts, rows, want, failures, what):
    """``acts`` [n] and Q rows ``rows`` [n, A] of an acting entry against the oracle's ``want`` [n, A]: the Q row always (Q_RTOL of
    max(1, max |want|)), the action where ``comparable``.  Returns (largest Q error relative to its scale, number compared by action)."""
    want = np.asarray(want, np.float64)
    rows = np.asarray(rows, np.float64).reshape(want.shape)
    acts = np.asarray(acts).reshape(-1)
    ok = comparable(want)
    worst = 0.0
    for e in range(want.shape[0]):
        scale = max(1.0, float(np.abs(want[e]).max()))
        err = float(np.abs(rows[e] - want[e]).max()) / scale
        worst = max(worst, err)
        if not err <= Q_RTOL:
            failures.append((what + " q row", e, err))
        if ok[e] and int(acts[e]) != int(np.argmax(want[e])):
            failures.append((what + " action", e, int(acts[e]), int(np.argmax(want[e]))))
    return worst, int(ok.sum())


def tie_biases(A):
    """[(bias [A], expected action)] of part (g): the maximum planted twice, the lower index must win; A = 1: action 0."""
    out = []
    for lo, hi in TIE_PAIRS:
        hi = A - 1 if hi < 0 else hi
        if hi >= A or lo > hi:
            continue
        bias = np.full(A, -1.0, np.float32)
        bias[[lo, hi]] = 0.5
        out.append((bias, lo))
    return out


def target_bump_indices(A):
    """The actions j of part (f): 0, A - 2, A - 1 where they exist."""
    return sorted({j for j in (0, A - 2, A - 1) if 0 <= j < A})


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _actions(a, A, B):
    """The batch holds action A - 1 (first sample) and action 0 (last sample); for A >= 16 action A // 2 is absent (its samples take
    A // 2 - 1), so that an all-zero column of the Dense_1 gradient is compared too."""
    a = np.asarray(a, np.int32).copy()
    if A >= 16:
        a[a == A // 2] = A // 2 - 1
    a[0] = A - 1
    a[B - 1] = 0
    return a


@functools.lru_cache(maxsize=None)
def idqn_inputs(rid):
    """(p, pt, batch, weights): seeds 3 / 4 / 5 / 6 as tests/test_gpu_conv_geometry.py builds them (+ 10 * shift), the actions as
    ``_actions`` places them."""
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    feats, s = feats_of(row), 10 * row.shift
    p = Q.init_params(3 + s, "cnn", OBS, row.A, feats, row.K)
    pt = Q.init_params(4 + s, "cnn", OBS, row.A, feats, row.K)
    rng = np.random.default_rng(5 + s)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(6 + s, row.B, OBS, row.A, "cnn")
    term = term.copy()
    term[row.B // 2] = True
    w = np.random.default_rng(9).uniform(0.05, 1.0, row.B).astype(np.float32)
    return p, pt, (st, _actions(a, row.A, row.B), r, s2, term), w


def bumped_target(pt, j):
    """The target parameters with +5 on Dense_1/bias[j] of every head: action j becomes the target maximum of every sample."""
    out = {n: v.copy() for n, v in pt.items()}
    out["Dense_1/bias"][:, j] += 5.0
    return out


def idqn_oracle(rid, dtype=np.float64):
    return _idqn_oracle(rid, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _idqn_oracle(rid, dtype_name):
    """Everything the oracle says about an iDQN row in ``dtype``: per head (loss, grads, aux) plain and weighted, the parameters after
    one Adam step from a zero state, and per bumped target action (loss, |TD|) of every head."""
    from oracle import qnet_ref as Q

    dtype = np.float64 if dtype_name == "float64" else np.float32
    row = BY_ID[rid]
    p, pt, batch, w = idqn_inputs(rid)
    K = row.K
    plain = [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N, dtype) for k in range(K)]
    weighted = [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N, dtype, weights=w) for k in range(K)]
    adam = {n: np.stack([Q.adam_update(p[n][k].astype(dtype), plain[k][1][n].astype(dtype), dtype(0), dtype(0), 0, LR, EPS, dtype)[0]
                         for k in range(K)]) for n in p}
    bumped = {}
    for j in target_bump_indices(row.A):
        ptj = bumped_target(pt, j)
        # (the online side does not change: only the target and what follows from it is recomputed)
        res = []
        for k in range(K):
            q_next = Q.forward(Q.head(ptj, k), batch[3], "cnn", dtype)
            tgt = Q.td_target(q_next, batch[2], batch[4], GAMMA_N, dtype)
            td = plain[k][2]["q"][np.arange(row.B), batch[1]] - tgt
            res.append(((td * td).mean(), np.abs(td)))
        bumped[j] = res
    return dict(plain=plain, weighted=weighted, adam=adam, bumped=bumped)


def iqn_hyper():
    from oracle import make_golden as G

    return G.FP_HYPER


@functools.lru_cache(maxsize=None)
def iqn_inputs(rid, shift=None):
    """(p, pt, batch, taus, act_taus [32, N]) of an i-IQN row, built as tests/test_gpu_conv_geometry.py builds its i-IQN leg (seeds
    3 / 4 / 5 / 6 / 7, + 10 * shift) with the actions of ``_actions``."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    feats, s = feats_of(row), 10 * (row.shift if shift is None else shift)
    p = I.init_params(3 + s, OBS, row.A, feats, row.K)
    pt = I.init_params(4 + s, OBS, row.A, feats, row.K)
    rng = np.random.default_rng(5 + s)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    st, a, r, s2, term = Q.synthetic_batch(6 + s, row.B, OBS, row.A, "cnn")
    term = term.copy()
    term[row.B // 2] = True
    taus = I.synthetic_taus(7 + s, row.K, row.N, row.B)
    act_taus = np.random.default_rng(8 + s).random((32, row.N)).astype(np.float32)
    return p, pt, (st, _actions(a, row.A, row.B), r, s2, term), taus, act_taus


def iqn_a_star_gap(rid, shift=None, dtype=np.float64):
    """Smallest top-two gap of the oracle's q_sel of head 0 over the first 32 samples, relative to max(1, max |q_sel|)."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    p, pt, batch, taus, _ = iqn_inputs(rid, shift)
    n = min(32, batch[0].shape[0])
    psi_t = I.trunk(Q.head(pt, 0), batch[3][:n], dtype)
    q_sel = I.quantile_values(Q.head(pt, 0), psi_t, taus[0][1][:, :n], dtype).mean(0)
    return float(top_gap(q_sel).min() / max(1.0, float(np.abs(q_sel).max())))


@functools.lru_cache(maxsize=None)
def iqn_record(rid, shift=None):
    """cnn_stages.iqn_record of the row (fp64): what check_iqn_step compares against."""
    p, pt, batch, taus, _ = iqn_inputs(rid, shift)
    return S.iqn_record(p, pt, batch, taus, iqn_hyper())


@functools.lru_cache(maxsize=None)
def iqn_acting_oracle(rid, dtype_name="float64"):
    """{(which, head): Q rows [n, A]} of ``iqn_ref.greedy_action`` for the first min(B, 32) states with fraction row e of ``act_taus``."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    dtype = np.float64 if dtype_name == "float64" else np.float32
    row = BY_ID[rid]
    p, pt, batch, _, act_taus = iqn_inputs(rid)
    n = min(row.B, 32)
    out = {}
    for which, params in ((0, p), (1, pt)):
        for k in range(row.K):
            out[(which, k)] = np.stack([I.greedy_action(Q.head(params, k), batch[0][e], act_taus[e], dtype)[1] for e in range(n)])
    return out


@functools.lru_cache(maxsize=None)
def iqn_step_fp32(rid, shift=None):
    """The quantities of ``cnn_stages.iqn_record`` restated in numpy fp32 (the host test's half-bar rule): losses, head 0's z_a, z_t and
    q_sel, every leaf's gradient and its parameters after the Adam step."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    p, pt, batch, taus, _ = iqn_inputs(rid, shift)
    hy = iqn_hyper()
    gamma_n = hy["gamma"] ** hy["n"]
    zeros = {n: np.zeros(a.shape, np.float32) for n, a in p.items()}
    _, _, aux0 = I.loss_and_grads(Q.head(p, 0), Q.head(pt, 0), batch, tuple(taus[0]), gamma_n, np.float32)
    p32, _, _, _, losses, grads = I.learn_on_batch(p, pt, zeros, zeros, np.zeros(row.K, np.int64), batch, taus, gamma_n, hy["lr"],
                                                   hy["eps"], np.float32, return_grads=True)
    return dict(losses=losses, z_online_head0=aux0["z_a"], z_target_head0=aux0["z_t"], q_select_head0=aux0["q_sel"],
                a_star_head0=aux0["a_star"], grads=grads, params=p32)
