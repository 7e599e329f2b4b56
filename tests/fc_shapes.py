"""The shape table of the one-launch MLP step (``k_fc_step_par``, csrc/fc_par_kernels.h + csrc/fc_par_phases.h) and a
Python restatement of the two LDS plans that decide which nets run it.

The restatement (``par_plan`` = ``fc_par_plan``, ``steps_plan`` = ``fc_steps_plan``, ``layout`` = the fc branch of
``build_layout`` in csrc/qnet.hip, ``mfma_plan`` / ``mfma_plan_g`` = the two fallback plans of csrc/fc_kernels.h) only BUILDS
the table and says which route a row expects.  tests/test_fc_shapes_host.py ties its constants to the headers' text and checks
every row's stated reason; tests/test_gpu_fc_shapes.py never trusts it: the route is asserted through ``idqn_profile_read``,
which names the kernel a step launched.

Two of the limits have no ordinary row:

* ``P % 4 != 0`` has no row at all, because no shape reaches it: ``add_leaf`` (csrc/qnet.hip) starts every leaf on a 256-byte
  boundary, so a head's arena ``P`` is always a multiple of 64 floats and ``fc_par_plan``'s ``P % 4 == 0`` cannot fail through
  ``idqn_create`` (tests/test_fc_shapes_host.py holds that against the library's own ``idqn_layout``).
* ``features = []`` (no hidden layer) is a REFUSAL row: the reference's ``DQNNet`` accepts it (its loop over the features is
  empty and ``Dense(n_actions)`` reads the observation), ``build_layout`` answers ``REFUSAL_NO_HIDDEN``.  The GPU test requires
  exactly that message of the create, so the day the library takes the shape the row has to become an inside row.
"""
import functools
from collections import namedtuple

import numpy as np

# ---- the constants the plans are built from; tests/test_fc_shapes_host.py reads the headers and fails if these differ ----------------
FCP_NPT = 24                       # csrc/fc_par_kernels.h
FCP_LDS_BUDGET = 160 * 1024 - 256  # csrc/fc_par_kernels.h
FCM_T = 512                        # csrc/fc_kernels.h
FCM_BSP = 33                       # csrc/fc_kernels.h
FCS_ROW_WORDS = 32 * 8             # csrc/fc_steps_kernels.h
FC_MAX_WIDTH = 512                 # csrc/fc_kernels.h
FC_LDS_BUDGET = 150 * 1024         # csrc/fc_kernels.h (the fallbacks' budget: only the expected fallback's NAME depends on it)
P_MAX = 512 * FCP_NPT              # 12,288 arena floats per head

Plan = namedtuple("Plan", "ok floats drows act_row buf_off wo_off wt_off misc_off why")


def dims(d0, feats, A):
    return [int(d0)] + [int(f) for f in feats] + [int(A)]


def layout(d0, feats, A):
    """(w_off[], b_off[], P): every leaf padded to a multiple of 64 floats (add_leaf, csrc/qnet.hip)."""
    d, off, w_off, b_off = dims(d0, feats, A), 0, [], []
    for din, dout in zip(d[:-1], d[1:]):
        w_off.append(off)
        off += (din * dout + 63) // 64 * 64
        b_off.append(off)
        off += (dout + 63) // 64 * 64
    return w_off, b_off, off


def par_plan(d0, feats, A):
    """fc_par_plan, statement for statement; ``why`` lists the conditions that failed (empty: the net fits)."""
    d = dims(d0, feats, A)
    P = layout(d0, feats, A)[2]
    why = []
    if P > 512 * FCP_NPT:
        why.append("P > 12288")
    if P % 4:
        why.append("P % 4")
    act_row, rows = [], 0
    for w in d:
        act_row.append(rows)
        rows += w
    if max(d) > 128:
        why.append("width > 128")
    if 32 * d[0] > 8 * FCM_T:
        why.append("d0 > 128")
    drows = (max(d) + 31) // 32 * 32
    buf_off = rows * FCM_BSP
    off = buf_off + 2 * drows * FCM_BSP + 32 * FCM_BSP
    off = (off + 3) & ~3
    wo_off = off
    off += P + 32
    wt_off = off
    off += P + 32
    misc_off = off
    floats = off + 128
    if floats * 4 > FCP_LDS_BUDGET:
        why.append("LDS")
    if max(d) > FC_MAX_WIDTH:  # (fc_setup clears the plan for the generic kernel's widths)
        why.append("width > FC_MAX_WIDTH")
    return Plan(not why, floats, drows, act_row, buf_off, wo_off, wt_off, misc_off, why)


def steps_plan(d0, feats, A):
    """fc_steps_plan: fc_par_plan plus the 32 element rows of the next step's minibatch behind its last block."""
    p = par_plan(d0, feats, A)
    floats = p.misc_off + 128 + FCS_ROW_WORDS
    why = list(p.why) + (["LDS (steps)"] if p.ok and floats * 4 > FCP_LDS_BUDGET else [])
    return p._replace(ok=not why, floats=floats, why=why)


def mfma_plan(d0, feats, A):
    """fc_mfma_plan: LDS floats of k_fc_step_mfma<false> (0: the weight matrix does not fit beside the activations)."""
    d = dims(d0, feats, A)
    dinmax, doutmax, dmax, L = max(d[:-1]), max(d[1:]), max(d), len(d) - 1
    ldw = (doutmax + 31) // 32 * 32 + 1
    drows = (dmax + 31) // 32 * 32
    floats = (dinmax + 1) * ldw + (L + 1) * dmax * FCM_BSP + 2 * drows * FCM_BSP + 32 * FCM_BSP + 96
    return 0 if floats * 4 > FC_LDS_BUDGET or dmax > FC_MAX_WIDTH else floats


def mfma_plan_g(d0, feats, A):
    d = dims(d0, feats, A)
    drows = (max(d) + 31) // 32 * 32
    floats = sum(d) * FCM_BSP + 2 * drows * FCM_BSP + 32 * FCM_BSP + 96
    return 0 if floats * 4 > FC_LDS_BUDGET or max(d) > FC_MAX_WIDTH else floats


def expected_route(d0, feats, A, B):
    """The kernel ``idqn_learn_on_batch`` launches for this net and batch, as the restatement sees it (the rows of the table
    only ever fall to k_fc_step_par or the MFMA two-launch step; anything else answers None and the host test refuses the row)."""
    if par_plan(d0, feats, A).ok and B <= 32:
        return "k_fc_step_par"
    if mfma_plan(d0, feats, A):
        return "k_fc_step_mfma<lds>"
    if mfma_plan_g(d0, feats, A):
        return "k_fc_step_mfma<global>"
    return None


# ---- the table -----------------------------------------------------------------------------------------------------------------------
# One stated reason per row: one limit and one side of it.  ``claim`` names the check tests/test_fc_shapes_host.py makes about the
# row on the restatement (a key of its CLAIMS), ``route`` is the kernel name the GPU test requires of idqn_profile_read (None: the
# create is refused with REFUSAL_NO_HIDDEN).  K <= 3 except where K is the point.
Row = namedtuple("Row", "id d0 feats A K B route claim why eps seed")
PAR = "k_fc_step_par"
REFUSAL_NO_HIDDEN = "n_features out of range"


def _r(id, d0, feats, A, K, B, claim, why, route=PAR, eps=1e-6, seed=0):
    return Row(id, d0, list(feats), A, K, B, route, claim, why, eps, seed)


INSIDE = [
    _r("L2_lunar", 8, [100], 4, 2, 32, "layers=2", "one hidden layer; the full batch of 32"),
    _r("L3_lunar", 8, [100, 100], 4, 3, 32, "layers=3", "two hidden layers: the LunarLander net (P = 11,648)"),
    _r("L4", 6, [24, 40, 16], 3, 2, 9, "layers=4", "three hidden layers; every sample terminal"),
    _r("L5", 5, [12, 20, 28, 36], 5, 2, 13, "layers=5", "four hidden layers"),
    _r("w1_hidden", 4, [1, 6], 2, 2, 5, "hidden=1", "hidden width 1: a one-column tile, then din = 1 (one masked MFMA step)"),
    _r("A1", 7, [10], 1, 2, 6, "A=1", "A = 1: max and argmax over one action, a one-column tile at the Q head"),
    _r("w31", 9, [31], 31, 2, 11, "hidden=A=31", "31 as hidden width and as A: one ragged column tile"),
    _r("w32", 8, [32], 32, 2, 8, "hidden=A=32", "32 as hidden width and as A: one full tile, the two nets on different waves"),
    _r("w33", 8, [33], 33, 2, 10, "hidden=A=33", "33 as hidden width and as A: a second tile of one column, 33 delta rows"),
    _r("w64", 6, [64], 64, 2, 12, "hidden=A=64", "64 as hidden width and as A: two full tiles"),
    _r("w65", 6, [65], 65, 2, 12, "hidden=A=65", "65 as hidden width and as A: a third tile of one column"),
    _r("w96", 4, [96], 96, 1, 16, "hidden=A=96", "96 as hidden width and as A: three full tiles, the fourth wave idle"),
    _r("w97", 4, [97], 97, 1, 16, "hidden=A=97", "97 as hidden width and as A: a fourth tile of one column"),
    _r("w127_hidden", 3, [127], 5, 2, 20, "hidden=127", "127 as a hidden width: the fourth tile one column short"),
    _r("A127", 2, [64], 127, 2, 20, "A=127", "A = 127 (127 x 127 alone exceeds 12,288 floats, so hidden and A take a row each)"),
    _r("w128_hidden", 12, [128], 6, 2, 17, "hidden=128", "128 as a hidden width: four full tiles"),
    _r("A128", 2, [64], 128, 2, 32, "A=128", "A = 128: four full tiles at the Q head, the widest delta buffer"),
    _r("odd_din_all", 5, [7, 9], 3, 2, 32, "din odd everywhere", "odd din at every layer position (5, 7, 9)"),
    _r("even_din_all", 8, [16, 34], 4, 2, 15, "din even everywhere", "even din at every layer position (8, 16, 34)"),
    _r("d0_1", 1, [16], 3, 2, 9, "d0=1", "d0 = 1: a single input row"),
    _r("d0_127", 127, [20], 3, 2, 32, "d0=127", "d0 = 127: the minibatch ends 32 elements short of 8 per thread"),
    _r("d0_128", 128, [24], 4, 2, 32, "d0=128", "d0 = 128: the minibatch is exactly 8 elements per thread"),
    _r("B1", 8, [50], 4, 2, 1, "B=1", "B = 1: 31 pad rows"),
    # (seed 7: with rewards of 1e-3 and 10 the loss is ~50, ulp 3.8e-6; of eight seeds tried on the fp32 oracle -- 0.82, 0.54, 0.66, 0.61,
    # 0.75, 0.93, 0.56, 0.43 of LOSS_ATOL -- this is the one that leaves the kernel half of the bar)
    _r("B2", 8, [50], 4, 2, 2, "B=2", "B = 2: 30 pad rows", seed=7),
    _r("B31", 8, [50], 4, 2, 31, "B=31", "B = 31: one pad row"),
    _r("P_above_8192", 40, [100, 48], 8, 1, 19, "8192<P<=10240", "P = 9,472: five of a thread's six float4 slots live, the sixth past P"),
    _r("P_mult_2048", 4, [56, 120], 8, 2, 21, "P%2048==0", "P = 8,192: a multiple of 2048, the tail test never cuts a slot short"),
    _r("P_largest", 4, [40, 96, 80], 2, 1, 32, "P=12288", "P = 12,288 = 512 x FCP_NPT: the largest arena, every slot of every thread live"),
    _r("near_budget", 4, [96, 112], 4, 2, 32, "LDS within 2 KB", "LDS floats x 4 is within 2 KB below FCP_LDS_BUDGET (and fits both plans)"),
    _r("par_not_steps", 4, [100, 104], 8, 2, 32, "par not steps", "fits fc_par_plan (32 bytes to spare), not fc_steps_plan: the n-step entry loops"),
    _r("K1_dqn", 8, [25, 25], 4, 1, 32, "K=1", "K = 1: the DQN agent, leaves without a head axis"),
    _r("K9", 6, [20], 3, 9, 10, "K=9", "K = 9: nine workgroups"),
]
REFUSED = [
    _r("L1_no_hidden", 8, [], 4, 2, 7, "refused", "no hidden layer (features = []): idqn_create refuses what DQNNet accepts", route=None),
]
OUTSIDE = [
    _r("out_w129", 8, [129], 4, 2, 16, "width>128", "a hidden width of 129: a fifth column tile", "k_fc_step_mfma<global>"),
    _r("out_d0_129", 129, [16], 4, 2, 16, "d0>128", "d0 = 129: more than 8 minibatch elements per thread", "k_fc_step_mfma<lds>"),
    _r("out_P", 4, [8, 40, 72, 96], 18, 2, 16, "P>12288", "P = 12,352: one leaf pad over 12,288 with every width <= 128", "k_fc_step_mfma<lds>"),
    _r("out_lds", 4, [16, 72, 128], 8, 2, 16, "LDS over", "16 bytes over FCP_LDS_BUDGET with P <= 12,288 and widths <= 128", "k_fc_step_mfma<global>"),
    _r("out_B33", 8, [100, 100], 4, 2, 33, "B>32", "B = 33 on the LunarLander net: a second sample block", "k_fc_step_mfma<lds>"),
]
TABLE = INSIDE + REFUSED + OUTSIDE
RUNNABLE = INSIDE + OUTSIDE
BY_ID = {r.id: r for r in TABLE}
ALL_TERMINAL = "L4"                       # the row whose samples are all terminal
RAGGED = ("B1", "B2", "B31")              # the pad-lane poison rows
TIE_ROWS = ("w128_hidden", "A1")          # ties: the maximum at indices 2 and 5 -> action 2; A = 1 -> action 0
# The rows the descendants' identity tests import: odd din and a 33-wide layer (w33: din = 33 at its Q head), a 128-wide layer,
# A = 1, d0 = 128, B = 1, the near-budget net -- and the par-but-not-steps net, which the n-step entry runs as a loop
DESCENDANT_ROWS = ("w33", "w128_hidden", "A1", "d0_128", "B1", "near_budget")
DESCENDANT_LOOP_ROW = "par_not_steps"

# ---- bars (section 5 of the issue: fixed on the CPU, never on what the kernel gave) -------------------------------------------------
GAMMA, N_STEP, LR = 0.97, 3, 1e-3         # as tests/test_gpu_fp_path.py::test_ragged_batches_and_shapes_against_oracle
GAMMA_N = GAMMA ** N_STEP
LOSS_ATOL = 1e-5                          # per-head loss (test_gpu_fp_path.py)
GRAD_RTOL = 2e-5                          # a leaf's gradient, relative to the leaf's largest entry (test_gpu_fp_path.py)
TD_RTOL, TD_ATOL = 2e-5, 2e-6             # |TD| (test_gpu_per_extension.py)
PARAM_ATOL = 2e-5                         # a parameter after the steps (test_gpu_fc_learn_steps.py::test_eight_steps_against_the_oracle)
Q_RTOL = 1e-5                             # Q-values, relative to max(1, max |q|)
GAP = 1e-4                                # greedy actions are compared where the fp64 top-two gap exceeds this
N_STEPS_CHAIN = 3
# mu / nu after the three steps, relative to the leaf's largest |mu| / |nu| of that head: the project had no bar.  The fp32 oracle's
# largest deviation from the fp64 oracle over the table is MOMENT_FP32_DEV (tests/test_fc_shapes_host.py measures it and requires
# it to stay within half of the bar); the bar is 4 x that, rounded up to one digit.
MOMENT_FP32_DEV = 3.78e-6   # row A1, mu of the one-element leaf Dense_1/bias (three gradients of mixed sign partly cancel)
MOMENT_RTOL = 1.6e-5


# ---- inputs and the oracle's answers, built once per row and shared, never modified ------------------------------------------------
def obs_of(row):
    return row.d0


def _batch(row, seed):
    """Q.synthetic_batch reshaped to the issue's batch: one terminal sample (all of them for ALL_TERMINAL; B = 1: in the second batch), action A - 1 on the
    first sample and action 0 on the last (B = 1: A - 1 on even seeds, 0 on odd ones), reward magnitudes log-spaced over
    1e-3 .. 10 with random signs (B = 1: 1e-2, 1e-1, 1 over the three batches -- one squared TD error of ~100 has an fp32 ulp of
    7.6e-6, which leaves nothing of a 1e-5 bar to share)."""
    from oracle import qnet_ref as Q

    B, A = row.B, row.A
    s, a, r, s2, term = Q.synthetic_batch(seed, B, row.d0, A, "fc")
    rng = np.random.default_rng(1000 + seed)
    mag = 10.0 ** np.linspace(-3.0, 1.0, B) if B > 1 else np.array([10.0 ** (seed % 3 - 2)])
    r = (rng.permutation(mag) * rng.choice([-1.0, 1.0], B)).astype(np.float32)
    term = np.zeros(B, bool)
    term[B // 2] = B > 1 or seed % 3 == 1  # (B = 1: the second of the three batches is the terminal one)
    if row.id == ALL_TERMINAL:
        term[:] = True
    a = a.copy()
    a[0] = A - 1 if (B > 1 or seed % 2 == 0) else 0
    if B > 1:
        a[B - 1] = 0
    return s, a.astype(np.int32), r, s2, term


@functools.lru_cache(maxsize=None)
def inputs(row_id):
    """(p, pt, batches[3], weights) of a row: parameters from Q.init_params with random biases, as
    test_ragged_batches_and_shapes_against_oracle builds them."""
    from oracle import qnet_ref as Q

    row = BY_ID[row_id]
    p = Q.init_params(3, "fc", row.d0, row.A, row.feats, row.K)
    pt = Q.init_params(4, "fc", row.d0, row.A, row.feats, row.K)
    rng = np.random.default_rng(5)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batches = tuple(_batch(row, 6 + 10 * row.seed + i) for i in range(N_STEPS_CHAIN))
    w = np.random.default_rng(9).uniform(0.05, 1.0, row.B).astype(np.float32)
    return p, pt, batches, w


def oracle(row_id, dtype=np.float64):
    """Everything the oracle says about a row in ``dtype``: per head (loss, grads, aux) plain and weighted on batch 0, the
    three chained Adam steps (per-step losses, cum, final p / mu / nu) and both nets' Q-values of batch 0's states."""
    return _oracle(row_id, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def _oracle(row_id, dtype_name):
    from oracle import qnet_ref as Q

    dtype = np.float64 if dtype_name == "float64" else np.float32
    row = BY_ID[row_id]
    p, pt, batches, w = inputs(row_id)
    K = row.K
    plain = [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batches[0], "fc", GAMMA_N, dtype) for k in range(K)]
    weighted = [Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batches[0], "fc", GAMMA_N, dtype, weights=w) for k in range(K)]
    cur = {n: v.astype(dtype) for n, v in p.items()}
    mu = {n: np.zeros(v.shape, dtype) for n, v in p.items()}
    nu = {n: np.zeros(v.shape, dtype) for n, v in p.items()}
    count, step_losses = np.zeros(K, np.int64), []
    for b in batches:
        cur, mu, nu, count, losses = Q.learn_on_batch(cur, pt, mu, nu, count, b, "fc", GAMMA_N, LR, row.eps, dtype)
        step_losses.append(np.asarray(losses, np.float64))
    q = np.stack([Q.forward(Q.head(p, k), batches[0][0], "fc", dtype) for k in range(K)])
    qt = np.stack([Q.forward(Q.head(pt, k), batches[0][0], "fc", dtype) for k in range(K)])
    return dict(plain=plain, weighted=weighted, losses=np.stack(step_losses), cum=np.sum(step_losses, axis=0), p=cur, mu=mu, nu=nu,
                count=count, q=q, qt=qt)


def rel_to_max(got, want):
    """max |got - want| relative to max |want| (the gradient bar's scale)."""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30))
