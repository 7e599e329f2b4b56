"""The shape table of the i-IQN learner step's heads (``idqn_iqn_learn_on_batch``): one row per branch on the number of 32-row blocks
per virtual net, ``NB = N * ceil(B / 32)``, and on the divisors of the fraction count ``N``.

**Routes of the Dense_0 layer** (csrc/qnet.hip: ``iqn_heads_forward`` and the tail of ``idqn_iqn_learn_on_batch``):

=========== =================================== =====================================================================================
route       condition                           kernels; launch names of ``idqn_profile_table``
=========== =================================== =====================================================================================
stream      NB % 8 != 0                         ``k_dense0_fwd3``, ``k_dense0_dgrad<4>``, the plain step's fused update over NB blocks:
                                                ``iqn dense0 dgrad``, ``factor planes`` (NB >= 2), ``dense0 wgrad + adam``
gemm-dgrad  NB % 8 == 0, NB % 16 != 0           ``k_iqn_d0_fwd``, ``k_iqn_d0_dgrad`` alone, the same fused update: the same three names
two-split   NB % 16 == 0, plan says not fused   ``k_iqn_d0_bwd`` (KS = 2) + ``k_iqn_d0_adam``: ``iqn dense0 dgrad + wgrad``, ``iqn dense0 adam``
fused       NB % 16 == 0, plan says fused       ``k_iqn_d0_bwd_adam`` (gate, host item table, Adam in the epilogue):
                                                ``iqn dense0 dgrad + wgrad + adam``
=========== =================================== =====================================================================================

The launch names tell the last two routes from each other and from the first two; *stream* and *gemm-dgrad* share their names (the
data gradient is ``iqn dense0 dgrad`` whichever kernel computes it, and the name ``iqn dense0 wgrad`` belongs to a branch no batch
reaches: with NB % 16 == 0 the weight gradient always rides in the data gradient's launch), so between those two the route follows from
NB alone.  ``expected_route`` restates the rule, with the planner's fused-versus-split decision (``plan_iqn_bwd_order``) for 256 CUs;
nothing under csrc/ is imported.

Inputs are built as ``tests/test_gpu_iqn_batches._small_inputs`` builds them (nonzero biases of both nets, terminal samples at both
ends of the batch) and conditioned as tools/make_iqn_batch_golden.py conditions its case (``_condition``).  tests/test_iqn_shapes_host.py checks on the CPU what the table covers, that every row's seed shift is the smallest
admissible one and that the oracle's own fp32 restatement uses at most half of every bar; tests/test_gpu_iqn_shapes.py holds every row
to the fp64 oracle (oracle/iqn_ref.py).
"""
import functools
import heapq
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id obs A feats K N B why")

FRAME, TINY = (20, 20, 4), (8, 8, 4)  # F = 9 C2 and F = C2 (the Conv_2 width)
N_CUS = 256                           # of the MI355X: what the planner is restated for
A_STAR_GAP = 1e-3                     # the oracle's q_sel top-two gap, relative to max(1, max |q_sel|) of the head
HALF = 0.5
# no online ReLU pre-activation (Conv_0 .. 2, Embed_0, Dense_0; every head, every chained step) within this of zero: there fp32 and fp64
# may take different branches and the fp64 derivative is no reference for fp32 arithmetic of any kind -- the conditioning and the
# figure of tools/make_iqn_batch_golden.py: an offending sample gets a fresh state and fresh online fractions (``_condition``).  Row N40 at seed shift 0: one Embed_0 unit of head 1 at 2.0e-8 (feature 226); numpy fp32
# stays on the oracle's side, the device does not, and column 226 of Embed_0/kernel's gradient moves by 1.6e-3 of the leaf's largest.
RELU_MARGIN = 2e-7
N_STEPS_CHAIN = 3
LOSS_RTOL, Z_RTOL, GRAD_RTOL, PARAM_LR, PARAM_RTOL = 1e-5, 2e-5, 3e-5, 0.02, 2e-7  # the bars of cnn_stages.check_iqn_step
ACT_Q_RTOL = 2e-6                     # acting Q rows, relative to max(1, max |q|) (tests/test_gpu_iqn_batches.py)
TD_RTOL, TD_ATOL = 2e-5, 2e-6         # td_abs of the weighted step (tests/test_gpu_iqn_per.py)
# mu / nu after the three chained steps, relative to the leaf's largest |mu| / |nu| of that head: the project had no bar.  The fp32
# oracle's largest deviation from the fp64 oracle over the chained rows, on conditioned inputs, is MOMENT_FP32_DEV (2.804e-6: row
# K18_N32_F576, nu; tests/test_iqn_shapes_host.py measures it on every chained row and requires it to stay below this figure); the bar
# is 4 x that, rounded up to two digits, the rule of tests/fc_shapes.py.  (Where a ReLU unit of steps 1 .. 2 falls on the other side of
# zero in fp32 the deviation is that unit's gradient -- 5.5e-4 at row K32_N16_J512 before its inputs were conditioned -- and says
# nothing about arithmetic.)
MOMENT_FP32_DEV = 2.81e-6
MOMENT_RTOL = 1.2e-5


def _r(id, why, N=16, K=2, B=32, J=256, C2=32, obs=FRAME, A=5):
    return Row(id, obs, A, [32, 32, C2, J], K, N, B, why)


TABLE = [
    # ---- divisors of N, all on the stream route (per / QG / HG in the reason) ---------------------------------------------------------
    _r("N2", "stream, 2 blocks: per / QG / HG = 2 / 2 / 2", N=2),
    _r("N3", "stream: per / QG / HG = 3 / 3 / 3, the first odd group size", N=3),
    _r("N5", "stream: per / QG / HG = 5 / 1 / 5", N=5),
    _r("N6", "stream: per / QG / HG = 6 / 3 / 6", N=6),
    _r("N7", "stream: per / QG / HG = 7 / 1 / 7, one embedding-backward group", N=7),
    _r("N9", "stream: per / QG / HG = 3 / 3 / 3 at more than 8 blocks", N=9),
    _r("N11", "stream, a prime above 8: per / QG / HG = 1 / 1 / 1", N=11),
    _r("N12", "stream: per / QG / HG = 6 / 4 / 6", N=12),
    _r("N33", "stream: per / QG / HG = 3 / 3 / 3 past 32 fractions (k_iqn_loss's LDS, acting NP = 64)", N=33),
    _r("N61", "stream, a prime: 61 blocks through the fused update and k_dense0_dgrad<4>, groups 1 / 1 / 1", N=61),
    _r("N63", "stream: 63 blocks, per / QG / HG = 7 / 3 / 7", N=63),
    _r("N7_J512", "stream with two column tiles: k_dense0_fwd3 over four 128-column tiles, k_dense0_dgrad<4> at 64 KB of LDS", N=7, J=512),
    # ---- gemm-dgrad -----------------------------------------------------------------------------------------------------------------
    _r("N8", "gemm-dgrad: one group of 8 blocks, per / QG / HG = 8 / 4 / 8", N=8),
    _r("N8_J512", "gemm-dgrad with two column tiles", N=8, J=512),
    _r("N24", "gemm-dgrad: three groups of 8 blocks", N=24),
    _r("N40", "gemm-dgrad: five groups of 8 blocks past 32 fractions", N=40),
    # ---- two-split ------------------------------------------------------------------------------------------------------------------
    _r("N16", "two-split: nbg = 2", N=16),
    _r("N16_J512", "two-split with two column tiles: four weight-gradient items per group", N=16, J=512),
    _r("N48", "two-split: nbg = 6", N=48),
    _r("N64", "two-split at the largest N: nbg = 8", N=64),
    _r("N16_F32", "two-split below one row tile: F = 32", N=16, obs=TINY),
    _r("N16_F64", "two-split below one row tile: F = 64", N=16, obs=TINY, C2=64),
    _r("N16_F576", "two-split with three row groups, the last ragged: F = 2 * 256 + 64", N=16, C2=64),
    # ---- fused, nb = 1 --------------------------------------------------------------------------------------------------------------
    _r("K18_N32_F576", "fused: G = 54 groups, 270 items", K=18, N=32, C2=64),
    _r("K11_N64_F576", "fused: G = 33 groups, 297 items, nbg = 8", K=11, N=64, C2=64),
    _r("K15_N32_F576_J512", "fused: G = 45 groups, 270 items, two weight-gradient items per gate group", K=15, N=32, C2=64, J=512),
    # ---- the fuse threshold itself --------------------------------------------------------------------------------------------------
    _r("K32_N16_J512", "threshold: G = 64, exactly 256 items: not fused (>)", K=32, N=16, J=512),
    _r("K33_N16_J512", "threshold: G = 66, 264 items: fused", K=33, N=16, J=512),
    # ---- nb > 1: the planner's model decides ----------------------------------------------------------------------------------------
    _r("N16_B33", "nb = 2 with one sample in the second block", N=16, B=33),
    _r("N16_B64", "nb = 2, both blocks full", N=16, B=64),
    _r("N4_B100", "nb = 4 at N = 4: NB = 16, ragged last block", N=4, B=100),
    _r("N8_B256", "nb = 8 at N = 8: NB = 64, the largest batch", N=8, B=256),
    _r("K18_N32_F576_B64", "nb = 2 at the fused shape: NB = 64, 486 items, two splits", K=18, N=32, C2=64, B=64),
    _r("K8_N8_F576_J512_B64", "nb = 2 where the planner's model prefers the fused launch: 24 groups, 96 items", K=8, N=8, C2=64, J=512, B=64),
    _r("K3_N16_F576_B64", "nb = 2 at few heads: 9 groups, at most two per XCD", K=3, N=16, C2=64, B=64),
    # ---- a ragged single block ------------------------------------------------------------------------------------------------------
    _r("N16_B1", "two-split, one sample (a terminal one)", N=16, B=1),
    _r("N16_B31", "two-split, one lane short of a block", N=16, B=31),
    _r("N7_B20", "stream, ragged block at an odd N", N=7, B=20),
]
BY_ID = {r.id: r for r in TABLE}
assert len(BY_ID) == len(TABLE)
IDS = [r.id for r in TABLE]

# the seed shift of a row (``seed_shift``): rows not named here take 0
_SHIFT = {"N3": 1, "N6": 1, "N11": 1, "N12": 2, "N33": 2, "N8": 1, "N16_J512": 1, "N16_F32": 1, "N16_F576": 1, "K18_N32_F576": 2, "K11_N64_F576": 3,
          "K15_N32_F576_J512": 11, "K32_N16_J512": 97, "K33_N16_J512": 199, "N16_B33": 1, "K18_N32_F576_B64": 36, "K8_N8_F576_J512_B64": 2, "K3_N16_F576_B64": 1}

ACT_ROWS = ("N33", "N61", "N64")                                                     # acting with NP = 64
FUSE_OFF_ROWS = ("K18_N32_F576", "K11_N64_F576", "K15_N32_F576_J512", "K8_N8_F576_J512_B64")  # IDQN_IQN_ADAM_FUSE=0
WEIGHTED_ROWS = ("N6", "N8", "N16", "K11_N64_F576")                                  # one row per route


def cdiv(a, b):
    return -(-a // b)


def divisor_at_most(n, cap):
    d = cap
    while d > 1 and n % d:
        d -= 1
    return d


def groups(row):
    """(per, QG, HG): fractions per wave of the embedding forward, fraction groups of the embedding backward and of k_iqn_dh."""
    return divisor_at_most(row.N, 8), divisor_at_most(row.N, 4), divisor_at_most(row.N, 8)


def dims(row):
    """(F, J, nb, NB)"""
    from oracle import qnet_ref as Q

    h, w, _ = row.obs
    for k, s in Q.CNN_GEOM:
        h, w = Q.same_pad(h, k, s)[0], Q.same_pad(w, k, s)[0]
    nb = cdiv(row.B, 32)
    return h * w * row.feats[2], row.feats[3], nb, row.N * nb


# ---- the planner, restated (csrc/qnet.hip: iqn_bwd_makespan, iqn_bwd_seq, plan_iqn_bwd_order) ------------------------------------------
def _makespan(seq, dw, ncu):
    """List scheduling of the items (0: a data-gradient item of length 1, 1: a weight-gradient item of length dw) on ncu units."""
    cus = [0.0] * ncu
    end = 0.0
    for it in seq:
        e = heapq.heappop(cus) + (dw if it else 1.0)
        heapq.heappush(cus, e)
        end = max(end, e)
    return end


def _seq(n, e, nbg, n_jh):
    return ([0] * nbg + [1] * n_jh) * e + [0] * (nbg * (n - e)) + [1] * (n_jh * (n - e))


def plan(row, n_cus=N_CUS):
    """dict(G, nbg, n_jh, items, fused): groups, data- and weight-gradient items per group, items of the merged launch, and whether the
    plan puts Adam into the launch's epilogue.  NB must be a multiple of 16."""
    F, J, nb, NB = dims(row)
    assert NB % 16 == 0 and J % 256 == 0
    nbg, n_jh, G = NB // 8, J // 256, row.K * cdiv(F, 256)
    dw = 1.68 * (NB / 32.0) * (512.0 / J) + 0.33
    xcd = max(1, n_cus // 8)
    fused = 0.0
    for x in range(8):
        n = (G - x + 7) // 8
        best_e, best = n, 0.0
        for e in range(n + 1):
            seq = _seq(n, e, nbg, n_jh)
            total = 0.0
            for sc in (0.92, 0.96, 1.0, 1.04, 1.08):
                total += _makespan(seq, dw * sc, xcd)
            if e == 0 or total < best:
                best, best_e = total, e
        fused = max(fused, _makespan(_seq(n, best_e, nbg, n_jh), dw, xcd))
    n_d, n_w1 = G * nbg, G * n_jh
    if nb == 1:
        fuse = n_d + n_w1 > n_cus
    else:
        unit_us = 84.0 * J / 512.0
        adam = float(row.K) * F * J * 32.0 / 4.0e6 / unit_us
        split = _makespan([0] * n_d + [1] * (2 * n_w1), (dw - 0.33) / 2, max(1, n_cus)) + adam
        fuse = fused < split
    return dict(G=G, nbg=nbg, n_jh=n_jh, items=n_d + n_w1, fused=bool(fuse), spans=(fused, None if nb == 1 else split))


def route(row, fuse_switch=True):
    """"stream" | "gemm-dgrad" | "two-split" | "fused"; ``fuse_switch`` False: IDQN_IQN_ADAM_FUSE=0."""
    NB = dims(row)[3]
    if NB % 8:
        return "stream"
    if NB % 16:
        return "gemm-dgrad"
    return "fused" if fuse_switch and plan(row)["fused"] else "two-split"


DENSE0_NAMES = ("iqn dense0 dgrad + wgrad + adam", "iqn dense0 dgrad + wgrad", "iqn dense0 adam", "iqn dense0 dgrad", "iqn dense0 wgrad",
                "factor planes", "dense0 wgrad + adam")


def expected_route(row, fuse_switch=True):
    """The names of the step's Dense_0 backward launches, in launch order, as ``idqn_profile_table`` lists them."""
    r = route(row, fuse_switch)
    if r == "fused":
        return ["iqn dense0 dgrad + wgrad + adam"]
    if r == "two-split":
        return ["iqn dense0 dgrad + wgrad", "iqn dense0 adam"]
    # the plain step's fused update over NB blocks: its dL/dh goes through the plane copy from two blocks on
    return ["iqn dense0 dgrad"] + (["factor planes"] if dims(row)[3] >= 2 else []) + ["dense0 wgrad + adam"]


def dense0_launches(profile_names):
    return [n for n in profile_names if n in DENSE0_NAMES]


def chained(row):
    """Rows that run three chained steps: every fused row, the K = 32 threshold row and one row of each other route."""
    return route(row) == "fused" or row.id in ("K32_N16_J512", "N6", "N8", "N16")


CHAIN_IDS = [r.id for r in TABLE if chained(r)]


# ---- inputs and the oracle -----------------------------------------------------------------------------------------------------------
def hyper():
    from oracle import make_golden as G

    return G.FP_HYPER


def seed_shift(row):
    """The smallest shift at which ``admissible`` holds (tests/test_iqn_shapes_host.py asserts that no smaller one does)."""
    return _SHIFT.get(row.id, 0)


def _seed(row, shift):
    return 100 + row.N + row.B + 7 * row.K + 1000 * (seed_shift(row) if shift is None else shift)


@functools.lru_cache(maxsize=None)
def params(rid, shift=None):
    """(p, pt): both nets with nonzero biases."""
    from oracle import iqn_ref as I

    row = BY_ID[rid]
    seed = _seed(row, shift)
    p = I.init_params(seed, row.obs, row.A, row.feats, row.K)
    pt = I.init_params(seed + 1, row.obs, row.A, row.feats, row.K)
    rng = np.random.default_rng(seed + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
            pt[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    return p, pt


def step_inputs(rid, step=0, shift=None):
    """(batch, taus [K][3][N][B]) of chained step ``step``, conditioned: ``raw_inputs`` with the samples that put an online ReLU
    pre-activation within RELU_MARGIN of zero replaced (``_condition``; the parameters of step t are the fp64 oracle's after t steps)."""
    row = BY_ID[rid]
    return _oracle(rid, "float64", shift, N_STEPS_CHAIN if chained(row) else 1)["inputs"][step]


@functools.lru_cache(maxsize=None)
def raw_inputs(rid, step=0, shift=None):
    """(batch, taus [K][3][N][B]) of chained step ``step``: a different batch and different fractions each, terminals at both ends."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    seed = _seed(row, shift) + 37 * step
    st, a, r, s2, term = Q.synthetic_batch(seed + 10, row.B, row.obs, row.A, "cnn")
    term = term.copy()
    term[0] = True
    term[row.B - 1] = True
    return (st, a, r, s2, term), I.synthetic_taus(seed + 20, row.K, row.N, row.B)


@functools.lru_cache(maxsize=None)
def act_inputs(rid):
    """(states [n], fractions [n, N]) of the acting check: the first min(B, 32) states of step 0."""
    row = BY_ID[rid]
    n = min(row.B, 32)
    return step_inputs(rid)[0][0][:n], np.random.default_rng(_seed(row, None) + 30).random((n, row.N)).astype(np.float32)


def top_gap(q):
    q = np.asarray(q, np.float64)
    if q.shape[-1] < 2:
        return np.full(q.shape[:-1], np.inf)
    top = np.sort(q, axis=-1)
    return top[..., -1] - top[..., -2]


def min_preact(p, state, tau_on):
    """Per sample: the smallest |pre-activation| of every ReLU on the online side of one head (fp64)."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    a = state.astype(np.float64) / 255.0
    m = np.full(state.shape[0], np.inf)
    for li, (k, s) in enumerate(Q.CNN_GEOM):
        y, _ = Q.conv_fwd(a, p[f"Conv_{li}/kernel"].astype(np.float64), p[f"Conv_{li}/bias"].astype(np.float64), s)
        m = np.minimum(m, np.abs(y).reshape(y.shape[0], -1).min(1))
        a = np.maximum(y, 0)
    psi = a.reshape(a.shape[0], -1)
    e = I.cos_features(tau_on) @ p["Embed_0/kernel"].astype(np.float64) + p["Embed_0/bias"].astype(np.float64)
    m = np.minimum(m, np.abs(e).min(axis=(0, 2)))
    pre = (psi[None] * np.maximum(e, 0)) @ p["Dense_0/kernel"].astype(np.float64) + p["Dense_0/bias"].astype(np.float64)
    return np.minimum(m, np.abs(pre).min(axis=(0, 2)))


def _condition(p, rid, step, shift):
    """``raw_inputs`` of the step with every sample that brings an online pre-activation of some head (parameters ``p``, fp64) within
    RELU_MARGIN of zero given a fresh state and fresh online fractions, until none does -- the conditioning of
    tools/make_iqn_batch_golden.py.  Returns (batch, taus, [(round, sample)])."""
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    (st, a, r, s2, term), taus = raw_inputs(rid, step, shift)
    st, taus = st.copy(), taus.copy()
    seed, replaced = _seed(row, shift) + 37 * step, []
    for rnd in range(50):
        bad = np.zeros(row.B, bool)
        for k in range(row.K):
            bad |= min_preact(Q.head(p, k), st, taus[k, 0]) < RELU_MARGIN
        if not bad.any():
            return (st, a, r, s2, term), taus, replaced
        for b in np.flatnonzero(bad):
            g = np.random.default_rng([seed, 1000 + rnd, int(b)])
            st[b] = g.integers(0, 256, size=st.shape[1:], dtype=np.uint8)
            taus[:, 0, :, b] = g.random(taus[:, 0, :, b].shape).astype(np.float32)
            replaced.append((rnd, int(b)))
    raise RuntimeError("no well-conditioned inputs found")


def oracle(rid, dtype=np.float64, shift=None, steps=None):
    row = BY_ID[rid]
    return _oracle(rid, np.dtype(dtype).name, shift, (N_STEPS_CHAIN if chained(row) else 1) if steps is None else steps)


@functools.lru_cache(maxsize=None)
def _oracle(rid, dtype_name, shift, steps):
    """``steps`` chained calls of ``iqn_ref.learn_on_batch``, restated head by head so that what it does not return is kept too: per
    step the losses [K], a* [K, B] and the relative top-two gap of q_sel [K, B]; of step 0 head 0's quantile values, every leaf
    gradient and the state after it; ``big`` -- per leaf, where the gradient of EVERY step exceeds 1e-3 of its head's largest (the
    elements whose Adam direction is not sign-like at any step); the parameters, mu and nu after the last step."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    dtype = np.float64 if dtype_name == "float64" else np.float32
    row, hy = BY_ID[rid], hyper()
    K, gamma_n = row.K, hy["gamma"] ** hy["n"]
    p0, pt = params(rid, shift)
    p = {n: a.astype(dtype).copy() for n, a in p0.items()}
    mu = {n: np.zeros(a.shape, dtype) for n, a in p0.items()}
    nu = {n: np.zeros(a.shape, dtype) for n, a in p0.items()}
    out = dict(losses=[], a_star=[], gap=[], inputs=[], replaced=[])
    big = {n: np.ones(a.shape, bool) for n, a in p0.items()}
    for t in range(steps):
        if dtype is np.float64:
            batch, taus, replaced = _condition(p, rid, t, shift)
            out["inputs"].append((batch, taus))
            out["replaced"].append(replaced)
        else:
            batch, taus = _oracle(rid, "float64", shift, steps)["inputs"][t]
        losses, a_star, gap = np.zeros(K, dtype), [], []
        grads = {n: np.zeros(a.shape, dtype) for n, a in p0.items()}
        for k in range(K):
            loss, g, aux = I.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, tuple(taus[k]), gamma_n, dtype)
            losses[k] = loss
            a_star.append(aux["a_star"])
            q_sel = np.asarray(aux["q_sel"], np.float64)
            gap.append(top_gap(q_sel) / max(1.0, float(np.abs(q_sel).max())))
            if t == 0 and k == 0:
                out["z_online_head0"], out["z_target_head0"], out["q_select_head0"] = aux["z_a"], aux["z_t"], aux["q_sel"]
            for n in p:
                grads[n][k] = g[n]
                big[n][k] &= np.abs(g[n]) > 1e-3 * np.abs(g[n]).max()
                p[n][k], mu[n][k], nu[n][k] = Q.adam_update(p[n][k], g[n].astype(dtype), mu[n][k], nu[n][k], t, hy["lr"], hy["eps"], dtype)
        out["losses"].append(losses)
        out["a_star"].append(np.stack(a_star))
        out["gap"].append(np.stack(gap))
        if t == 0:
            out["grads"] = grads
            out["params_step0"] = {n: a.copy() for n, a in p.items()}
    out.update(params=p, mu=mu, nu=nu, big=big, steps=steps)
    return out


def record(rid, shift=None):
    """What ``cnn_stages.iqn_record`` returns for step 0 of the row, served from ``oracle`` (one fp64 evaluation per row)."""
    o, K = oracle(rid, shift=shift), BY_ID[rid].K
    rec = {"hyper": hyper(), "losses": o["losses"][0], "z_online_head0": o["z_online_head0"], "z_target_head0": o["z_target_head0"],
           "a_star_head0": o["a_star"][0][0], "q_select_head0": o["q_select_head0"], "leaves": {}}
    for leaf, g in o["grads"].items():
        flat_g, flat_p = g.reshape(K, -1), o["params_step0"][leaf].reshape(K, -1)
        rec["leaves"][leaf] = {"idx": np.arange(flat_g.shape[1]), "grad": flat_g, "param": flat_p, "grad_absmax": np.abs(flat_g).max(1)}
    return rec


@functools.lru_cache(maxsize=None)
def min_gap(rid, shift=None):
    """Smallest top-two gap of the fp64 oracle's q_sel of step 0, relative to max(1, max |q_sel|) of the head, over every head and
    every live (non-terminal) sample -- a terminal sample's a* does not reach the loss -- and over EVERY sample of head 0, whose a* the
    step check compares exactly.  Only the target nets' forward: cheap enough to search hundreds of shifts."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = BY_ID[rid]
    pt = params(rid, shift)[1]
    batch, taus = raw_inputs(rid, 0, shift)  # (conditioning leaves the next states and the selection fractions alone)
    live = ~np.asarray(batch[4], bool)
    worst = np.inf
    for k in range(row.K):
        ph = Q.head(pt, k)
        q_sel = I.quantile_values(ph, I.trunk(ph, batch[3]), taus[k][1]).mean(0)
        gap = top_gap(q_sel) / max(1.0, float(np.abs(q_sel).max()))
        use = gap if k == 0 else gap[live]
        if use.size:
            worst = min(worst, float(use.min()))
    return worst


def chain_errors(got_losses, got, want, K, lr):
    """The chained comparison: ``got_losses`` [steps][K] and ``got`` = (params, mu, nu) {leaf: [K, ...]} after the last step against the
    oracle dict ``want``.  Returns the figures as shares of their bars: loss (LOSS_RTOL of max(1, |loss|) per step), param (the
    post-Adam rule of check_iqn_step with steps * PARAM_LR * lr, where the gradient of every step is not negligible), mu and nu
    (relative to the leaf's largest entry per head; bar MOMENT_RTOL -- returned as the plain relative deviation)."""
    steps = want["steps"]
    fig = dict(loss=0.0, param=0.0, mu=0.0, nu=0.0)
    for t in range(steps):
        w = np.asarray(want["losses"][t], np.float64)
        fig["loss"] = max(fig["loss"], float(np.abs(np.asarray(got_losses[t], np.float64) - w).max() / max(1.0, np.abs(w).max()) / LOSS_RTOL))
    gp, gm, gv = got
    for leaf in want["params"]:
        wp = np.asarray(want["params"][leaf], np.float64).reshape(K, -1)
        big = want["big"][leaf].reshape(K, -1)
        if big.any():
            err = np.abs(np.asarray(gp[leaf], np.float64).reshape(K, -1) - wp)
            fig["param"] = max(fig["param"], float((err[big] / (steps * PARAM_LR * lr + PARAM_RTOL * np.abs(wp[big]))).max()))
        for key, g, w in (("mu", gm, want["mu"]), ("nu", gv, want["nu"])):
            ww = np.asarray(w[leaf], np.float64).reshape(K, -1)
            scale = np.abs(ww).max(1)[:, None] + 1e-300
            fig[key] = max(fig[key], float((np.abs(np.asarray(g[leaf], np.float64).reshape(K, -1) - ww) / scale).max()))
    return fig


def fp32_shares(rid, shift=None):
    """The fp32 oracle's deviation from the fp64 oracle as shares of the bars the GPU test applies (check_iqn_step's for step 0, the
    chained comparison's where the row is chained; mu / nu as plain relative deviations), and whether its a* is the fp64 oracle's on
    every step."""
    row = BY_ID[rid]
    o64, o32 = oracle(rid, shift=shift), oracle(rid, np.float32, shift=shift)
    K, lr = row.K, hyper()["lr"]
    w = np.asarray(o64["losses"][0], np.float64)
    fig = dict(loss=float(np.abs(o32["losses"][0] - w).max() / max(1.0, np.abs(w).max()) / LOSS_RTOL), z=0.0, grad=0.0, param=0.0)
    for key in ("z_online_head0", "z_target_head0", "q_select_head0"):
        w = np.asarray(o64[key])
        fig["z"] = max(fig["z"], float(np.abs(o32[key] - w).max() / max(1.0, np.abs(w).max()) / Z_RTOL))
    for leaf, g in o64["grads"].items():
        wg, wp = g.reshape(K, -1), o64["params_step0"][leaf].reshape(K, -1)
        scale = np.abs(wg).max(1)[:, None]
        fig["grad"] = max(fig["grad"], float((np.abs(o32["grads"][leaf].reshape(K, -1) - wg) / (GRAD_RTOL * scale + 1e-12)).max()))
        bigm = np.abs(wg) > 1e-3 * scale
        err = np.abs(o32["params_step0"][leaf].reshape(K, -1) - wp)
        fig["param"] = max(fig["param"], float((err[bigm] / (PARAM_LR * lr + PARAM_RTOL * np.abs(wp[bigm]))).max()))
    if o64["steps"] > 1:
        c = chain_errors(o32["losses"], (o32["params"], o32["mu"], o32["nu"]), o64, K, lr)
        fig.update(chain_loss=c["loss"], chain_param=c["param"], mu=c["mu"], nu=c["nu"])
    same_a_star = all(np.array_equal(a, b) for a, b in zip(o32["a_star"], o64["a_star"]))
    return fig, same_a_star


def admissible(rid, shift=None):
    """The two conditions on a row's inputs (the third, no online ReLU pre-activation within RELU_MARGIN of zero, holds by construction:
    ``_condition``): the fp64 oracle's q_sel top-two gap of step 0 exceeds A_STAR_GAP for every head and live
    sample (``min_gap``), and the fp32 oracle stays within half of every bar (mu / nu of a chained row: within MOMENT_FP32_DEV, a quarter
    of theirs) with the fp64 oracle's a* on every step."""
    if not min_gap(rid, shift) > A_STAR_GAP:
        return False
    fig, same = fp32_shares(rid, shift)
    bars = {k: v for k, v in fig.items() if k not in ("mu", "nu")}
    return same and max(bars.values()) <= HALF and max(fig.get("mu", 0.0), fig.get("nu", 0.0)) <= MOMENT_FP32_DEV


@functools.lru_cache(maxsize=None)
def acting_oracle(rid, dtype_name="float64"):
    """{(which, head): Q rows [n, A]} of ``iqn_ref.greedy_action`` on ``act_inputs``."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    dtype = np.float64 if dtype_name == "float64" else np.float32
    row = BY_ID[rid]
    states, taus = act_inputs(rid)
    out = {}
    for which, prm in enumerate(params(rid)):
        for k in range(row.K):
            out[(which, k)] = np.stack([I.greedy_action(Q.head(prm, k), states[e], taus[e], dtype)[1] for e in range(len(states))])
    return out
