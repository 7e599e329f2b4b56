"""The factored Dense_0 update (``idqn_finish_step_factored``): the table of block counts, geometries and factor layouts that
tests/test_factored_shapes_host.py (CPU) and tests/test_gpu_factored_update.py (device) walk, the fp64 / float32 references of
the update, the synthetic factors, and the single-GPU emulation of several ranks.  Not a test module.

The update contracts the gathered factors of the Dense_0 weight gradient over ``nb_total`` blocks of 32 samples,

    G[k] = sum_bb a3[bb, k] (F x 32) . dh[bb, k]^T (32 x J),

and applies Adam to Dense_0/kernel in the same launch.  Block ``bb`` of head ``k`` lies at

    base + (bb // nb_inner) * outer + k * head + (bb % nb_inner) * inner        (floats)

which csrc computes in three places (k_split_factors, the a3 staging loop and the f32 contraction loop of dense0_wgrad_body).
The rules of launch_dense0_wgrad (csrc/qnet.hip) that decide which kernel runs are restated below as plain Python.
"""
import collections

import numpy as np

B1, B2 = 0.9, 0.999
LR, EPS = 6.25e-5, 1.5e-4     # the goldens' hyper-parameters (tests/golden/fp_path_*.json): their theta bar holds at this lr
GRAD_BAR = 2e-5               # * max |G[k]|: the project's gradient bar (tests/test_gpu_fp_path.py)
THETA_BAR = 3e-7              # the goldens' bar on a parameter after one step at LR
WARM_COUNT = 10_000

# ---- the rules of launch_dense0_wgrad, restated ---------------------------------------------------------------------------------
CH = 8                          # sample blocks the bf16-plane kernel stages per chunk (dense0_update.h, ALDS with RT = 1)
KEEP_BYTES = 84 << 20           # d0_keep_heads: K * F * J * 4 above this -> every head stores theta non-temporally


def nq(J):
    return 2 if J % 256 == 0 else 1          # 256- or 128-wide column tiles


def n_jt(J):
    return J // (128 * nq(J))


def bf3(nb_total, J):
    """The update runs on the bf16 matrix cores from planes ("factor planes" launch + k_dense0_wgrad_alds)."""
    return nb_total >= 2 and J % 256 == 0


def keep_heads(K, F, J):
    return K if K * F * J * 4 <= KEEP_BYTES else 0


def update_kernels(K, F, J, nb_total):
    """Kernel launches behind the one "dense0 wgrad + adam" line of the profile table: [(kernel, heads)]."""
    if not bf3(nb_total, J):
        return [("k_dense0_wgrad<true, %d>" % nq(J), K)]
    keep = min(keep_heads(K, F, J), K)
    return [(n, h) for n, h in (("k_dense0_wgrad_alds<1, false>", keep), ("k_dense0_wgrad_alds<1, true>", K - keep)) if h > 0]


def chunks(nb_total):
    """[(c0, nc)] of the staging loop."""
    return [(c0, min(CH, nb_total - c0)) for c0 in range(0, nb_total, CH)]


def bounds(case):
    """The bounds a case straddles (names used by the coverage test)."""
    nb, ni, J = case.nb_total, case.nb_inner, case.J
    out = set()
    if nb == 1:
        out.add("one block, fused f32 update")
    if any(bb // ni > 0 and bb % ni > 0 for bb in range(nb)):
        out.add("bo > 0 and bi > 0")
    if nb > 1 and ni == 1:
        out.add("outer term alone")
    if nb > 1 and ni == nb:
        out.add("inner term alone")
    if bf3(nb, J):
        cs = chunks(nb)
        if nb == CH:
            out.add("exactly one full chunk")
        if len(cs) > 1:
            out.add("c0 > 0")
            if cs[-1][1] == 1:
                out.add("last chunk of one block")
            if 1 < cs[-1][1] < CH:
                out.add("ragged later chunk of several blocks")
            if cs[-1][1] == CH:
                out.add("two full chunks")
        if len(cs) > 2:
            out.add("third chunk")
        if any(nc % 2 == 1 and nc > 1 for _, nc in cs):
            out.add("odd nc > 1")
        if n_jt(J) > 1:
            out.add("bf3, n_jt = 2")
        else:
            out.add("bf3, n_jt = 1")
        if keep_heads(case.K, F_OF[case.geom], J) == 0:
            out.add("non-temporal theta store")
    elif nb > 2:
        out.add("f32 route over more than two strided blocks, n_jt = %d" % n_jt(J))
    if F_OF[case.geom] == 32:
        out.add("F / 32 = 1")
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------------
GEOMS = {  # name: (frame, conv widths)
    "G0": ((8, 8, 4), [32, 32, 32]),      # 2x2 -> 1x1 -> 1x1, F = 32
    "G1": ((17, 17, 4), [32, 64, 64]),    # 5x5 -> 3x3 -> 3x3, F = 576
    "GA": ((84, 84, 4), [32, 64, 64]),    # Atari, F = 7744
}
F_OF = {"G0": 32, "G1": 576, "GA": 7744}
N_ACTIONS = 4

ROWS = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (4, 2), (6, 3), (8, 1), (8, 4), (9, 1), (9, 3), (10, 5), (16, 2), (17, 1)]
F32_ROWS = [(1, 1), (2, 1), (4, 2), (9, 3)]

Case = collections.namedtuple("Case", "geom K J nb_total nb_inner family")  # family: plain | dead | warm


def case_id(c):
    return "%s-K%d-J%d-%dx%d-%s" % (c.geom, c.K, c.J, c.nb_total, c.nb_inner, c.family)


CASES = ([Case("G1", 3, J, nb, ni, "plain") for J in (256, 512) for nb, ni in ROWS]
         + [Case("G1", 3, J, nb, ni, "plain") for J in (128, 384) for nb, ni in F32_ROWS]
         + [Case("G0", 1, 256, 9, 3, "plain"), Case("GA", 6, 512, 2, 1, "plain"), Case("GA", 6, 512, 9, 3, "plain")]
         # ragged shards: the trailing 24 columns of every shard's last block carry dL/dh = 0 and a3 != 0
         + [Case("G1", 3, 256, nb, ni, "dead") for nb, ni in ((2, 2), (4, 2), (9, 3), (10, 5))]
         + [Case("G1", 3, 128, 4, 2, "dead")]
         # mid-training Adam state
         + [Case("G1", 3, 256, nb, ni, "warm") for nb, ni in ((1, 1), (4, 2), (9, 3))]
         + [Case("G1", 3, 128, 4, 2, "warm"), Case("G1", 3, 512, 17, 1, "warm")])
LIVE_IN_DEAD_BLOCK = 8  # a shard of 40 samples: 8 live columns in its second block


# ---- layouts --------------------------------------------------------------------------------------------------------------------
Layout = collections.namedtuple("Layout", "name buf a3_off dh_off a3_strides dh_strides nb_inner X Y")  # strides: (outer, head, inner)


def _place(lay, a3, dh):
    nb_total, K = a3.shape[:2]
    for bb in range(nb_total):
        for k in range(K):
            block_of(lay, "a3", bb, k)[:] = a3[bb, k].reshape(-1)
            block_of(lay, "dh", bb, k)[:] = dh[bb, k].reshape(-1)
    return lay


def packed(a3, dh, nb_inner):
    """``[rank][dh | a3]``: what parallel._factored_step and csrc/dp.hip hand over after the all-gather."""
    nb_total, K = a3.shape[:2]
    X, Y = a3[0, 0].size, dh[0, 0].size
    n_a3, n_dh = K * nb_inner * X, K * nb_inner * Y
    buf = np.zeros((nb_total // nb_inner) * (n_a3 + n_dh), np.float32)
    return _place(Layout("packed", buf, n_dh, 0, (n_a3 + n_dh, nb_inner * X, X), (n_a3 + n_dh, nb_inner * Y, Y), nb_inner, X, Y), a3, dh)


def split(a3, dh, nb_inner):
    """Two separate arrays ``[rank][head][block]`` (idqn_export_dense0_factors per rank, concatenated)."""
    nb_total, K = a3.shape[:2]
    X, Y = a3[0, 0].size, dh[0, 0].size
    buf = np.zeros(nb_total * K * (X + Y), np.float32)
    return _place(Layout("split", buf, 0, nb_total * K * X, (K * nb_inner * X, nb_inner * X, X), (K * nb_inner * Y, nb_inner * Y, Y),
                         nb_inner, X, Y), a3, dh)


def gapped(a3, dh, nb_inner):
    """Outer, head and inner strides each enlarged by a different multiple of 4 floats (the kernels load float4: 16-byte
    alignment holds), every gap float NaN: one read outside a block poisons a whole tile."""
    nb_total, K = a3.shape[:2]
    n_outer = nb_total // nb_inner
    X, Y = a3[0, 0].size, dh[0, 0].size

    def strides(n, g_inner, g_head, g_outer):
        inner = n + 4 * g_inner
        head = nb_inner * inner + 4 * g_head
        outer = K * head + 4 * g_outer
        return outer, head, inner

    sa, sd = strides(X, 1, 2, 3), strides(Y, 3, 1, 2)
    lead = 20
    a3_off = lead
    dh_off = a3_off + n_outer * sa[0] + 8
    buf = np.full(dh_off + n_outer * sd[0], np.nan, np.float32)
    return _place(Layout("gapped", buf, a3_off, dh_off, sa, sd, nb_inner, X, Y), a3, dh)


LAYOUTS = {"packed": packed, "split": split, "gapped": gapped}


def block_offset(lay, which, bb, k, exchange=False):
    """Float offset of block ``bb`` of head ``k`` -- the address rule of the kernels; ``exchange`` restates it WRONGLY (outer
    and inner strides swapped) for the host test."""
    off, (outer, head, inner) = (lay.a3_off, lay.a3_strides) if which == "a3" else (lay.dh_off, lay.dh_strides)
    if exchange:
        outer, inner = inner, outer
    return off + (bb // lay.nb_inner) * outer + k * head + (bb % lay.nb_inner) * inner


def block_of(lay, which, bb, k, exchange=False):
    """numpy view of a block, through the strides."""
    o = block_offset(lay, which, bb, k, exchange)
    n = lay.X if which == "a3" else lay.Y
    return lay.buf[o : o + n]


# ---- references -----------------------------------------------------------------------------------------------------------------
def gradient(a3, dh, dtype=np.float64, blocks=None):
    """G [K, F, J].  fp64: one product over all samples.  float32: block after block, in block order, each block's product
    and the running sum in float32 -- the yardstick of what float32 accumulation can deliver on these inputs.
    ``blocks``: the block indices to sum (default every block once; the host test passes wrong lists)."""
    nb_total, K = a3.shape[:2]
    blocks = range(nb_total) if blocks is None else blocks
    F, J = a3.shape[2], dh.shape[2]
    G = np.zeros((K, F, J), dtype)
    for k in range(K):
        if dtype == np.float64:
            A = np.concatenate([a3[bb, k] for bb in blocks], axis=1).astype(np.float64)
            D = np.concatenate([dh[bb, k] for bb in blocks], axis=1).astype(np.float64)
            G[k] = A @ D.T
        else:
            for bb in blocks:
                G[k] += a3[bb, k].astype(dtype) @ dh[bb, k].astype(dtype).T
    return G


def adam_from_gradient(G, theta, mu, nu, count, lr=LR, eps=EPS, dtype=np.float64):
    from oracle import qnet_ref as Q

    out = [np.empty(G.shape, dtype) for _ in range(3)]
    for k in range(G.shape[0]):
        t, m, v = Q.adam_update(theta[k].astype(dtype), G[k].astype(dtype), mu[k].astype(dtype), nu[k].astype(dtype), count[k], lr, eps, dtype)
        out[0][k], out[1][k], out[2][k] = t, m, v
    return out


def reference_update(a3, dh, theta, mu, nu, count, lr=LR, eps=EPS, dtype=np.float64, blocks=None):
    """(theta', mu', nu', G), each [K, F, J]: a3 [nb_total, K, F, 32], dh [nb_total, K, J, 32], state [K, F, J], count [K]."""
    G = gradient(a3, dh, dtype, blocks)
    return tuple(adam_from_gradient(G, theta, mu, nu, count, lr, eps, dtype)) + (G,)


def recovered_gradient(mu_new, mu_old):
    """The gradient a step used, read back from its first moment (fp64 arithmetic on the stored float32 values):
    mu' = b1 mu + (1 - b1) g.  From zero moments this is mu' / (1 - b1)."""
    return (np.asarray(mu_new, np.float64) - B1 * np.asarray(mu_old, np.float64)) / (1 - B1)


def errors(got, want, mu_old):
    """Per head k: the three figures the bars apply to.  got / want: (theta', mu', nu'[, G]); want in fp64.
    "nu": |nu' - nu'_ref| minus the part a gradient error of the gradient bar explains is what the nu bar limits, see bars()."""
    g_got, g_want = recovered_gradient(got[1], mu_old), recovered_gradient(want[1], mu_old)
    K = g_want.shape[0]
    return {"grad": np.array([np.abs(g_got[k] - g_want[k]).max() for k in range(K)]),
            "theta": np.array([np.abs(got[0][k].astype(np.float64) - want[0][k]).max() for k in range(K)]),
            "nu": np.array([nu_excess(got[2][k], want[2][k], g_want[k]).max() for k in range(K)])}


def nu_excess(nu_got, nu_want, g_want):
    """nu' = b2 nu + (1 - b2) g^2.  A gradient within d = GRAD_BAR * max |G[k]| of the exact one moves nu' by at most
    (1 - b2) (2 |g| d + d^2); storing nu' in float32 after a multiply and a fused multiply-add adds at most 2^-22 |nu'|
    (two roundings of half an ulp, 2^-24 relative each, with a factor two of slack for the products' own roundings).
    Returned: |error| divided by that allowance -- at most 1 where nu' is as good as the gradient bar permits."""
    d = GRAD_BAR * np.abs(g_want).max()
    allow = (1 - B2) * (2 * np.abs(g_want) * d + d * d) + 2.0 ** -22 * np.abs(nu_want) + 1e-300
    return np.abs(nu_got.astype(np.float64) - nu_want) / allow


def bars(want, mu_old, f32_errs):
    """Per head: the bar of each figure of errors().  Primary: gradient 2e-5 max |G[k]|, theta 3e-7, nu allowance 1.
    A figure that misses its primary bar is held to 4 x the float32 reference's own error on the same row instead
    (the rule of tests/impala_shapes.py::f32_errors), i.e. the bar in force is max(primary, 4 x float32 error)."""
    g = recovered_gradient(want[1], mu_old)
    K = g.shape[0]
    primary = {"grad": np.array([GRAD_BAR * np.abs(g[k]).max() for k in range(K)]), "theta": np.full(K, THETA_BAR), "nu": np.ones(K)}
    return primary, {q: np.maximum(primary[q], 4 * f32_errs[q]) for q in primary}


# ---- synthetic factors ----------------------------------------------------------------------------------------------------------
def _seed(case):
    return [F_OF[case.geom], case.K, case.J, case.nb_total, case.nb_inner, ("plain", "dead", "warm").index(case.family)]


def factors(case):
    """(a3 [nb_total, K, F, 32] >= 0 with exact zeros, dh [nb_total, K, J, 32] of both signs) float32, a few scales: the heads'
    dL/dh differ by up to 50 x (the gradient bar is per head), the blocks' by up to 4 x (every block stays far above the bar, so
    a block left out or taken twice cannot hide)."""
    rng = np.random.default_rng(_seed(case))
    F, K, J, nb = F_OF[case.geom], case.K, case.J, case.nb_total
    a3 = np.maximum(rng.standard_normal((nb, K, F, 32), dtype=np.float32) - 0.3, 0)  # post-ReLU: about 62 % exact zeros
    dh = rng.standard_normal((nb, K, J, 32), dtype=np.float32)
    head_scale = np.array([2e-3, 2e-4, 1e-2, 5e-4, 4e-3, 1e-3], np.float32)[np.arange(K) % 6]
    block_scale = np.array([1.0, 0.5, 2.0], np.float32)[np.arange(nb) % 3]
    dh *= head_scale[None, :, None, None] * block_scale[:, None, None, None]
    a3 *= np.array([1.0, 0.25], np.float32)[(np.arange(nb) // 2) % 2][:, None, None, None]
    if case.family == "dead":
        for bb in range(nb):
            if bb % case.nb_inner == case.nb_inner - 1:
                dh[bb, :, :, LIVE_IN_DEAD_BLOCK:] = 0.0
                a3[bb, :, :, LIVE_IN_DEAD_BLOCK:] += np.float32(0.125)  # biases reach the dead columns: nothing but dL/dh = 0 protects G
    return a3, dh


def state(case):
    """(theta, mu, nu [K, F, J] float32, count [K]) before the step: cold (zero moments, count 0), or for the warm family
    moments of the size a long run leaves (mu ~ the gradient's scale, nu ~ its square) at count 10 000."""
    rng = np.random.default_rng(_seed(case) + [1])
    F, K, J = F_OF[case.geom], case.K, case.J
    theta = rng.uniform(-0.05, 0.05, (K, F, J)).astype(np.float32)
    if case.family != "warm":
        return theta, np.zeros((K, F, J), np.float32), np.zeros((K, F, J), np.float32), np.zeros(K, np.int64)
    a3, dh = factors(case)
    gs = np.abs(gradient(a3, dh)).mean(axis=(1, 2))
    mu = (rng.standard_normal((K, F, J)) * gs[:, None, None] * 0.5).astype(np.float32)
    nu = (rng.uniform(0.3, 1.5, (K, F, J)) * gs[:, None, None] ** 2).astype(np.float32)
    return theta, mu, nu, np.full(K, WARM_COUNT, np.int64)


_REF = {}


def reference(case):
    """{"want": fp64 (theta', mu', nu', G), "f32": the float32 reference's errors(), "primary" / "bars": bars()}; computed once."""
    if case not in _REF:
        a3, dh = factors(case)
        theta, mu, nu, count = state(case)
        want = reference_update(a3, dh, theta, mu, nu, count)
        f32 = errors(reference_update(a3, dh, theta, mu, nu, count, dtype=np.float32), want, mu)
        primary, inforce = bars(want, mu, f32)
        _REF[case] = {"want": want, "f32": f32, "primary": primary, "bars": inforce}
        if len(_REF) > 4:  # the large cases are not kept around
            _REF.pop(next(iter(_REF)))
    return _REF[case]


# ---- several ranks on one GPU ---------------------------------------------------------------------------------------------------
Gathered = collections.namedtuple("Gathered", "a3_all dh_all nb_total nb_inner finish_args td_abs")


def emulate_ranks(agent, batch, R, weights=None):
    """What R ranks compute up to the gathered factors, on one GPU: the batch is cut into R equal shards; per shard the first
    half of the step (mean divisor = the global batch), the export of its factors to where all_gather would put them
    (``[rank][head][block]``), the conv backward (idqn_backward_rest), and the sum of the small-leaf gradient regions (what the
    all-reduce does; the K losses live there).  Leaves the summed region in the agent and returns the gathered factors with the
    arguments of ``idqn_finish_step_factored`` up to ``phases``.  ``weights`` [B]: importance weights through
    idqn_set_per_buffers; the |TD| of every shard come back as ``td_abs`` [K, B]."""
    import torch

    from slimdqn import _hip

    lib, q = _hip.lib(), _hip.current_stream
    K = agent._K
    F, J = next(shape for n, _, shape in agent._leaves if n == "Dense_0/kernel")
    B = len(np.asarray(batch.action))
    assert B % R == 0
    b = B // R
    nb = -(-b // 32)
    X, Y = F * 32, J * 32
    a3_all = torch.empty(R * K * nb * X, dtype=torch.float32, device="cuda")
    dh_all = torch.empty(R * K * nb * Y, dtype=torch.float32, device="cuda")
    small = torch.zeros_like(agent._grad_small)
    Shard = type(batch)
    td_abs = None
    if weights is not None:
        agent._ensure_handle(b)
        w_dev = torch.from_numpy(np.ascontiguousarray(weights, np.float32)).cuda()
        td_dev = torch.zeros((R, K, b), dtype=torch.float32, device="cuda")
    for r in range(R):
        shard = Shard(*[np.asarray(f)[b * r : b * (r + 1)] for f in batch])
        if weights is not None:
            _hip.check(lib.idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev[b * r :]), _hip.ptr(td_dev[r])), "set")
        agent._learn(shard, flags=_hip.F_STOP_BEFORE_DENSE0_WGRAD, mean_divisor=B)
        _hip.check(lib.idqn_export_dense0_factors(agent._handle, _hip.ptr(a3_all[r * K * nb * X :]),
                                                  _hip.ptr(dh_all[r * K * nb * Y :]), q()), "export")
        _hip.check(lib.idqn_backward_rest(agent._handle, q()), "rest")
        small += agent._grad_small  # what the all-reduce of the small-leaf region does
    if weights is not None:
        _hip.check(lib.idqn_set_per_buffers(agent._handle, None, None), "clear")
        td_abs = td_dev.permute(1, 0, 2).reshape(K, B).cpu().numpy()
    agent._grad_small.copy_(small)
    args = (agent._handle, _hip.ptr(a3_all), _hip.ptr(dh_all), R * nb, nb, K * nb * X, nb * X, X, K * nb * Y, nb * Y, Y)
    return Gathered(a3_all, dh_all, R * nb, nb, args, td_abs)


# ---- the end-to-end rows ----------------------------------------------------------------------------------------------------------
E2E_K, E2E_GAMMA, E2E_LR, E2E_EPS = 2, 0.99, LR, EPS
E2E_SHARDS = [(3, 32), (2, 64), (2, 40), (5, 40)]  # ranks x samples per rank; the last: nb_total = 10, nb_inner = 2, ragged
# Seeds of (parameters, target parameters, batch) follow from (J, ranks, shard) in e2e_inputs; with them the float32 run of the
# oracle meets every bar on every element against the fp64 run (tests/test_factored_shapes_host.py asserts it).  A row whose
# float32 run ever misses gets its seed here.
E2E_SEEDS = {}


def e2e_inputs(J, R, b):
    from oracle import qnet_ref as Q

    obs, convs = GEOMS["G1"]
    feats = convs + [J]
    s = E2E_SEEDS.get((J, R, b), 100 + J + 7 * R + b)
    p = Q.init_params(s, "cnn", obs, N_ACTIONS, feats, E2E_K)
    pt = Q.init_params(s + 1, "cnn", obs, N_ACTIONS, feats, E2E_K)
    rng = np.random.default_rng(s + 2)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = list(Q.synthetic_batch(s + 3, R * b, obs, N_ACTIONS, "cnn"))
    batch[4][(R * b) // 2] = True
    return obs, feats, p, pt, tuple(batch)


def e2e_oracle(J, R, b, dtype=np.float64, steps=1, weights=None):
    """[(params, mu, nu, losses, grads)] after each of ``steps`` chained steps on the same batch, from cold Adam state."""
    from oracle import qnet_ref as Q

    obs, feats, p, pt, batch = e2e_inputs(J, R, b)
    params = {n: v.astype(dtype) for n, v in p.items()}
    mu = {n: np.zeros(v.shape, dtype) for n, v in p.items()}
    nu = {n: np.zeros(v.shape, dtype) for n, v in p.items()}
    count = np.zeros(E2E_K, np.int64)
    out = []
    for _ in range(steps):
        if weights is None:
            params, mu, nu, count, losses, grads = Q.learn_on_batch(params, pt, mu, nu, count, batch, "cnn", E2E_GAMMA, E2E_LR, E2E_EPS,
                                                                    dtype, return_grads=True)
        else:  # (learn_on_batch has no weights argument: the same loop with the weighted loss)
            grads = {n: np.zeros(a.shape, dtype) for n, a in params.items()}
            losses = np.zeros(E2E_K, dtype)
            new = ({n: a.copy() for n, a in params.items()}, {n: a.copy() for n, a in mu.items()}, {n: a.copy() for n, a in nu.items()})
            for k in range(E2E_K):
                losses[k], g, _ = Q.loss_and_grads(Q.head(params, k), Q.head(pt, k), batch, "cnn", E2E_GAMMA, dtype, weights=weights)
                for n in params:
                    grads[n][k] = g[n]
                    new[0][n][k], new[1][n][k], new[2][n][k] = Q.adam_update(params[n][k], g[n].astype(dtype), mu[n][k], nu[n][k], count[k],
                                                                             E2E_LR, E2E_EPS, dtype)
            params, mu, nu = new
            count = count + 1
        out.append((params, mu, nu, losses, grads))
    return out
