"""The persistent conv kernel (csrc/convp_pp.hip) at frames other than 84x84: the table of shapes, the child process that runs
one row, and the parser of the library's ``[plan]`` lines.  A plain helper module like ``tests/cnn_stages.py``;
``tests/test_gpu_conv_pp_shapes.py`` runs the rows on the GPU, ``tests/test_conv_pp_shapes_host.py`` checks this file itself.

Which kernel ran is read off the shipped library: with ``IDQN_PLAN_PRINT`` set it prints ``[plan] fwd role R ...`` for every
one-item plan it makes and ``[plan] pp role R nets N nb NB: parts P -> I items on W workgroups, NT T, ring G, ...`` when the
persistent plan of a role was chosen (``plan_fwd`` / ``plan_fwd_pp`` in csrc/qnet.hip).  The switches are read once per process,
so every row runs in child processes (``run_child``).

Roles: 0..2 forward of Conv_0..2, 3 data gradient of Conv_2, 4 data gradient of Conv_1.  A role goes persistent when its
one-item plan has more than 256 items and its bit is set in ``IDQN_CONV_PP`` -- whose DEFAULT is 15, roles 0..3: the Conv_1
data gradient (role 4) measured flat and stays on the one-item launch unless ``IDQN_CONV_PP=31`` asks for it.  Rows that cover
role 4 therefore run their persistent child with ``IDQN_CONV_PP=31`` (``Row.pp_mask``); the other rows run it with the
default environment, where role 4 is pinned NOT persistent.  The second child of every row runs with ``IDQN_CONV_PP=0``.

Every pinned plan is (parts, NT, ring, n_items, n_wg); ``None``: the role does not run the persistent kernel in that row.
``paired``: whether the data gradient and the weight gradient of Conv_1 / Conv_2 ran as ONE launch (convp_pair.hip; the data
gradient then is no launch of its own and has no plan of role 4 / 3 at all).

Classes (the host test derives them from the pinned values with ``classes_of`` and asserts that none is empty):
  1    role r persistent at a frame other than 84x84              r0..r3: every training row; r4: rows 0, 3, 4, 5
  2    parts = 1 | parts >= 2 with OW % parts != 0                parts 1: rows 0, 1, 2, 4, 5; uneven: row 2 (r1: 7 columns in 2),
                                                                   row 3 (r1: 9 in 2, r2: 9 in 4, r4: 9 / 9 / 9 / 9 .. in 2)
  3    NT = 2 through the floor | NT = 4 | Conv_0 with NT 5 or 6  floor: row 0 (r4), row 1 (r3), row 4 (r3, r4); NT 4: row 2
                                                                   (r0, r2, r3); Conv_0 NT 5: row 3 (18 output columns, parts 1)
  4    ring 2 | ring 3                                            ring 2: r1 of every row that has it; ring 3: the others
  5    role 4 with an odd Conv_1 input | an even x even one       odd: row 0 (5x5), row 3 (3x18: odd x even); even: row 4 (4x8)
  6    n_items % 8 != 0 | n_items % n_wg != 0 | 256 < n_items < 512 | >= 3 items per workgroup
                                                                   % 8: row 1 (990, 540, 810: 5 sample blocks, 9 heads);
                                                                   256..512: row 0 (r3: 408), row 3 (r0: 270, r1: 360);
                                                                   >= 3: row 0 (1360), row 1 (990), row 2 (880, 960), row 4
  7    B % 32 != 0 on a persistent row                            rows 0, 1, 3, 4, 5 (250 and 130)
  8a   a width mix whose template is not built                    row 5: [32, 32, 64]: roles 1 (CT 1, NQ 4) and 3 (CT 1, NQ 3)
                                                                   stay on the one-item launch, roles 0, 2, 4 go persistent --
                                                                   with 6 (role 2) and 4 (role 4) supersteps instead of 12 and 8
  8b   a role whose candidates are ALL refused                    unreachable, see UNREACHABLE
  9    the acting set (``role + 8``)                              ACT_ROW, through the i-IQN handle; see its comment
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, N_STEP, LR, EPS = 0.97, 3, 1e-3, 1e-6  # as tests/test_gpu_conv_geometry.py
GAMMA_N = GAMMA ** N_STEP
CHILD_TIMEOUT = 120  # seconds, per child
SMALL_B = 20         # the step in between of the plan-switching sequence: one sample block, one-item plans
CUS = 256            # cu_budget() of csrc/qnet.hip

Row = namedtuple("Row", "obs feats A K B pp_mask plans paired seed")
P = lambda parts, NT, ring, n_items, n_wg: (parts, NT, ring, n_items, n_wg)  # noqa: E731

TABLE = [
    # 0: 5x5 -> 3x3 -> 3x3; 136 / 272 slots of 3..5 rows each.  All five roles; role 3 has 408 items on 256 workgroups (some run
    #    one item, some two); role 4's variants are 3x3, 3x2, 2x3, 2x2 (np_max 3, CT 1: the NT floor); 250 = 7 x 32 + 26
    Row((17, 17, 4), [32, 64, 64, 128], 4, 17, 250, "31",
        (P(1, 2, 3, 1360, 256), P(1, 2, 2, 816, 256), P(1, 2, 3, 816, 256), P(1, 2, 3, 408, 256), P(1, 2, 3, 1360, 256)),
        {"conv1": False, "conv2": False}, 5),
    # 1: 11x11 -> 6x6 -> 6x6, five sample blocks (the last with 2 samples), nine heads: item counts that are no multiple of 8;
    #    role 3 cuts its 6 columns in 3 (np 2, CT 2: the floor again); default environment: role 4 stays one-item
    Row((41, 41, 4), [32, 64, 64, 128], 5, 9, 130, None,
        (P(1, 3, 3, 990, 256), P(1, 3, 2, 540, 256), P(1, 3, 3, 540, 256), P(3, 2, 3, 810, 256), None),
        {"conv1": False, "conv2": False}, 4),
    # 2: 11x13 -> 6x7 -> 6x7, eight full blocks: NT 4 for Conv_0 (13 columns), Conv_2 and its data gradient (7 columns, CT 2);
    #    Conv_1 cuts its 7 columns in 4 + 3; role 3 has 240 items: the persistent kernel with ONE item on every workgroup
    Row((43, 49, 4), [32, 64, 64, 128], 6, 5, 256, None,
        (P(1, 4, 3, 880, 256), P(2, 2, 2, 960, 256), P(1, 4, 3, 480, 256), P(1, 4, 2, 240, 240), None),
        {"conv1": False, "conv2": False}, 3),
    # 3: 3x18 -> 2x9 -> 2x9: Conv_0 with 18 columns in one part (NT 5); 9 columns in 2 and in 4 parts; role 4 over an
    #    odd x even input (variants 2x9, 2x9, 1x9, 1x9) in 5 + 4 columns; Conv_2's gradients run paired
    Row((9, 69, 4), [32, 64, 64, 128], 3, 9, 130, "31",
        (P(1, 5, 3, 270, 256), P(2, 3, 2, 360, 256), P(4, 2, 3, 720, 256), None, P(2, 2, 3, 540, 256)),
        {"conv1": False, "conv2": True}, 0),
    # 4: 4x8 -> 2x4 -> 2x4: role 4 over an even x even input (four variants of 2x4)
    Row((13, 30, 4), [32, 64, 64, 128], 4, 17, 250, "31",
        (P(1, 2, 3, 1088, 256), P(1, 2, 2, 544, 256), P(1, 2, 3, 544, 256), P(2, 2, 3, 544, 256), P(1, 2, 3, 1088, 256)),
        {"conv1": False, "conv2": False}, 5),
    # 5: row 0's frame with Conv_1 32 wide: <3, 1, 4, .> (role 1) and <3, 1, 3, .> (role 3) are not built
    Row((17, 17, 4), [32, 32, 64, 128], 4, 17, 250, "31",
        (P(1, 2, 3, 1360, 256), None, P(1, 2, 3, 816, 256), None, P(1, 2, 3, 1360, 256)),
        {"conv1": False, "conv2": False}, 0),
]
IDS = ["%dx%d-%s-K%d-B%d" % (r.obs[0], r.obs[1], "x".join(map(str, r.feats[:3])), r.K, r.B) for r in TABLE]

# Class 9.  ``idqn_q_values`` takes at most 32 states: ONE slot, whose one-item plan passes 256 items only when Conv_0 has more
# than 256 x 24 output positions (nt_max 6, CT 1) or Conv_1 / Conv_2 more than 256 x 6 -- frames of about 316x316 and up, so
# no frame up to 128x128 reaches the persistent kernel through it.  ``idqn_iqn_q_values`` (i-IQN handles) takes up to
# max_batch = 256 states on the same acting set: 8 slots, and from 112x112 on (28x28 -> 14x14 -> 14x14) all three forward
# plans have 264 items and go persistent.  That row: K = 1, 250 states (a ragged eighth block), 8 fractions.
ActRow = namedtuple("ActRow", "obs feats A K n n_quantiles plans")
ACT_ROW = ActRow((112, 112, 4), [32, 64, 64, 256], 4, 1, 250, 8,
                 (P(2, 4, 3, 448, 256), P(4, 2, 2, 448, 256), P(2, 4, 3, 224, 224)))

# Class 8b, from plan_fwd_pp: a candidate `parts` is refused when its template is not built, when NSS - 1 < NT or when
# ring x stage + epilogue slots pass 160 KB.  For a BUILT (NPA, CT, NQ) the candidate parts = OW always exists: np_max = 1,
# NT = 2 (the floor), and NSS = KH x NCC is 8 (Conv_0), 2 x CI / 16 >= 4 (roles 1, 4), 3 x C / 16 >= 6 (roles 2, 3) for widths
# of 32 or 64, so NSS - 1 >= 3 > NT; its stage is at most (4 x 2 x 3 + 4 x 3) KB = 36 KB (role 1), two of them plus the
# largest epilogue (4 x (6 KB + 2 x 2 KB) = 40 KB) fit 160 KB.  So a role either has no template at all (8a) or a plan.
UNREACHABLE = {"8b.all_refused": "for a built (NPA, CT, NQ) the candidate parts = OW (NT 2, one position per item) always "
                                 "fits: NSS - 1 >= 3 and 2 x 36 KB + 40 KB <= 160 KB"}

CLASSES = ["1.r0", "1.r1", "1.r2", "1.r3", "1.r4", "2.parts1", "2.uneven", "3.floor", "3.nt4", "3.conv0_nt56", "4.ring2",
           "4.ring3", "5.odd", "5.even", "6.mod8", "6.mod_wg", "6.one_or_two", "6.three", "7.ragged", "8a.unbuilt",
           "8b.all_refused", "9.acting"]


# ---- the oracle-side geometry of a role ---------------------------------------------------------------------------------
def role_shape(obs, feats, role):
    """(CT, NPA, NQ, [(OH, OW) of every variant]) of a role, from ``cnn_stages.geometry`` (role_geom in csrc/qnet.hip)."""
    import cnn_stages as S

    geo = S.geometry(obs, feats)
    f0, f1, f2 = feats[:3]
    if role <= 2:
        g = geo[role]
        return ([f0, f1, f2][role] // 32, 1 if role == 0 else 3, [2, 4, 3][role], [(g["OH"], g["OW"])])
    if role == 3:  # stride 1: one variant, the extent of Conv_2's input
        return (f1 // 32, 3, 3, [(geo[2]["IH"], geo[2]["IW"])])
    g = geo[1]     # stride 2: four parities of Conv_1's input
    return (f0 // 32, 3, 2, [((g["IH"] - rh + 1) // 2, (g["IW"] - rw + 1) // 2) for rh in (0, 1) for rw in (0, 1)])


def pp_built(NPA, CT, NQ, NT):
    """convp_pp_built of csrc/convp_pp.hip."""
    return (NPA, CT, NQ) in ((1, 1, 2), (3, 2, 4), (3, 2, 3), (3, 1, 2)) and 2 <= NT <= (6 if NPA == 1 else 4)


def n_slots(role, K, n_samples, acting=False):
    nb = (n_samples + 31) // 32
    return (1 if acting else 2 * K if role <= 2 else K) * nb


def implied(obs, feats, role, parts, slots):
    """(n_items, raw tiles per wave before the floor, any OW % parts != 0) that `parts` column ranges per output row imply."""
    CT, _, _, var = role_shape(obs, feats, role)
    np_max = max((ow + parts - 1) // parts for _, ow in var)
    return slots * sum(oh * parts for oh, _ in var), (np_max * CT + 3) // 4, any(ow % parts for _, ow in var)


def classes_of(row):
    """The classes of the module docstring that a training row's PINNED values claim."""
    import cnn_stages as S

    out = set()

    g1 = S.geometry(row.obs, row.feats)[1]
    for role, plan in enumerate(row.plans):
        if plan is None:
            continue
        parts, NT, ring, n_items, n_wg = plan
        _, raw_nt, uneven = implied(row.obs, row.feats, role, parts, n_slots(role, row.K, row.B))
        if row.obs[:2] != (84, 84) and row.feats[:3] == [32, 64, 64]:
            out.add("1.r%d" % role)
        out.add("2.parts1" if parts == 1 else "2.uneven" if uneven else "2.even_parts")
        if raw_nt < 2 and NT == 2:
            out.add("3.floor")
        if NT == 4:
            out.add("3.nt4")
        if role == 0 and NT in (5, 6):
            out.add("3.conv0_nt56")
        out.add("4.ring%d" % ring)
        if role == 4:
            out.add("5.odd" if (g1["IH"] % 2 or g1["IW"] % 2) else "5.even")
        if n_items % 8:
            out.add("6.mod8")
        if n_items % n_wg:
            out.add("6.mod_wg")
        if 256 < n_items < 512:
            out.add("6.one_or_two")
        if n_items >= 3 * n_wg:
            out.add("6.three")
        if row.B % 32:
            out.add("7.ragged")
    if any(p is None for p in row.plans) and any(p is not None for p in row.plans):
        for role, plan in enumerate(row.plans):
            CT, NPA, NQ, _ = role_shape(row.obs, row.feats, role)
            if plan is None and not any(pp_built(NPA, CT, NQ, nt) for nt in range(2, 7)):
                out.add("8a.unbuilt")
    return out


# ---- the library's plan lines ---------------------------------------------------------------------------------------------
_FWD = re.compile(r"^\[plan\] fwd role (\d+) nets (\d+) nb (\d+) target (\d+): (\d+) workgroups, NT (\d+), ring (\d+), stage (\d+) B, "
                  r"lds (\d+) B, supersteps (\d+), ranges/slot (\d+) \(NPA (\d+) CT (\d+) NQ (\d+)\)$")
_PP = re.compile(r"^\[plan\] pp role (\d+) nets (\d+) nb (\d+): parts (\d+) -> (\d+) items on (\d+) workgroups, NT (\d+), ring (\d+), "
                 r"stage (\d+) B, lds (\d+) B$")
_PP_CANDIDATE = re.compile(r"^\[plan\] pp role (\d+) parts (\d+): (\d+) items, NT (\d+), ring (\d+), stage (\d+) B, lds (\d+) B, model \d+ k cycles$")
_FWD_KEYS = "role nets nb target n_items NT ring stage lds supersteps ranges NPA CT NQ".split()
_PP_KEYS = "role nets nb parts n_items n_wg NT ring stage lds".split()


def parse_plan_lines(text):
    """{"fwd": [dict], "pp": [dict], "candidates": n, "unknown": [line]} of a child's stderr.  "fwd": every one-item plan made
    (role 8..10: the acting set's; target 128: planned for a paired launch); "pp": every persistent plan CHOSEN (the lines
    that name nets and nb; its role is printed without the acting bit); "unknown": ``[plan] fwd`` / ``[plan] pp`` lines that
    match none of the formats -- a changed fprintf must fail the tests, not silently empty the lists."""
    out = {"fwd": [], "pp": [], "candidates": 0, "unknown": []}
    for line in text.splitlines():
        line = line.strip()
        if not (line.startswith("[plan] fwd ") or line.startswith("[plan] pp ")):
            continue
        m = _FWD.match(line)
        if m:
            out["fwd"].append(dict(zip(_FWD_KEYS, map(int, m.groups()))))
            continue
        m = _PP.match(line)
        if m:
            out["pp"].append(dict(zip(_PP_KEYS, map(int, m.groups()))))
            continue
        if _PP_CANDIDATE.match(line):
            out["candidates"] += 1
            continue
        out["unknown"].append(line)
    return out


def chosen_plans(parsed, nb, roles=range(5)):
    """Per role: (parts, NT, ring, n_items, n_wg) of the persistent plan chosen for launches of `nb` sample blocks, or None
    when the role has no such line (it ran the one-item launch, or inside a paired launch)."""
    out = []
    for role in roles:
        hits = [p for p in parsed["pp"] if p["role"] == role and p["nb"] == nb]
        assert len(hits) <= 1, ("a plan is made once per handle", hits)
        out.append(P(hits[0]["parts"], hits[0]["NT"], hits[0]["ring"], hits[0]["n_items"], hits[0]["n_wg"]) if hits else None)
    return tuple(out)


def paired_routes(profile_rows):
    """{"conv1": bool, "conv2": bool} from the launch names of ``idqn_profile_table``: True when the layer's data gradient and
    weight gradient ran as one launch."""
    names = set(profile_rows)
    out = {}
    for layer in ("conv1", "conv2"):
        pair, sep = layer + " dgrad + wgrad" in names, {layer + " dgrad", layer + " wgrad"} <= names
        assert pair != sep, (layer, sorted(names))
        out[layer] = pair
    return out


# ---- digests ------------------------------------------------------------------------------------------------------------------
def digest(a):
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def digests(arrays, prefix=""):
    return {prefix + n: digest(a) for n, a in arrays.items()}


def differing(da, db, prefix_a="", prefix_b=""):
    """Names (without prefix) whose digests differ or that only one side has."""
    a = {n[len(prefix_a):]: v for n, v in da.items() if n.startswith(prefix_a)}
    b = {n[len(prefix_b):]: v for n, v in db.items() if n.startswith(prefix_b)}
    return sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))


class Recorded:
    """What ``cnn_stages.stage_errors`` / ``border_report`` read of an agent, served from the arrays a child saved."""

    class _Host:
        def __init__(self, a):
            self._a = a

        def cpu(self):
            return self

        def numpy(self):
            return self._a

    def __init__(self, arrays):
        self._arrays = arrays

    def _debug(self, name):
        return Recorded._Host(self._arrays["first/" + name])

    def _flat_grad(self):
        return {n[len("leafgrad/"):]: a for n, a in self._arrays.items() if n.startswith("leafgrad/")}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def inputs(obs, feats, A, K, B, seed=0):
    """Parameters and one batch, built as tests/test_gpu_conv_geometry.py::_inputs builds them (nonzero biases, one terminal
    sample); `seed` shifts every generator."""
    from oracle import qnet_ref as Q

    p = Q.init_params(3 + seed, "cnn", obs, A, feats, K)
    pt = Q.init_params(4 + seed, "cnn", obs, A, feats, K)
    rng = np.random.default_rng(5 + seed)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    batch = list(Q.synthetic_batch(6 + seed, B, obs, A, "cnn"))
    batch[4][B // 2] = True
    return p, pt, tuple(batch)


def act_inputs(row, seed=0):
    """Parameters (nonzero biases), states and fractions [N, n] of the acting row."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    p = I.init_params(3 + seed, row.obs, row.A, row.feats, row.K)
    rng = np.random.default_rng(5 + seed)
    for n in p:
        if n.endswith("bias"):
            p[n] = (0.05 * rng.standard_normal(p[n].shape)).astype(np.float32)
    states = Q.synthetic_batch(6 + seed, row.n, row.obs, row.A, "cnn")[0]
    tau = rng.random((row.n_quantiles, row.n)).astype(np.float32)
    return p, states, tau


def fp32_restatement_error(row):
    """(largest relative error, its stage) of the oracle evaluated in numpy fp32 against the oracle in fp64, over the backward
    stages and leaf gradients of every head of a row's inputs -- the reference's own error in the device's number format.

    A row has 10^6 .. 10^7 ReLU units.  One whose pre-activation is a few 1e-9 of the layer's largest lands on either side of
    zero depending on how an fp32 sum is ordered, and an entry of the layer's gradient -- up to the stage's largest -- then appears
    or vanishes whatever kernel computes it: on such inputs the fp64 derivative is no reference for ANY fp32 computation.  So a
    row's inputs are admissible only if (a) plain numpy fp32 arithmetic meets STAGE_BAR on them and (b) ``relu_exposure`` is
    below STAGE_BAR; ``Row.seed`` is the smallest seed shift (``inputs``) at which both hold, and the host test asserts both.  Seed 0 of row 2: numpy fp32 misses d_conv2 of head 3 by
    1.66e-3 -- a Conv_2 unit at 7.0e-9 of the largest -- and the device's da3 of that head is off by the same 1.66e-3, with every
    forward stage within 2e-6 and every byte equal to the one-item launches'.  Seed 0 of row 0: d_conv2 of head 13 by 0.17."""
    from oracle import qnet_ref as Q

    import cnn_stages as S

    p, pt, batch = inputs(row.obs, row.feats, row.A, row.K, row.B, row.seed)
    worst = (0.0, "")
    for k in range(row.K):
        _, g64, a64 = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N)
        _, g32, a32 = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", np.float32(GAMMA_N), dtype=np.float32)
        errs = {"h%d_%s" % (k, key): S.relerr(a32["trace"][key].astype(np.float64), a64["trace"][key])
                for key in ("d_dense0", "d_conv2", "d_conv1", "d_conv0")}
        errs.update({"h%d_grad_%s" % (k, leaf): S.relerr(g32[leaf].astype(np.float64), g64[leaf]) for leaf in g64})
        name = max(errs, key=errs.get)
        if errs[name] > worst[0]:
            worst = (errs[name], name)
    return worst


RELU_TAU = 2.0 ** -24


def relu_exposure(row):
    """(b) of ``fp32_restatement_error``: the largest gradient ARRIVING at a ReLU unit whose fp64 pre-activation lies within
    RELU_TAU (half an fp32 ulp) of the layer's largest pre-activation of zero, relative to the largest entry of that layer's
    gradient stage, over the four ReLU layers and every head -- as (value, stage).  Partial sums of the layer's magnitude are
    rounded with that absolute granularity, so two fp32 summation orders need not agree on the sign of such a unit (numpy's and
    the device's do not: seed shift 2 of row 0 passes (a), and the device's da1 of head 14 is off by 4.4e-3); if it flips, the
    stage moves by exactly the gradient arriving at it."""
    from oracle import qnet_ref as Q

    p, pt, batch = inputs(row.obs, row.feats, row.A, row.K, row.B, row.seed)
    x0 = batch[0].astype(np.float64) / 255.0
    worst = (0.0, "")
    for k in range(row.K):
        aux = Q.loss_and_grads(Q.head(p, k), Q.head(pt, k), batch, "cnn", GAMMA_N)[2]
        tape, tr = aux["tape"], aux["trace"]
        w = lambda n: p[n][k].astype(np.float64)  # noqa: E731
        pre = []
        for li in range(3):
            a_in = x0 if li == 0 else tape[li - 1][4]
            pre.append(Q.conv_fwd(a_in, w(f"Conv_{li}/kernel"), w(f"Conv_{li}/bias"), Q.CNN_GEOM[li][1])[0])
        pre.append(tape[3][2] @ w("Dense_0/kernel") + w("Dense_0/bias"))
        for li, key in enumerate(("d_conv0", "d_conv1", "d_conv2", "d_dense0")):
            near = np.abs(pre[li]) <= RELU_TAU * np.abs(pre[li]).max()
            if not near.any():
                continue
            if li < 2:    # what arrives at Conv_li's units: the input gradient of Conv_{li+1}
                g = Q.conv_bwd(tape[li + 1][2], tape[li + 1][3], w(f"Conv_{li + 1}/kernel"), Q.CNN_GEOM[li + 1][1], tr[f"d_conv{li + 1}"])[0]
            elif li == 2:
                g = tr["d_dense0"] @ w("Dense_0/kernel").T
            else:
                g = tr["d_dense1"] @ w("Dense_1/kernel").T
            e = float(np.abs(g.reshape(pre[li].shape)[near]).max() / np.abs(tr[key]).max())
            if e > worst[0]:
                worst = (e, "h%d_%s" % (k, key))
    return worst


# ---- the child ------------------------------------------------------------------------------------------------------------------
DEBUG_NAMES = ("a1p", "a2p", "a3", "da3p", "da2p", "da1p", "q", "dh")
STATE_NAMES = ("_grad", "_losses", "_online", "_mu", "_nu", "_cum")


def child_main():
    """One row in this process: PP_SPEC (json) says which.  Training rows: an F_GRADS_ONLY step at B ("first/"), the same
    at SMALL_B, the first again ("third/"), then one full step ("full/").  Prints ``RESULT{json}``: one digest per array, the
    launch names of the first step; saves the arrays the parent compares with the oracle to spec["save"] (if set)."""
    t0 = time.time()
    import ctypes as C

    import torch

    from slimdqn import _hip

    spec = json.loads(os.environ["PP_SPEC"])
    out, save = {}, {}
    if spec["mode"] == "act":
        from slimdqn.networks.iiqn import iIQN

        row = ActRow(tuple(spec["obs"]), spec["feats"], spec["A"], spec["K"], spec["n"], spec["n_quantiles"], None)
        p, states, tau = act_inputs(row, spec["seed"])
        agent = iIQN(0, row.obs, row.A, row.K, row.feats, "cnn", LR, GAMMA, N_STEP, 1, 10**9, 10**9, adam_eps=EPS,
                     n_quantiles=row.n_quantiles)
        agent._load_flat(agent._online, p)
        q = agent.q_values(agent.params, states, 0, taus=tau).cpu().numpy().copy()
        torch.cuda.synchronize()
        arrays = {"act/q": q}
        for name in ("infer_a1p", "infer_a2p", "infer_a3"):
            arrays["act/" + name] = agent._debug(name).cpu().numpy()
        save = {"act/q": q}
        out["digests"] = digests(arrays)
    else:
        from slimdqn.networks.idqn import iDQN

        Batch = namedtuple("Batch", "state action reward next_state is_terminal")
        obs, feats, A, K, B = tuple(spec["obs"]), spec["feats"], spec["A"], spec["K"], spec["B"]
        p, pt, batch = inputs(obs, feats, A, K, B, spec["seed"])
        agent = iDQN(0, obs, A, K, feats, "cnn", LR, GAMMA, N_STEP, 1, 10**9, 10**9, adam_eps=EPS)
        agent._load_flat(agent._online, p)
        agent._load_flat(agent._target, pt)
        agent._ensure_handle(B)  # ONE handle, sized for the large batch, for the whole sequence
        assert agent._w0 != (0, 0) and len(agent._leaves) == 10, "not the matrix-core path's layout"

        def grads_only(b, extra=0):
            agent._learn(Batch(*b), flags=_hip.F_GRADS_ONLY | extra)
            torch.cuda.synchronize()
            snap = {n: agent._debug(n).cpu().numpy() for n in DEBUG_NAMES}
            snap["_grad"] = agent._grad.cpu().numpy().copy()
            snap["_losses"] = agent._losses.cpu().numpy().copy()
            return snap

        first = grads_only(batch, _hip.F_PROFILE_ALL)
        buf = C.create_string_buffer(8192)
        _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, 8192), "idqn_profile_table")
        out["launches"] = [ln.split("\t")[0] for ln in buf.value.decode().splitlines()]
        leafgrad = agent._flat_grad()
        grads_only(tuple(x[:SMALL_B] for x in batch))
        third = grads_only(batch)
        agent._learn(Batch(*batch))
        torch.cuda.synchronize()
        full = {n: getattr(agent, n).cpu().numpy().copy() for n in STATE_NAMES}
        out["count"] = agent._count.cpu().numpy().tolist()
        out["digests"] = {**digests(first, "first/"), **digests(third, "third/"), **digests(full, "full/")}
        save = {"first/" + n: a for n, a in first.items()}
        save.update({"leafgrad/" + n: a for n, a in leafgrad.items()})
        save.update({"online/" + n: a for n, a in agent._flat(agent._online).items()})
        agent._destroy_handle()
    if spec.get("save"):
        np.savez(spec["save"], **save)
    out["seconds"] = round(time.time() - t0, 2)
    print("RESULT" + json.dumps(out))


def spec_of(row, seed=0, save=None):
    if isinstance(row, ActRow):
        return dict(mode="act", obs=row.obs, feats=row.feats, A=row.A, K=row.K, n=row.n, n_quantiles=row.n_quantiles, seed=seed, save=save)
    return dict(mode="train", obs=row.obs, feats=row.feats, A=row.A, K=row.K, B=row.B, seed=seed, save=save)


def run_child(spec, pp=None):
    """Run one row in a fresh process on the shipped library, plan printing on.  pp: the value of IDQN_CONV_PP (None: unset).
    Returns (result dict, parsed plan lines, wall seconds)."""
    env = dict(os.environ)
    for name in ("IDQN_HIP_LIB", "IDQN_CONV_PP", "IDQN_CONV"):
        env.pop(name, None)
    env["IDQN_PLAN_PRINT"] = "1"
    env["PP_SPEC"] = json.dumps(spec)
    if pp is not None:
        env["IDQN_CONV_PP"] = pp
    code = ("import os, sys; sys.path[:0] = [%r, %r, %r]; import conv_pp_shapes; conv_pp_shapes.child_main()"
            % (ROOT, os.path.join(ROOT, "i-dqn_amd"), os.path.join(ROOT, "tests")))
    t0 = time.time()
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    wall = time.time() - t0
    assert done.returncode == 0, "child exited with %s\n%s" % (done.returncode, done.stderr[-3000:])
    line = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):]), parse_plan_lines(done.stderr), wall
