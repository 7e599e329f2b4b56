"""CPU: the shape table of the one-launch MLP step (tests/fc_shapes.py) is what it says it is.

* the constants of the Python restatement of ``fc_par_plan`` / ``fc_steps_plan`` equal the headers', read as text;
* the restated arena layout equals the library's own ``idqn_layout`` for every row (and every head stride is a multiple of 64
  floats, which is why ``P % 4 != 0`` has no row);
* every row's stated reason holds on the restatement, and its expected route is the one the restatement derives;
* the table covers what it is there to cover;
* the fp32 oracle alone stays within HALF of every bar the GPU test applies, for every row: the other half is the kernel's
  different summation order.  A row that fails this is a badly chosen input, not a reason to widen a bar.
"""
import os
import re

import numpy as np
import pytest

import fc_shapes as F

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "i-dqn_amd", "csrc")
IDS = [r.id for r in F.TABLE]
RUN_IDS = [r.id for r in F.RUNNABLE]


def _define(header, name):
    """The value of ``#define name <expr>`` in a header, the expression (integers, + - * and parentheses) evaluated."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*)?$" % re.escape(name), text, re.M)
    assert m, f"{header}: no #define {name}"
    expr = m.group(1)
    assert re.fullmatch(r"[0-9+\-*() ]+", expr), f"{header}: {name} is no plain integer expression: {expr!r}"
    return eval(expr, {"__builtins__": {}})  # noqa: S307  (digits and arithmetic only, checked above)


@pytest.mark.parametrize("header,name", [
    ("fc_par_kernels.h", "FCP_NPT"), ("fc_par_kernels.h", "FCP_LDS_BUDGET"), ("fc_kernels.h", "FCM_T"), ("fc_kernels.h", "FCM_BSP"),
    ("fc_steps_kernels.h", "FCS_ROW_WORDS"), ("fc_kernels.h", "FC_MAX_WIDTH"), ("fc_kernels.h", "FC_LDS_BUDGET"),
])
def test_restated_constants_equal_the_headers(header, name):
    assert getattr(F, name) == _define(header, name)


def test_the_plan_text_the_restatement_follows_is_still_there():
    """The statements of fc_par_plan / fc_steps_plan whose arithmetic the restatement copies, as text: a change to one of them
    has to come with a change to tests/fc_shapes.py."""
    par = re.sub(r"\s+", " ", open(os.path.join(CSRC, "fc_par_kernels.h")).read())
    steps = re.sub(r"\s+", " ", open(os.path.join(CSRC, "fc_steps_kernels.h")).read())
    for stmt in ("bool ok = P <= 512L * FCP_NPT && P % 4 == 0;",
                 "ok = ok && n.d[l] <= 128 && n.d[l + 1] <= 128;",
                 "ok = ok && 32L * n.d[0] <= 8L * FCM_T;",
                 "p.drows = (n.dmax + 31) / 32 * 32;",
                 "p.buf_off = rows * FCM_BSP;",
                 "long off = p.buf_off + 2L * p.drows * FCM_BSP + 32L * FCM_BSP;",
                 "off = (off + 3) & ~3L;",
                 "off += P + 32;",
                 "p.floats = off + 128;",
                 "if (!ok || p.floats * 4 > FCP_LDS_BUDGET) p.floats = 0;"):
        assert stmt in par, stmt
    for stmt in ("if (p.floats) p.floats = p.misc_off + 128 + FCS_ROW_WORDS;", "if (p.floats * 4 > FCP_LDS_BUDGET) p.floats = 0;"):
        assert stmt in steps, stmt


def _lib_layout(row):
    from slimdqn import _hip

    cfg = _hip.make_config("fc", row.K, row.A, (row.d0, 1, 1), row.feats, max(row.B, 32), F.LR, row.eps, F.GAMMA_N)
    return _hip.layout(cfg)


@pytest.mark.parametrize("rid", RUN_IDS)
def test_restated_layout_equals_idqn_layout(rid):
    row = F.BY_ID[rid]
    leaves, P = _lib_layout(row)
    w_off, b_off, P_py = F.layout(row.d0, row.feats, row.A)
    assert P == P_py and P % 64 == 0
    assert [off for _, off, _ in leaves] == [o for pair in zip(w_off, b_off) for o in pair]


def test_every_head_stride_is_a_multiple_of_64():
    """Why ``P % 4 != 0`` has no row: no MLP shape gives one (a sweep of odd widths through the library's own layout)."""
    from slimdqn import _hip

    for d0, feats, A in [(1, [1], 1), (3, [5, 7], 3), (127, [33], 31), (9, [1, 1, 1], 2), (65, [129, 3], 17)]:
        cfg = _hip.make_config("fc", 1, A, (d0, 1, 1), feats, 32, 1e-3, 1e-6, 0.9)
        assert _hip.layout(cfg)[1] % 64 == 0


def test_the_refusal_row_is_refused_with_its_message():
    from slimdqn import _hip

    for row in F.REFUSED:
        with pytest.raises(_hip.HipExtensionError, match=F.REFUSAL_NO_HIDDEN):
            _lib_layout(row)


def _hidden(w):
    return lambda r, d, P, pp, sp: w in d[1:-1] and pp.ok


def _both(w):
    return lambda r, d, P, pp, sp: w in d[1:-1] and d[-1] == w and pp.ok


CLAIMS = {
    "layers=2": lambda r, d, P, pp, sp: len(d) == 3 and pp.ok,
    "layers=3": lambda r, d, P, pp, sp: len(d) == 4 and pp.ok,
    "layers=4": lambda r, d, P, pp, sp: len(d) == 5 and pp.ok,
    "layers=5": lambda r, d, P, pp, sp: len(d) == 6 and pp.ok,
    "hidden=1": _hidden(1), "hidden=127": _hidden(127), "hidden=128": _hidden(128),
    "hidden=A=31": _both(31), "hidden=A=32": _both(32), "hidden=A=33": _both(33), "hidden=A=64": _both(64), "hidden=A=65": _both(65),
    "hidden=A=96": _both(96), "hidden=A=97": _both(97),
    "A=1": lambda r, d, P, pp, sp: d[-1] == 1 and pp.ok,
    "A=127": lambda r, d, P, pp, sp: d[-1] == 127 and pp.ok,
    "A=128": lambda r, d, P, pp, sp: d[-1] == 128 and pp.ok,
    "din odd everywhere": lambda r, d, P, pp, sp: len(d) >= 4 and all(w & 1 for w in d[:-1]) and pp.ok,
    "din even everywhere": lambda r, d, P, pp, sp: len(d) >= 4 and not any(w & 1 for w in d[:-1]) and pp.ok,
    "d0=1": lambda r, d, P, pp, sp: d[0] == 1 and pp.ok,
    "d0=127": lambda r, d, P, pp, sp: d[0] == 127 and pp.ok,
    "d0=128": lambda r, d, P, pp, sp: d[0] == 128 and 32 * d[0] == 8 * F.FCM_T and pp.ok,
    "B=1": lambda r, d, P, pp, sp: r.B == 1 and pp.ok,
    "B=2": lambda r, d, P, pp, sp: r.B == 2 and pp.ok,
    "B=31": lambda r, d, P, pp, sp: r.B == 31 and pp.ok,
    # slots j = 0..4 of thread 0 start below P (4 * 512 * 4 = 8192 < P), slot 5 of every thread starts at or past it
    "8192<P<=10240": lambda r, d, P, pp, sp: 8192 < P <= 4 * F.FCM_T * 5 and pp.ok,
    "P%2048==0": lambda r, d, P, pp, sp: P % (4 * F.FCM_T) == 0 and P < F.P_MAX and pp.ok,
    "P=12288": lambda r, d, P, pp, sp: P == F.P_MAX and pp.ok,
    "LDS within 2 KB": lambda r, d, P, pp, sp: pp.ok and sp.ok and 0 <= F.FCP_LDS_BUDGET - pp.floats * 4 < 2048,
    "par not steps": lambda r, d, P, pp, sp: pp.ok and not sp.ok and sp.why == ["LDS (steps)"],
    "K=1": lambda r, d, P, pp, sp: r.K == 1 and pp.ok,
    "K=9": lambda r, d, P, pp, sp: r.K == 9 and pp.ok,
    "refused": lambda r, d, P, pp, sp: r.feats == [] and r.route is None,
    # outside rows: exactly the named condition fails, and by the smallest step
    "width>128": lambda r, d, P, pp, sp: pp.why == ["width > 128"] and max(d[1:]) == 129 and d[0] <= 128,
    "d0>128": lambda r, d, P, pp, sp: d[0] == 129 and max(d[1:]) <= 128 and "d0 > 128" in pp.why and "LDS" not in pp.why and P <= F.P_MAX,
    "P>12288": lambda r, d, P, pp, sp: pp.why == ["P > 12288"] and P == F.P_MAX + 64,
    "LDS over": lambda r, d, P, pp, sp: pp.why == ["LDS"] and 0 < pp.floats * 4 - F.FCP_LDS_BUDGET <= 64,
    "B>32": lambda r, d, P, pp, sp: pp.ok and r.B == 33,
}


@pytest.mark.parametrize("rid", IDS)
def test_every_row_is_there_for_the_reason_it_states(rid):
    row = F.BY_ID[rid]
    d = F.dims(row.d0, row.feats, row.A)
    P = F.layout(row.d0, row.feats, row.A)[2]
    pp, sp = F.par_plan(row.d0, row.feats, row.A), F.steps_plan(row.d0, row.feats, row.A)
    assert row.why and row.claim in CLAIMS
    assert CLAIMS[row.claim](row, d, P, pp, sp), (row.why, d, P, pp, sp.why)
    if row.route is not None:
        assert F.expected_route(row.d0, row.feats, row.A, row.B) == row.route
        assert (row in F.INSIDE) == (row.route == F.PAR)
    assert row.K <= 3 or row.claim == "K=9"


def test_the_table_covers_what_it_is_there_for():
    assert 30 <= len(F.TABLE) <= 40 and len({r.id for r in F.TABLE}) == len(F.TABLE)
    ins = [F.dims(r.d0, r.feats, r.A) for r in F.INSIDE]
    for w in (1, 31, 32, 33, 64, 65, 96, 97, 127, 128):
        assert any(w in d[1:-1] for d in ins), f"no inside row with hidden width {w}"
        assert any(d[-1] == w for d in ins), f"no inside row with A = {w}"
    for pos in range(3):  # odd and even din at every layer position of a three-layer net
        assert any(len(d) == 4 and d[pos] & 1 for d in ins) and any(len(d) == 4 and not d[pos] & 1 for d in ins)
    assert {1, 2, 31, 32} <= {r.B for r in F.INSIDE} and {1, 9} <= {r.K for r in F.INSIDE}
    assert {1, 127, 128} <= {r.d0 for r in F.INSIDE}
    assert {len(d) - 2 for d in ins} >= {1, 2, 3, 4}
    assert F.ALL_TERMINAL in F.BY_ID and all(F.BY_ID[i].B == b for i, b in zip(F.RAGGED, (1, 2, 31)))
    assert F.BY_ID[F.TIE_ROWS[0]].A >= 6 and F.BY_ID[F.TIE_ROWS[1]].A == 1
    assert all(F.BY_ID[i] in F.INSIDE for i in F.DESCENDANT_ROWS + (F.DESCENDANT_LOOP_ROW,))


def test_the_batches_are_shaped_as_the_issue_asks():
    for row in F.RUNNABLE:
        _, _, batches, w = F.inputs(row.id)
        assert len(batches) == 3 and 0.05 <= w.min() and w.max() <= 1.0
        s, a, r, s2, t = batches[0]
        assert any(b[4].any() for b in batches) and (row.B == 1 or (t.any() and t.all() == (row.id == F.ALL_TERMINAL)))
        assert a[0] == row.A - 1 and (row.B == 1 or a[-1] == 0) and a.min() >= 0 and a.max() < row.A
        if row.B > 1:
            assert np.isclose(np.abs(r).min(), 1e-3) and np.isclose(np.abs(r).max(), 10.0)
        assert any(not np.array_equal(batches[0][0], b[0]) for b in batches[1:])


def _fp32_margins(rid):
    """The fp32 oracle's deviation from the fp64 oracle, as a fraction of each bar of the GPU test (mu / nu: the raw
    deviation relative to the leaf's largest entry)."""
    row = F.BY_ID[rid]
    a, b = F.oracle(rid, np.float32), F.oracle(rid, np.float64)
    m = {"loss": 0.0, "grad": 0.0, "td": 0.0, "wloss": 0.0, "wgrad": 0.0, "step_loss": 0.0, "cum": 0.0, "param": 0.0, "q": 0.0,
         "moment": 0.0}
    for k in range(row.K):
        for tag, key in (("", "plain"), ("w", "weighted")):
            (la, ga, xa), (lb, gb, xb) = a[key][k], b[key][k]
            m[tag + "loss"] = max(m[tag + "loss"], abs(float(la) - lb) / F.LOSS_ATOL)
            for leaf in gb:
                m[tag + "grad"] = max(m[tag + "grad"], F.rel_to_max(ga[leaf], gb[leaf]) / F.GRAD_RTOL)
        ta, tb = np.abs(a["weighted"][k][2]["td"]).astype(np.float64), np.abs(b["weighted"][k][2]["td"])
        m["td"] = max(m["td"], float((np.abs(ta - tb) / (F.TD_ATOL + F.TD_RTOL * tb)).max()))
    m["step_loss"] = float(np.abs(a["losses"] - b["losses"]).max() / F.LOSS_ATOL)
    m["cum"] = float(np.abs(a["cum"] - b["cum"]).max() / (F.LOSS_ATOL * F.N_STEPS_CHAIN))
    for leaf in b["p"]:
        m["param"] = max(m["param"], float(np.abs(a["p"][leaf].astype(np.float64) - b["p"][leaf]).max() / F.PARAM_ATOL))
        for k in range(row.K):
            for mom in ("mu", "nu"):
                m["moment"] = max(m["moment"], F.rel_to_max(a[mom][leaf][k], b[mom][leaf][k]))
    for key in ("q", "qt"):
        scale = F.Q_RTOL * max(1.0, float(np.abs(b[key]).max()))
        m["q"] = max(m["q"], float(np.abs(a[key].astype(np.float64) - b[key]).max() / scale))
    return m


@pytest.mark.parametrize("rid", RUN_IDS)
def test_fp32_oracle_is_within_half_of_every_bar(rid):
    m = _fp32_margins(rid)
    print(rid, {k: f"{v:.3g}" for k, v in m.items()})
    moment = m.pop("moment")
    assert all(v <= 0.5 for v in m.values()), m
    assert moment <= F.MOMENT_FP32_DEV * (1 + 1e-9), "MOMENT_FP32_DEV in tests/fc_shapes.py is no longer the table's largest"
    assert moment <= 0.5 * F.MOMENT_RTOL


def test_the_moment_bar_is_four_times_the_measured_fp32_deviation():
    worst = max(_fp32_margins(rid)["moment"] for rid in RUN_IDS)
    assert worst == pytest.approx(F.MOMENT_FP32_DEV, rel=0.05), worst
    assert 4 * F.MOMENT_FP32_DEV <= F.MOMENT_RTOL <= 5 * F.MOMENT_FP32_DEV
