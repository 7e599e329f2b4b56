"""CPU: the table, the plan-line parser and the digest harness of tests/conv_pp_shapes.py (the GPU side is
tests/test_gpu_conv_pp_shapes.py), and the oracle alone on every row."""
import time

import numpy as np
import pytest

import cnn_stages as S
import conv_pp_shapes as T

# literal output of the fprintf formats in csrc/qnet.hip (plan_fwd, plan_fwd_pp)
SAMPLE = """\
[plan] fwd role 0 nets 10 nb 8 target 256: 400 workgroups, NT 5, ring 3, stage 22528 B, lds 81920 B, supersteps 8, ranges/slot 5 (NPA 1 CT 1 NQ 2)
[plan] pp role 0 parts 1: 1680 items, NT 6, ring 3, stage 28672 B, lds 110592 B, model 1234 k cycles
[plan] pp role 0 parts 2: 3360 items, NT 3, ring 3, stage 18432 B, lds 79872 B, model 1500 k cycles
[plan] pp role 0 nets 10 nb 8: parts 1 -> 1680 items on 256 workgroups, NT 6, ring 3, stage 28672 B, lds 110592 B
[plan] fwd role 1 nets 10 nb 8 target 256: 400 workgroups, NT 3, ring 2, stage 67584 B, lds 159744 B, supersteps 8, ranges/slot 5 (NPA 3 CT 2 NQ 4)
[plan] pp role 1 nets 10 nb 8: parts 2 -> 1760 items on 256 workgroups, NT 3, ring 2, stage 67584 B, lds 159744 B
[plan] fwd role 3 nets 5 nb 8 target 128: 120 workgroups, NT 3, ring 2, stage 43008 B, lds 135168 B, supersteps 12, ranges/slot 3 (NPA 3 CT 2 NQ 3)
[plan] fwd role 4 nets 5 nb 8 target 256: 320 workgroups, NT 4, ring 3, stage 20480 B, lds 94208 B, supersteps 8, ranges/slot 8 (NPA 3 CT 1 NQ 2)
[plan] wgrad layer 2: 240 workgroups, 16 chunks of ~3 positions, PG 2, MT 6, lds 147456 B
[plan] fwd role 9 nets 1 nb 1 target 256: 30 workgroups, NT 2, ring 3, stage 30720 B, lds 92160 B, supersteps 8, ranges/slot 30 (NPA 3 CT 2 NQ 4)
some other line of stderr
"""


def test_parser_on_literal_lines():
    got = T.parse_plan_lines(SAMPLE)
    assert got["unknown"] == [] and got["candidates"] == 2
    assert [f["role"] for f in got["fwd"]] == [0, 1, 3, 4, 9]
    assert got["fwd"][0] == dict(role=0, nets=10, nb=8, target=256, n_items=400, NT=5, ring=3, stage=22528, lds=81920,
                                 supersteps=8, ranges=5, NPA=1, CT=1, NQ=2)
    assert got["fwd"][2]["target"] == 128
    assert got["pp"] == [dict(role=0, nets=10, nb=8, parts=1, n_items=1680, n_wg=256, NT=6, ring=3, stage=28672, lds=110592),
                         dict(role=1, nets=10, nb=8, parts=2, n_items=1760, n_wg=256, NT=3, ring=2, stage=67584, lds=159744)]
    # role 4 has only a fwd line, role 3 only a paired-launch plan, role 2 nothing: none of them is persistent
    assert T.chosen_plans(got, 8) == ((1, 6, 3, 1680, 256), (2, 3, 2, 1760, 256), None, None, None)
    assert T.chosen_plans(got, 1) == (None,) * 5


def test_parser_reports_a_changed_format():
    got = T.parse_plan_lines("[plan] pp role 1 nets 10 blocks 8: parts 2 -> 1760 items\n[plan] fwd role 1: 3 workgroups\n")
    assert len(got["unknown"]) == 2 and not got["pp"] and not got["fwd"]
    with pytest.raises(AssertionError):
        T.chosen_plans(T.parse_plan_lines(SAMPLE + SAMPLE), 8)


def test_paired_routes_from_launch_names():
    names = ["stage (pixels + kernel packing)", "conv0 fwd", "conv2 dgrad + wgrad", "conv1 dgrad", "conv1 wgrad", "conv0 wgrad"]
    assert T.paired_routes(names) == {"conv1": False, "conv2": True}
    with pytest.raises(AssertionError):
        T.paired_routes(["conv1 dgrad", "conv1 wgrad"])  # nothing about conv2


def test_digest_harness_sees_a_swapped_slot():
    rng = np.random.default_rng(0)
    a = {"a1p": rng.standard_normal((6, 40)).astype(np.float32), "_grad": rng.standard_normal(50).astype(np.float32)}
    same = {n: v.copy() for n, v in a.items()}
    assert T.differing(T.digests(a, "first/"), T.digests(same, "third/"), "first/", "third/") == []
    swapped = {n: v.copy() for n, v in a.items()}
    swapped["a1p"][[1, 4]] = swapped["a1p"][[4, 1]]
    assert T.differing(T.digests(a), T.digests(swapped)) == ["a1p"]
    assert T.differing(T.digests(a), T.digests({"a1p": a["a1p"]})) == ["_grad"]
    assert T.digest(a["a1p"]) != T.digest(a["a1p"].reshape(40, 6))  # same bytes, another shape
    # -0.0 and 0.0 are different bytes
    assert T.digest(np.zeros(4, np.float32)) != T.digest(-np.zeros(4, np.float32))
    rec = T.Recorded({"first/a3": a["a1p"], "leafgrad/Conv_0/kernel": a["_grad"]})
    assert rec._debug("a3").cpu().numpy() is a["a1p"] and list(rec._flat_grad()) == ["Conv_0/kernel"]


def _check_plan(obs, feats, role, plan, slots):
    parts, NT, ring, n_items, n_wg = plan
    CT, NPA, NQ, var = T.role_shape(obs, feats, role)
    want_items, raw_nt, _ = T.implied(obs, feats, role, parts, slots)
    assert 1 <= parts <= min(ow for _, ow in var)
    assert n_items == want_items and n_wg == min(n_items, T.CUS)
    assert NT == max(2, raw_nt) and T.pp_built(NPA, CT, NQ, NT)
    assert ring in (2, 3)
    NSS = {0: 8, 1: 4 * feats[0] // 16, 2: 3 * feats[1] // 16, 3: 3 * feats[2] // 16, 4: 2 * feats[1] // 16}[role]
    assert NSS - 1 >= NT


def test_table_integrity():
    seen = set()
    for row in T.TABLE:
        H, W, C = row.obs
        assert C == 4 and H >= 8 and W >= 8 and (H, W) != (84, 84)                       # what cnn_fast_shape() accepts
        assert len(row.feats) == 4 and all(f in (32, 64) for f in row.feats[:3]) and 128 <= row.feats[3] <= 512
        assert 1 <= row.A <= 32 and row.B > T.SMALL_B and len(row.plans) == 5 and set(row.paired) == {"conv1", "conv2"}
        assert row.pp_mask in (None, "31")
        if row.pp_mask is None:
            assert row.plans[4] is None, "the default IDQN_CONV_PP mask (15) leaves role 4 on the one-item launch"
        for role, plan in enumerate(row.plans):
            if plan is not None:
                _check_plan(row.obs, row.feats, role, plan, T.n_slots(role, row.K, row.B))
                assert not (role >= 3 and row.paired["conv2" if role == 3 else "conv1"]), "a paired data gradient has no plan"
        seen |= T.classes_of(row)
    for role, plan in enumerate(T.ACT_ROW.plans):
        _check_plan(T.ACT_ROW.obs, T.ACT_ROW.feats, role, plan, T.n_slots(role, T.ACT_ROW.K, T.ACT_ROW.n, acting=True))
    assert T.ACT_ROW.obs[0] <= 128 and T.ACT_ROW.obs[1] <= 128 and T.ACT_ROW.feats[3] % 256 == 0 and T.ACT_ROW.n <= 256
    if all(p is not None for p in T.ACT_ROW.plans):
        seen.add("9.acting")
    for c in T.CLASSES:
        assert (c in seen) != (c in T.UNREACHABLE), (c, "claimed by a row XOR written off with a reason")
        assert c in seen or len(T.UNREACHABLE[c]) > 40


@pytest.mark.parametrize("i", range(len(T.TABLE)), ids=T.IDS)
def test_oracle_alone(i):
    row = T.TABLE[i]
    t0 = time.time()
    p, pt, batch = T.inputs(row.obs, row.feats, row.A, row.K, row.B, row.seed)
    heads = S.oracle_heads(p, pt, batch, row.K, T.GAMMA_N)
    print(f"oracle: {time.time() - t0:.1f} s")
    assert batch[4][row.B // 2] and any(np.abs(v).max() > 0 for n, v in p.items() if n.endswith("bias"))
    for k, (loss, grads, aux) in enumerate(heads):
        assert np.isfinite(loss)
        # no stage's largest entry is zero: the relative bar of cnn_stages.stage_errors means something
        for li in range(3):
            assert np.abs(aux["tape"][li][4]).max() > 0, (k, "activation", li)
        for key in ("d_dense0", "d_conv2", "d_conv1", "d_conv0"):
            assert np.abs(aux["trace"][key]).max() > 0, (k, key)
        assert np.abs(aux["q"]).max() > 0 and np.abs(aux["q_next"]).max() > 0
        for leaf, g in grads.items():
            assert np.isfinite(g).all() and np.abs(g).max() > 0, (k, leaf)
    err, stage = T.fp32_restatement_error(row)
    print(f"numpy fp32 restatement against fp64: {err:.2e} ({stage})")
    assert err < 2e-5, "plain fp32 arithmetic misses the stage bar on this row's inputs: another seed (conv_pp_shapes.py)"
    exposure, stage = T.relu_exposure(row)
    print(f"largest gradient arriving at a ReLU unit within half an ulp of zero: {exposure:.2e} ({stage})")
    assert exposure < 2e-5, "a ReLU that fp32 rounding decides carries a gradient above the stage bar: another seed"
    # (actions are not compared on the training rows: no top-two gap condition applies)


def test_oracle_alone_acting_row():
    """The acting row compares Q rows, not actions; its states must give live, finite Q-values."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = T.ACT_ROW
    p, states, tau = T.act_inputs(row)
    assert states.shape == (row.n,) + row.obs and tau.shape == (row.n_quantiles, row.n)
    for e in (0, row.n - 1):
        _, q = I.greedy_action(Q.head(p, 0), states[e], tau[:, e])
        assert np.isfinite(q).all() and np.abs(q).max() > 0
