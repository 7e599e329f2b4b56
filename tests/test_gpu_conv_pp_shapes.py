"""GPU: the persistent conv kernel (csrc/convp_pp.hip) at frames other than 84x84 -- fp64 parity, bit parity with the one-item
launches, and the plans pinned.

``tests/conv_pp_shapes.py`` has the table and says which row covers which plan class.  Every row runs in two child processes on
the shipped library (a switch is read once per process): the persistent child (default environment, or ``IDQN_CONV_PP=31``
where the row covers the Conv_1 data gradient, which the default mask leaves on the one-item launch) and ``IDQN_CONV_PP=0``.

Per row:
* the ``[plan]`` lines of the persistent child equal the pinned (parts, NT, ring, n_items, n_wg) of every role, and the
  ``IDQN_CONV_PP=0`` child has no persistent plan at all; the paired / separate route of the Conv_1 / Conv_2 gradients is pinned;
* the persistent child against the fp64 oracle, at the bars of tests/test_gpu_conv_geometry.py and test_gpu_fp_path.py: every stage
  of every head and 32-sample block, zero borders, losses, and the parameters after one full step;
* the persistent child against ``IDQN_CONV_PP=0``, byte for byte: every activation / gradient buffer (borders included), the
  gradient arena, losses, parameters and Adam state after the full step;
* one handle that switches plans: the step at B, a step at 20 samples (one-item plans), the step at B again -- the third equals
  the first byte for byte.

Every child has a timeout of 120 s (``conv_pp_shapes.CHILD_TIMEOUT``); observed on an MI355X: about 3 s of wall time per child
(2.3 s of it importing torch and creating the handle), the oracle of a row 0.4 .. 2.7 s on the CPU.  DESIGN.md 5 lists the
observed errors.

Inputs: seeded as tests/test_gpu_conv_geometry.py::_inputs seeds them, shifted by ``Row.seed`` -- the smallest shift at which the
oracle's own numpy-fp32 restatement meets STAGE_BAR against fp64 and no ReLU unit within half an fp32 ulp of zero carries a gradient
above it (``conv_pp_shapes.fp32_restatement_error`` and ``relu_exposure``, asserted on the CPU):
at the other seeds a ReLU unit within a few 1e-9 of zero makes the fp64 derivative no reference for fp32 arithmetic of any kind.
"""
import functools
import os
import time

import numpy as np
import pytest

import cnn_stages as S
import conv_pp_shapes as T

pytestmark = pytest.mark.gpu
LOSS_ATOL = 1e-5  # per-head loss (test_gpu_fp_path.py)
STAGE_BAR = 2e-5  # every stage, relative to the stage's largest entry (test_gpu_fp_path.py)
Q_RTOL = 2e-6     # i-IQN Q-values, relative to max(1, max |q|) (test_gpu_conv_geometry.py::test_iqn_step_and_acting_against_oracle)


@functools.lru_cache(maxsize=None)
def _reference(i):
    """Inputs and what the oracle says about row i: computed once, never modified."""
    from oracle import qnet_ref as Q

    row = T.TABLE[i]
    t0 = time.time()
    p, pt, batch = T.inputs(row.obs, row.feats, row.A, row.K, row.B, row.seed)
    heads = S.oracle_heads(p, pt, batch, row.K, T.GAMMA_N)
    adam = {}
    for n in p:  # Q.learn_on_batch's update from a zero optimizer state (tests/test_gpu_conv_geometry.py::_reference)
        adam[n] = np.stack([Q.adam_update(p[n][k].astype(np.float64), heads[k][1][n], 0.0, 0.0, 0, T.LR, T.EPS)[0]
                            for k in range(row.K)])
    print(f"oracle of row {i}: {time.time() - t0:.1f} s")
    return p, pt, batch, heads, adam


@pytest.mark.parametrize("i", range(len(T.TABLE)), ids=T.IDS)
def test_persistent_row(i, tmp_path):
    row = T.TABLE[i]
    nb = (row.B + 31) // 32
    save = str(tmp_path / "persistent.npz")
    got, plans, wall = T.run_child(T.spec_of(row, seed=row.seed, save=save), pp=row.pp_mask)
    ref, ref_plans, ref_wall = T.run_child(T.spec_of(row, seed=row.seed), pp="0")
    print(f"child wall time: persistent {wall:.1f} s (inside {got['seconds']} s), IDQN_CONV_PP=0 {ref_wall:.1f} s")
    failures = []

    # ---- which kernel ran ----------------------------------------------------------------------------------------------
    assert not plans["unknown"] and not ref_plans["unknown"], (plans["unknown"], ref_plans["unknown"])
    for line in plans["pp"]:
        print("[plan] pp", line)
    chosen = T.chosen_plans(plans, nb)
    print("chosen:", chosen)
    if chosen != tuple(row.plans):
        failures.append(("plans", chosen, tuple(row.plans)))
    if [p for p in T.chosen_plans(plans, 1) if p is not None]:
        failures.append(("the 20-sample step in between ran a persistent plan", T.chosen_plans(plans, 1)))
    if ref_plans["pp"]:
        failures.append(("IDQN_CONV_PP=0 made a persistent plan", ref_plans["pp"]))
    routes = T.paired_routes(got["launches"])
    print("routes:", routes)
    if routes != row.paired or T.paired_routes(ref["launches"]) != row.paired:
        failures.append(("paired routes", routes, T.paired_routes(ref["launches"]), row.paired))
    assert got["count"] == [1] * row.K and ref["count"] == [1] * row.K

    # ---- persistent against one item per workgroup, and the third step against the first: byte for byte -----------------
    diff = T.differing(got["digests"], ref["digests"])
    if diff:
        failures.append(("differs from IDQN_CONV_PP=0", diff))
    diff = T.differing(got["digests"], got["digests"], "first/", "third/")
    if diff:
        failures.append(("the third step differs from the first", diff))
    assert sum(n.startswith("first/") for n in got["digests"]) == len(T.DEBUG_NAMES) + 2
    assert sum(n.startswith("full/") for n in got["digests"]) == len(T.STATE_NAMES)

    # ---- persistent against the fp64 oracle --------------------------------------------------------------------------------
    p, pt, batch, heads, adam = _reference(i)
    with np.load(save) as z:
        arrays = {n: z[n] for n in z.files}
    os.remove(save)
    losses = arrays["first/_losses"][: row.K]
    for k in range(row.K):
        if not abs(losses[k] - heads[k][0]) <= LOSS_ATOL:
            failures.append(("loss", k, float(losses[k]), float(heads[k][0])))
    rec = T.Recorded(arrays)
    errs = S.stage_errors(rec, p, pt, batch, row.obs, row.feats, row.A, row.K, row.B, T.GAMMA_N, "bf16x3", oracle=heads)
    worst = max(errs, key=errs.get)
    print(f"worst stage: {worst} {errs[worst]:.3e}")
    failures += [("stage", n, e) for n, e in errs.items() if not e < STAGE_BAR]
    for name, (outside, inside) in S.border_report(rec, row.obs, row.feats, row.K, row.B, "bf16x3").items():
        print(f"border {name}: max |outside| {outside:.3e}, min over slots of max |interior| {inside:.3e}")
        if not outside == 0.0:
            failures.append(("border not zero", name, outside))
        if not inside > 0.0:
            failures.append(("interior all zero in some slot", name, inside))
    for leaf in adam:  # the rule of test_gpu_fp_path.py::test_many_block_step_against_oracle
        err = np.abs(arrays["online/" + leaf] - adam[leaf])
        print(f"adam {leaf}: max {err.max():.3e}, within 3e-7: {(err <= 3e-7).mean():.4f}")
        if not (err.max() <= 2e-5 and (err <= 3e-7).mean() >= 0.98):
            failures.append(("adam", leaf, float(err.max()), float((err <= 3e-7).mean())))
    assert not failures, failures


def test_acting_set_goes_persistent_through_the_iqn_handle(tmp_path):
    """Class 9: 250 states through ``idqn_iqn_q_values`` on a 112x112 frame -- the acting set's three forward plans (one net, eight
    blocks) go persistent.  Pinned plans, every Q row against oracle/iqn_ref.py, byte parity with IDQN_CONV_PP=0."""
    from oracle import iqn_ref as I
    from oracle import qnet_ref as Q

    row = T.ACT_ROW
    save = str(tmp_path / "act.npz")
    got, plans, wall = T.run_child(T.spec_of(row, save=save), pp=None)
    ref, ref_plans, ref_wall = T.run_child(T.spec_of(row), pp="0")
    print(f"child wall time: persistent {wall:.1f} s, IDQN_CONV_PP=0 {ref_wall:.1f} s")
    assert not plans["unknown"] and not ref_plans["unknown"]
    acting = sorted(f["role"] for f in plans["fwd"] if f["nb"] == 8)
    assert acting == [8, 9, 10], ("the one-item plans of the acting set carry role + 8", plans["fwd"])
    chosen = T.chosen_plans(plans, 8, roles=range(3))
    print("chosen:", chosen)
    assert all(p["nets"] == 1 for p in plans["pp"])
    assert chosen == tuple(row.plans), (chosen, row.plans)
    assert not ref_plans["pp"]
    assert T.differing(got["digests"], ref["digests"]) == []
    p, states, tau = T.act_inputs(row)
    with np.load(save) as z:
        q = z["act/q"]
    assert q.shape == (row.n, row.A)
    t0 = time.time()
    worst = 0.0
    for e in range(row.n):
        _, want = I.greedy_action(Q.head(p, 0), states[e], tau[:, e])
        err = np.abs(q[e] - want).max() / max(1.0, np.abs(want).max())
        worst = max(worst, err)
    print(f"oracle {time.time() - t0:.1f} s, worst relative Q error {worst:.3e}")
    assert worst <= Q_RTOL
