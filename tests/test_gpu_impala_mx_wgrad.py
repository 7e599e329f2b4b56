"""The impala matrix-core weight gradient on the device (IDQN_IMP_WGRAD=bf16x3, csrc/impala_mx_wgrad_kernels.h), row by row of
tests/impala_mx_wgrad_shapes.py: the switch and the route (``idqn_profile_table`` names ``k_imp_wgrad_mx`` once per eligible
layer), what the switch alone may move, every row against the fp64 oracle at the bars of tests/test_gpu_impala.py (imported, not
restated), three chained Adam steps at the bars of tests/test_gpu_impala_mx.py, the weighted step with |TD|, two fresh handles,
a smaller batch after a larger one, a used handle against a fresh one, the replay-sourced step, and ``valu`` against a child
process that never saw the variable.

The library reads both switches when a handle is created; every agent here creates its own under ``monkeypatch.setenv``."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import impala_mx_wgrad_shapes as W
import test_gpu_impala as G  # the bars: _grad_bar's 2e-5 with the 4 x f32_errors fallback, and the loss / Q figures below
import test_gpu_impala_mx as X  # the used-handle history and the replay-sourced configuration

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(W.ROWS)
VAR, CONV = "IDQN_IMP_WGRAD", "IDQN_IMP_CONV"


def _agent(name):
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = W.case(name)
    agent = iDQN(0, obs, A, K, feats, "impala", W.LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=W.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _batch(name, n=None):
    return Batch(*[np.array(a[:n]) for a in W.case(name)[7]])


def _grad_bar(name, k, leaf):
    """tests/test_gpu_impala.py's own bar (2e-5, or 4 x the float32 autograd's error), evaluated on this file's table"""
    table, G.S = G.S, W
    try:
        return G._grad_bar(name, k, leaf)
    finally:
        G.S = table


def _modes(monkeypatch, wgrad, conv):
    for var, v in ((VAR, wgrad), (CONV, conv)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, v)


def _launches(agent, batch):
    """launch names of one gradient-only step, in order of first appearance, and their counts"""
    from slimdqn import _hip

    agent._learn(batch, flags=_hip.F_PROFILE_ALL | _hip.F_GRADS_ONLY)
    buf = C.create_string_buffer(1 << 14)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, len(buf)), "idqn_profile_table")
    rows = [ln.split("\t") for ln in buf.value.decode().splitlines()]
    return {r[0]: int(r[2]) for r in rows}


@pytest.mark.parametrize("name", NAMES)
def test_switch_and_route(name, monkeypatch):
    obs, feats, A, K, B, *_ = W.case(name)
    mx, valu = W.expected_wgrad_launches(obs, feats)
    _modes(monkeypatch, None, None)
    off = _launches(_agent(name), _batch(name))
    assert off.get("k_imp_wgrad") == 15 and off.get("k_imp_wreduce") == 15 and "k_imp_wgrad_mx" not in off, off
    _modes(monkeypatch, "bf16x3", None)
    on = _launches(_agent(name), _batch(name))
    # (the table counts per name: one k_imp_wreduce per weight-gradient launch of either kernel -- imp_wgrad launches the pair)
    assert on.get("k_imp_wgrad_mx", 0) == mx and on.get("k_imp_wgrad", 0) == valu and on.get("k_imp_wreduce") == mx + valu == 15, on
    assert valu >= 1  # the uint8 conv
    # nothing else of the step changes its name or count
    strip = lambda t: {n: c for n, c in t.items() if not n.startswith("k_imp_wgrad")}  # noqa: E731
    assert strip(on) == strip(off)
    if name != "workload":
        return
    assert (mx, valu) == (14, 1)
    # a garbage value is refused at create, with nothing allocated; non-impala handles ignore the variable
    import torch

    monkeypatch.setenv(VAR, "bf16")
    bad = _agent("one_row")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(Exception) as e:
        bad._ensure_handle(4)
    assert "IDQN_IMP_WGRAD must be valu or bf16x3, got 'bf16'" in str(e.value), str(e.value)
    assert bad._handle is None
    assert torch.cuda.mem_get_info()[0] == free0
    from slimdqn.networks.idqn import iDQN

    fc = iDQN(0, 8, 4, 2, [16, 16], "fc", 1e-3, 0.99, 1, 1, 10**9, 10**9)
    fc._ensure_handle(8)
    assert fc._handle is not None


@pytest.mark.parametrize("name", ["mixed_mx_valu", "all_mx"])
def test_only_what_should_move_moves(name, monkeypatch):
    from slimdqn import _hip

    obs, feats, A, K, B, *_ = W.case(name)
    mx = {W.leaf_name(s, i) for s, i in W.mx_layers(obs, feats)}
    out = {}
    for mode in (None, "bf16x3"):
        _modes(monkeypatch, mode, None)
        agent = _agent(name)
        agent._ensure_handle(B)
        import torch

        td_dev = torch.zeros(K * B, dtype=torch.float32, device="cuda")
        w_dev = torch.ones(B, dtype=torch.float32, device="cuda")
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
        try:
            losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
        finally:
            _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
        acts = {nm % s: agent._debug(nm % s).cpu().numpy().tobytes() for s in range(3) for nm in ("imp_c0_%d", "imp_pool%d", "imp_stack%d")}
        out[mode] = (losses.tobytes(), td_dev.cpu().numpy().tobytes(), acts, {n: g.copy() for n, g in agent._flat_grad().items()})
        agent._destroy_handle()
    off, on = out[None], out["bf16x3"]
    assert off[0] == on[0] and off[1] == on[1]
    for nm in off[2]:
        assert off[2][nm] == on[2][nm], nm
    want = W.oracle(name)
    for leaf, g in off[3].items():
        layer = leaf.rsplit("/", 1)[0]
        if layer in mx and leaf.endswith("kernel"):
            assert g.tobytes() != on[3][leaf].tobytes(), leaf  # the route is real
            for k in range(K):
                ref = want[k]["grads"][leaf]
                err = np.abs(on[3][leaf][k] - ref).max() / (np.abs(ref).max() + 1e-300)
                print(name, k, leaf, "relative gradient error", err, "bar", _grad_bar(name, k, leaf))
                assert err <= _grad_bar(name, k, leaf), (leaf, err)
        elif layer not in mx:
            assert g.tobytes() == on[3][leaf].tobytes(), leaf


ORACLE_CASES = [(n, "bf16x3") for n in NAMES] + [("all_mx", None), ("mixed_mx_valu", None)]


@pytest.mark.parametrize("name, conv", ORACLE_CASES)
def test_row_against_the_oracle(name, conv, monkeypatch):
    from slimdqn import _hip

    _modes(monkeypatch, "bf16x3", conv)
    obs, feats, A, K, B, p, pt, batch = W.case(name)
    want = W.oracle(name)
    agent = _agent(name)
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    Gr = agent._flat_grad()
    n32 = min(B, 32)
    for k in range(K):
        w = want[k]
        print(name, k, "loss", losses[k], w["loss"])
        errs = {leaf: np.abs(Gr[leaf][k] - g).max() / (np.abs(g).max() + 1e-300) for leaf, g in w["grads"].items()}
        for leaf, err in errs.items():  # every figure first, then the bars
            print(name, k, leaf, "relative gradient error", err, "bar", _grad_bar(name, k, leaf))
        q = agent.q_values(agent.params, batch[0][:n32], k).cpu().numpy()
        qt = agent.q_values(agent.target_params, batch[3][:n32], k).cpu().numpy()
        print(name, k, "Q error", np.abs(q - w["q"][:n32]).max(), "target Q error", np.abs(qt - w["q_next"][:n32]).max())
        assert abs(losses[k] - w["loss"]) <= 1e-5 * max(1.0, abs(w["loss"])), (k, losses[k], w["loss"])
        for leaf, err in errs.items():
            assert err <= _grad_bar(name, k, leaf), (leaf, err)
        assert np.abs(q - w["q"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q"]).max())
        assert np.abs(qt - w["q_next"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q_next"]).max())
        i = min(1, B - 1)
        row = np.sort(w["q"][i])
        if row[-1] - row[-2] > 1e-4:  # (a near-tie of the oracle's own row decides nothing)
            assert int(agent._best_action(0, k, np.asarray(batch[0][i]))) == int(np.argmax(w["q"][i]))


@pytest.mark.parametrize("name", NAMES)
def test_three_chained_steps(name, monkeypatch):
    """As tests/test_gpu_impala_mx.py::test_three_chained_steps, its bars unchanged, both switches on.  The weight gradient
    feeds no pool of its own step; it moves the parameters the next step's pools see, so the selections are printed per step,
    head and Stack (row ``workload`` has a pool window six float32 ulps wide after the first step)."""
    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    _modes(monkeypatch, "bf16x3", "bf16x3")
    obs, feats, A, K, B, p, pt, batch = W.case(name)
    agent = _agent(name)
    b = _batch(name)
    for step in range(3):
        before = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        agent._learn(b)
        after = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        for k in range(K):
            _, grads = T.loss_and_grads(Q.head(before["_online"], k), Q.head(pt, k), batch, "impala", W.GAMMA_N)
            for si, ref in enumerate(W.stage_outputs_of(Q.head(before["_online"], k), batch[0])[0]):  # a figure, not a bar
                got = agent._debug("imp_c0_%d" % si).cpu().numpy()[k * ref.size : (k + 1) * ref.size].reshape(ref.shape)
                print(name, step, k, "imp_c0_%d" % si, "pool windows whose selection differs from fp64's:",
                      int((W.pool_selection(got) != W.pool_selection(ref)).sum()))
            for leaf, g in grads.items():
                th, m, v = Q.adam_update(before["_online"][leaf][k].astype(np.float64), g, before["_mu"][leaf][k].astype(np.float64),
                                         before["_nu"][leaf][k].astype(np.float64), step, W.LR, W.EPS)
                gm = np.abs(g).max() + 1e-300
                worst = np.unravel_index(np.abs(after["_online"][leaf][k] - th).argmax(), th.shape)
                print(name, step, k, leaf, "mu error / max |g|", np.abs(after["_mu"][leaf][k] - m).max() / gm, "worst parameter error / lr",
                      np.abs(after["_online"][leaf][k] - th)[worst] / W.LR, "where the oracle's gradient / max |g| is", g[worst] / gm)
                assert np.abs(after["_mu"][leaf][k] - m).max() <= 1e-4 * gm, (step, leaf)
                assert np.abs(after["_nu"][leaf][k] - v).max() <= 1e-4 * gm * gm, (step, leaf)
                err = np.abs(after["_online"][leaf][k] - th)
                assert err.max() <= W.LR * 1.01 + 1e-6, (step, leaf)
                assert np.median(err) <= 2e-5, (step, leaf, np.median(err))
    assert (agent._count.cpu().numpy() == 3).all()


@pytest.mark.parametrize("name", NAMES)
def test_weighted_step_and_td(name, monkeypatch):
    import torch

    from slimdqn import _hip

    _modes(monkeypatch, "bf16x3", "bf16x3")
    obs, feats, A, K, B, p, pt, batch = W.case(name)
    agent = _agent(name)
    wts = np.random.default_rng(5).uniform(0.2, 1.0, B).astype(np.float32)
    agent._ensure_handle(B)
    w_dev, td_dev = torch.from_numpy(wts).cuda(), torch.zeros(K * B, dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    try:
        losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    Gr, td = agent._flat_grad(), td_dev.cpu().numpy().reshape(K, B)
    for k in range(K):
        loss, grads, td_want = W.weighted_oracle(name, k, wts)
        assert abs(losses[k] - loss) <= 1e-5 * max(1.0, abs(loss))
        assert np.abs(td[k] - td_want).max() <= 1e-5 * max(1.0, np.abs(td_want).max())
        for leaf, g in grads.items():
            assert np.abs(Gr[leaf][k] - g).max() <= _grad_bar(name, k, leaf) * (np.abs(g).max() + 1e-300), leaf


def _step_bytes(name):
    """losses and gradients of a gradient-only step, then all six arenas after a full step, on a fresh agent"""
    from slimdqn import _hip

    agent = _agent(name)
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    grads = agent._grad.cpu().numpy().tobytes()
    agent._learn(_batch(name))
    out = (losses, grads) + tuple(getattr(agent, s).cpu().numpy().tobytes() for s in X.ARENAS)
    agent._destroy_handle()
    return out


@pytest.mark.parametrize("name", ["all_mx", "many_chunks", "workload"])
def test_two_fresh_handles_give_equal_bytes(name, monkeypatch):
    _modes(monkeypatch, "bf16x3", "bf16x3")
    assert _step_bytes(name) == _step_bytes(name)


@pytest.mark.parametrize("conv", [None, "bf16x3"])
def test_a_smaller_batch_after_a_larger_one(conv, monkeypatch):
    """A handle sized for B = 5 steps at B = 5 (two chunks per eligible Stack-0 layer), then at B = 2 (one): the gradients are
    a fresh handle's stepped once at B = 2 -- no partial of the longer chunk list is read."""
    from slimdqn import _hip

    _modes(monkeypatch, "bf16x3", conv)
    name = "small_after_large"
    obs, feats, A, K, B, *_ = W.case(name)
    assert B == 5 and W.plan(5, 10, 9, 32, 32)[3] == 2 and W.plan(2, 10, 9, 32, 32)[3] == 1
    used = _agent(name)
    used._learn(_batch(name), flags=_hip.F_GRADS_ONLY)
    l_used = used._learn(_batch(name, 2), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    g_used = used._grad.cpu().numpy().tobytes()
    fresh = _agent(name)
    fresh._ensure_handle(5)
    l_fresh = fresh._learn(_batch(name, 2), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    assert l_used == l_fresh and g_used == fresh._grad.cpu().numpy().tobytes()


def test_a_used_handle_equals_a_fresh_one(monkeypatch):
    """tests/test_gpu_impala_mx.py's history (step, Q-values, acting, target update and sync, a second step) with the weight
    gradient on the matrix cores as well: that test turns IDQN_IMP_CONV on itself"""
    monkeypatch.setenv(VAR, "bf16x3")
    X.test_a_used_handle_equals_a_fresh_one(monkeypatch)


def test_replay_sourced_step_is_gather_then_learn(monkeypatch):
    monkeypatch.setenv(VAR, "bf16x3")
    X.test_replay_sourced_step_is_gather_then_learn(monkeypatch)


def mode_off_digest(name="mixed_mx_valu"):
    return hashlib.sha256(b"".join(_step_bytes(name))).hexdigest()


CHILD = r"""
import json, sys, os
assert "IDQN_IMP_WGRAD" not in os.environ and "IDQN_IMP_CONV" not in os.environ
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_impala_mx_wgrad as Y
print("RESULT" + json.dumps(Y.mode_off_digest()))
"""


def test_valu_is_the_unset_path(monkeypatch):
    """IDQN_IMP_WGRAD=valu here against a child process that never had the variable: the same bytes of a full step, and the
    launches of the vector-ALU kernel only."""
    env = dict(os.environ)
    for s in (VAR, CONV, "IDQN_HIP_LIB"):
        env.pop(s, None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    unset = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])
    _modes(monkeypatch, "valu", None)
    assert mode_off_digest() == unset
    got = _launches(_agent("mixed_mx_valu"), _batch("mixed_mx_valu"))
    assert got.get("k_imp_wgrad") == 15 and not any("_mx" in n for n in got), got
    _modes(monkeypatch, "bf16x3", None)
    assert mode_off_digest() != unset  # the mode changes the bytes: the comparison above can fail
