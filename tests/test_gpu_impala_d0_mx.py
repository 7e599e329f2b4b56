"""The impala f32 matrix-core Dense_0 forward on the device (IDQN_IMP_D0=mfma, csrc/impala_d0_mx_kernels.h), row by row of
tests/impala_d0_mx_shapes.py: the switch and the route (``idqn_profile_table`` names ``k_imp_d0_fwd_mx`` in place of
``k_imp_d0_fwd``, in a learner step and in ``idqn_q_values``), and BYTE equality of mode on against mode off -- ``==`` on raw
bytes, no tolerance anywhere: losses, |TD|, the gradient arena, the hidden activations and the Stack-2 input gradient of a
weighted step, every arena after three chained Adam steps, ``idqn_q_values`` of both parameter sets at n = 1, 2, 32,
``idqn_act_host``; then the many-state acting entry against the loop, handle history, the replay-sourced step, one row against
the fp64 oracle at the bars of tests/test_gpu_impala.py (imported, not restated), and ``valu`` against a child process that
never had the variable.

The library reads the switch when a handle is created; every agent here creates its own under ``monkeypatch.setenv``."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import impala_d0_mx_shapes as D
import test_gpu_impala as G  # the bars: _grad_bar's 2e-5 with the 4 x f32_errors fallback, and the loss / Q figures below
import test_gpu_impala_mx as X  # the used-handle history and the replay-sourced configuration

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(D.ROWS)
VAR, CONV, WGRAD = "IDQN_IMP_D0", "IDQN_IMP_CONV", "IDQN_IMP_WGRAD"
ARENAS = X.ARENAS
OLD, NEW = "k_imp_d0_fwd", "k_imp_d0_fwd_mx"


def _agent(name):
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = D.case(name)
    agent = iDQN(0, obs, A, K, feats, "impala", D.LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=D.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _batch(name, n=None):
    return Batch(*[np.array(a[:n]) for a in D.case(name)[7]])


def _states(name, n):
    batch = D.case(name)[7]
    pool = [np.asarray(s) for s in list(batch[0]) + list(batch[3])]
    return [pool[i % len(pool)] for i in range(n)]


def _modes(monkeypatch, d0, conv=None, wgrad=None):
    for var, v in ((VAR, d0), (CONV, conv), (WGRAD, wgrad)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, v)


def _table(agent):
    from slimdqn import _hip

    buf = C.create_string_buffer(1 << 14)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, len(buf)), "idqn_profile_table")
    return {ln.split("\t")[0]: int(ln.split("\t")[2]) for ln in buf.value.decode().splitlines()}


def _launches(name):
    """launch names and counts of one gradient-only learner step, and of one idqn_q_values call after it, on a fresh agent"""
    from slimdqn import _hip

    agent = _agent(name)
    agent._learn(_batch(name), flags=_hip.F_PROFILE_ALL | _hip.F_GRADS_ONLY)
    step = _table(agent)
    agent._q_values(1, D.ROWS[name][3] - 1, np.stack(_states(name, 2)))  # (the timeline stays on until the next step begins)
    qv = _table(agent)
    agent._destroy_handle()
    return step, qv


@pytest.mark.parametrize("name", NAMES)
def test_switch_and_route(name, monkeypatch):
    tables = {}
    for mode in (None, "valu", "mfma"):
        _modes(monkeypatch, mode)
        tables[mode] = _launches(name)
    assert tables[None] == tables["valu"]
    (off, off_q), (on, on_q) = tables[None], tables["mfma"]
    if not D.applies(name):  # no hidden layer: no such launch, the same table on and off
        assert on == off and on_q == off_q and OLD not in off and NEW not in on
        return
    assert off.get(OLD) == 1 and NEW not in off and NEW not in off_q, (off, off_q)
    assert on.get(NEW) == 1 and OLD not in on, on
    assert on_q.get(NEW) == 1 and OLD not in on_q, on_q
    # nothing else of either call changes its name or count
    strip = lambda t: {n: c for n, c in t.items() if n not in (OLD, NEW)}  # noqa: E731
    assert strip(on) == strip(off) and strip(on_q) == strip(off_q)
    assert list(on) == [NEW if n == OLD else n for n in off], "the same place in the step"


def test_a_garbage_value_is_refused_and_other_handles_ignore_the_variable(monkeypatch):
    import torch

    from slimdqn.networks.idqn import iDQN

    _modes(monkeypatch, "bf16x3")  # a value of the OTHER switches
    bad = _agent("f64")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(Exception) as e:
        bad._ensure_handle(4)
    assert "IDQN_IMP_D0 must be valu or mfma, got 'bf16x3'" in str(e.value), str(e.value)
    assert bad._handle is None
    assert torch.cuda.mem_get_info()[0] == free0
    for arch, obs, feats in (("fc", 8, [16, 16]), ("cnn", (20, 20, 4), [32, 32, 32, 128])):
        other = iDQN(0, obs, 4, 2, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)
        other._ensure_handle(8)
        assert other._handle is not None, arch
        other._destroy_handle()
    _modes(monkeypatch, "mfma")
    for arch, obs, feats in (("fc", 8, [16, 16]), ("cnn", (20, 20, 4), [32, 32, 32, 128])):
        other = iDQN(0, obs, 4, 2, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)
        other._ensure_handle(8)
        assert other._handle is not None, arch
        other._destroy_handle()


def _everything(name, full=True):
    """{what: bytes} of a fresh agent: the weighted gradient-only step, then (``full``) three chained Adam steps, Q-values of
    both parameter sets and the single-state acting call; otherwise one acting call"""
    import torch

    from slimdqn import _hip

    obs, feats, A, K, B, *_ = D.case(name)
    agent = _agent(name)
    agent._ensure_handle(B)
    wts = np.random.default_rng(5).uniform(0.2, 1.0, B).astype(np.float32)
    w_dev, td_dev = torch.from_numpy(wts).cuda(), torch.zeros(K * B, dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, _hip.ptr(w_dev), _hip.ptr(td_dev)), "idqn_set_per_buffers")
    try:
        losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    finally:
        _hip.check(_hip.lib().idqn_set_per_buffers(agent._handle, None, None), "idqn_set_per_buffers")
    out = {"weighted losses": losses.tobytes(), "|TD|": td_dev.cpu().numpy().tobytes(), "gradient arena": agent._grad.cpu().numpy().tobytes()}
    assert np.isfinite(losses).all() and np.abs(agent._grad.cpu().numpy()).max() > 0
    for nm in ("imp_hid", "imp_d2") if D.applies(name) else ("imp_d2",):
        out[nm] = agent._debug(nm).cpu().numpy().tobytes()
    st = _states(name, 32)
    if full:
        out["unweighted losses"] = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
        out["unweighted gradients"] = agent._grad.cpu().numpy().tobytes()
        for step in range(3):
            out["losses of Adam step %d" % step] = agent._learn(_batch(name)).cpu().numpy().tobytes()
        for a in ARENAS:
            out["after three steps: " + a] = getattr(agent, a).cpu().numpy().tobytes()
        assert (agent._count.cpu().numpy() == 3).all()
        for which in (0, 1):
            for n in (1, 2, 32):
                out["q_values %d n=%d" % (which, n)] = agent._q_values(which, K - 1, np.stack(st[:n])).cpu().numpy().tobytes()
    for which in (0, 1) if full else (0,):
        act = int(agent._best_action(which, K - 1, st[1]))
        out["act_host %d" % which] = agent._q_out[0].cpu().numpy().tobytes() + bytes([act])
    agent._destroy_handle()
    return out


def _assert_same(on, off):
    assert on.keys() == off.keys()
    for what in off:
        assert on[what] == off[what], what


@pytest.mark.parametrize("name", NAMES)
def test_mode_on_bytes_are_mode_off_bytes(name, monkeypatch):
    full = name != "workload"  # (the workload's widths: one step and one acting call)
    _modes(monkeypatch, None)
    off = _everything(name, full)
    _modes(monkeypatch, "mfma")
    on = _everything(name, full)
    _assert_same(on, off)


def test_the_three_switches_together(monkeypatch):
    name = D.CROSS_MODES_ROW
    assert X.M.mx_layers(*D.ROWS[name][:2]), "the row has layers the conv modes move"
    _modes(monkeypatch, None, "bf16x3", "bf16x3")
    off = _everything(name)
    _modes(monkeypatch, "mfma", "bf16x3", "bf16x3")
    on = _everything(name)
    _assert_same(on, off)
    _modes(monkeypatch, None)
    assert _everything(name)["gradient arena"] != off["gradient arena"]  # (the other switches were on: the bytes moved)


@pytest.mark.parametrize("name", ["f65", "f448", "two_hidden"])
def test_best_actions_equals_the_loop(name, monkeypatch):
    """idqn_act_host_many_impala (k_imp_act_many_d0, untouched) against the loop of idqn_act_host, whose captured graph holds
    the route the handle was created with"""
    _modes(monkeypatch, "mfma")
    K = D.ROWS[name][3]
    agent = _agent(name)
    states = _states(name, 9)
    agent.act_many_imp_sizes = (1, 2, 9)
    for n in (1, 2, 9):
        heads = [(e + n) % K for e in range(n)]
        acts = agent._best_actions(1 if n == 2 else 0, heads, states[:n])
        assert agent.__dict__.get("_act_many_imp_ok") is True, "this is the loop"
        rows = agent._q_out[:n].cpu().numpy().copy()
        for e in range(n):
            a1 = int(agent._best_action(1 if n == 2 else 0, heads[e], states[e]))
            assert agent._q_out[0].cpu().numpy().tobytes() == rows[e].tobytes() and a1 == int(acts[e]), (n, e)
    agent._destroy_handle()


def test_a_smaller_batch_after_a_larger_one(monkeypatch):
    """B = 33 (two sample blocks), then B = 5 on the same handle: a fresh handle's B = 5 step"""
    from slimdqn import _hip

    _modes(monkeypatch, "mfma")
    name = D.HISTORY_ROW
    assert D.ROWS[name][4] == 33
    used = _agent(name)
    used._learn(_batch(name), flags=_hip.F_GRADS_ONLY)
    l_used = used._learn(_batch(name, 5), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    g_used = used._grad.cpu().numpy().tobytes()
    h_used = used._debug("imp_hid").cpu().numpy().tobytes()
    fresh = _agent(name)
    fresh._ensure_handle(33)
    l_fresh = fresh._learn(_batch(name, 5), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    assert l_used == l_fresh and g_used == fresh._grad.cpu().numpy().tobytes()
    K, Dh = D.ROWS[name][3], D.dense0(name)[1]
    n = 2 * K * 5 * Dh * 4  # what the B = 5 step wrote: [2K][5][D]
    assert h_used[:n] == fresh._debug("imp_hid").cpu().numpy().tobytes()[:n]


def test_a_used_handle_equals_a_fresh_one(monkeypatch):
    """tests/test_gpu_impala_mx.py's history (step, Q-values, acting with one state and nine, target update and sync, a
    second step, interleaved) with Dense_0 on the matrix cores as well: that test turns IDQN_IMP_CONV on itself"""
    monkeypatch.setenv(VAR, "mfma")
    X.test_a_used_handle_equals_a_fresh_one(monkeypatch)


def test_replay_sourced_step_is_gather_then_learn(monkeypatch):
    """the replay-sourced step under the mode is the mode's own step on the gathered batch, whose bytes are the default's
    (test_mode_on_bytes_are_mode_off_bytes)"""
    monkeypatch.setenv(VAR, "mfma")
    X.test_replay_sourced_step_is_gather_then_learn(monkeypatch)


def _grad_bar(name, k, leaf):
    """tests/test_gpu_impala.py's own bar (2e-5, or 4 x the float32 autograd's error), evaluated on this file's table"""
    table, G.S = G.S, D
    try:
        return G._grad_bar(name, k, leaf)
    finally:
        G.S = table


def test_row_against_the_oracle(monkeypatch):
    from slimdqn import _hip

    _modes(monkeypatch, "mfma")
    name = D.ORACLE_ROW
    obs, feats, A, K, B, p, pt, batch = D.case(name)
    want = D.oracle(name)
    agent = _agent(name)
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    Gr = agent._flat_grad()
    for k in range(K):
        w = want[k]
        print(name, k, "loss", losses[k], w["loss"])
        errs = {leaf: np.abs(Gr[leaf][k] - g).max() / (np.abs(g).max() + 1e-300) for leaf, g in w["grads"].items()}
        for leaf, err in errs.items():  # every figure first, then the bars
            print(name, k, leaf, "relative gradient error", err, "bar", _grad_bar(name, k, leaf))
        q = agent.q_values(agent.params, batch[0], k).cpu().numpy()
        qt = agent.q_values(agent.target_params, batch[3], k).cpu().numpy()
        print(name, k, "Q error", np.abs(q - w["q"]).max(), "target Q error", np.abs(qt - w["q_next"]).max())
        assert abs(losses[k] - w["loss"]) <= 1e-5 * max(1.0, abs(w["loss"])), (k, losses[k], w["loss"])
        for leaf, err in errs.items():
            assert err <= _grad_bar(name, k, leaf), (leaf, err)
        assert np.abs(q - w["q"]).max() <= 1e-5 * max(1.0, np.abs(w["q"]).max())
        assert np.abs(qt - w["q_next"]).max() <= 1e-5 * max(1.0, np.abs(w["q_next"]).max())
        row = np.sort(w["q"][1])
        if row[-1] - row[-2] > 1e-4:  # (a near-tie of the oracle's own row decides nothing)
            assert int(agent._best_action(0, k, np.asarray(batch[0][1]))) == int(np.argmax(w["q"][1]))
    agent._destroy_handle()


def mode_digest(name="f257"):
    return hashlib.sha256(b"".join(v for _, v in sorted(_everything(name).items()))).hexdigest()


CHILD = r"""
import json, sys, os
assert not any(v in os.environ for v in ("IDQN_IMP_D0", "IDQN_IMP_CONV", "IDQN_IMP_WGRAD"))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_impala_d0_mx as Y
print("RESULT" + json.dumps(Y.mode_digest()))
"""


def test_a_process_that_never_had_the_variable(monkeypatch):
    """``valu`` and ``mfma`` here against a child process that never had the variable: the same bytes of everything"""
    env = dict(os.environ)
    for s in (VAR, CONV, WGRAD, "IDQN_HIP_LIB"):
        env.pop(s, None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    unset = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])
    _modes(monkeypatch, "valu")
    assert mode_digest() == unset
    _modes(monkeypatch, "mfma")
    assert mode_digest() == unset
