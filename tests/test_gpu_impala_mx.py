"""The impala matrix-core conv mode on the device (IDQN_IMP_CONV=bf16x3, csrc/impala_mx_kernels.h), row by row of
tests/impala_mx_shapes.py: the switch and the route (``idqn_profile_table`` names ``k_imp_conv_mx`` for exactly the eligible
layers), every row against the fp64 oracle at the bars of tests/test_gpu_impala.py (imported, not restated), three chained Adam
steps, the weighted step with |TD|, two fresh handles, per-state independence of every acting route, the ineligible layers'
bytes, the mode-off path against a child process that never saw the variable, and a used handle against a fresh one.

The library reads the switch when a handle is created; every agent here creates its own under ``monkeypatch.setenv``."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from collections import Counter, namedtuple

import numpy as np
import pytest

import impala_mx_shapes as M
import test_gpu_impala as G  # the bars: _grad_bar's 2e-5 with the 4 x f32_errors fallback, and the loss / Q / stage figures below

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(M.ROWS)
VAR = "IDQN_IMP_CONV"
ARENAS = ("_online", "_target", "_mu", "_nu", "_count", "_cum")


def _agent(name):
    from slimdqn.networks.idqn import iDQN

    obs, feats, A, K, B, p, pt, batch = M.case(name)
    agent = iDQN(0, obs, A, K, feats, "impala", M.LR, 0.99, 1, 1, 10**9, 10**9, adam_eps=M.EPS)
    agent._load_flat(agent._online, p)
    agent._load_flat(agent._target, pt)
    return agent


def _batch(name):
    return Batch(*[np.array(a) for a in M.case(name)[7]])


def _grad_bar(name, k, leaf):
    """tests/test_gpu_impala.py's own bar (2e-5, or 4 x the float32 autograd's error), evaluated on this file's table"""
    table, G.S = G.S, M
    try:
        return G._grad_bar(name, k, leaf)
    finally:
        G.S = table


def _conv_launches(agent, batch):
    from slimdqn import _hip

    agent._learn(batch, flags=_hip.F_PROFILE_ALL | _hip.F_GRADS_ONLY)
    buf = C.create_string_buffer(1 << 14)
    _hip.check(_hip.lib().idqn_profile_table(agent._handle, buf, len(buf)), "idqn_profile_table")
    rows = [ln.split("\t") for ln in buf.value.decode().splitlines()]
    return {r[0]: int(r[2]) for r in rows if r[0].startswith("k_imp_conv")}, [r[0] for r in rows]


@pytest.mark.parametrize("name", NAMES)
def test_switch_and_route(name, monkeypatch):
    from slimdqn import _hip

    obs, feats, A, K, B, *_ = M.case(name)
    monkeypatch.setenv(VAR, "bf16x3")
    agent = _agent(name)
    got, _ = _conv_launches(agent, _batch(name))
    fwd, bwd = M.expected_launches(obs, feats)
    assert got == dict(Counter(fwd + bwd)), (got, Counter(fwd + bwd))
    assert "k_imp_conv<u8>" in got and not any(n.startswith("k_imp_conv_mx<u8") for n in got)
    if name != "workload":
        return
    # a garbage value is refused at create, with nothing allocated; non-impala handles ignore the variable
    import torch

    monkeypatch.setenv(VAR, "bf16")
    bad = _agent("one_row")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    with pytest.raises(Exception) as e:
        bad._ensure_handle(4)
    assert VAR in str(e.value) and "valu or bf16x3" in str(e.value) and "'bf16'" in str(e.value), str(e.value)
    assert bad._handle is None
    assert torch.cuda.mem_get_info()[0] == free0
    from slimdqn.networks.idqn import iDQN

    fc = iDQN(0, 8, 4, 2, [16, 16], "fc", 1e-3, 0.99, 1, 1, 10**9, 10**9)
    fc._ensure_handle(8)
    assert fc._handle is not None


@pytest.mark.parametrize("name", NAMES)
def test_row_against_the_oracle(name, monkeypatch):
    from slimdqn import _hip

    monkeypatch.setenv(VAR, "bf16x3")
    obs, feats, A, K, B, p, pt, batch = M.case(name)
    want = M.oracle(name)
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
        # the kept buffers of the step just run: nets [online 0..K-1 | target 0..K-1] x B samples
        stage_errs = []
        for which in (0, 1):
            c0s, pools, stacks = M.stage_outputs(name, k, which)
            for si in range(3):
                for nm, ref in (("imp_c0_%d" % si, c0s[si]), ("imp_pool%d" % si, pools[si]), ("imp_stack%d" % si, stacks[si])):
                    got = agent._debug(nm).cpu().numpy()[(which * K + k) * ref.size : (which * K + k + 1) * ref.size].reshape(ref.shape)
                    stage_errs.append((nm, which, np.abs(got - ref).max(), 1e-5 * max(1.0, np.abs(ref).max())))
                    if nm.startswith("imp_c0") and which == 0:
                        flips = int((M.pool_selection(got) != M.pool_selection(ref)).sum())
                        print(name, k, nm, "pool windows whose selection differs from fp64's:", flips)
        for nm, which, err, bar in stage_errs:
            print(name, k, nm, which, "stage error", err, "bar", bar)
        assert abs(losses[k] - w["loss"]) <= 1e-5 * max(1.0, abs(w["loss"])), (k, losses[k], w["loss"])
        for leaf, err in errs.items():
            assert err <= _grad_bar(name, k, leaf), (leaf, err)
        for nm, which, err, bar in stage_errs:
            assert err <= bar, (nm, which, err)
        q = agent.q_values(agent.params, batch[0][:n32], k).cpu().numpy()
        assert np.abs(q - w["q"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q"]).max())
        qt = agent.q_values(agent.target_params, batch[3][:n32], k).cpu().numpy()
        assert np.abs(qt - w["q_next"][:n32]).max() <= 1e-5 * max(1.0, np.abs(w["q_next"]).max())
        i = min(1, B - 1)
        row = np.sort(w["q"][i])
        if row[-1] - row[-2] > 1e-4:  # (a near-tie of the oracle's own row decides nothing)
            assert int(agent._best_action(0, k, np.asarray(batch[0][i]))) == int(np.argmax(w["q"][i]))


@pytest.mark.parametrize("name", NAMES)
def test_three_chained_steps(name, monkeypatch):
    """As tests/test_gpu_impala.py::test_three_chained_steps, its bars unchanged.

    Row ``workload`` is the sensitive one: at the parameters after the first step, head 1's Stack-1 ``c0`` has a pool window
    whose two largest inputs are 3.5e-7 apart at 0.55 in fp64 (six float32 ulps).  A kernel that chains all six partial
    products of a pass into one accumulator selected the runner-up there on the device, which put that step's gradients 3e-4
    of a leaf's largest magnitude off and one ``Stack_0/Conv_2/kernel`` element 1.60 lr from the oracle (bar 1.01 lr); with
    the small products and x0 w0 in accumulators of their own (csrc/impala_mx_kernels.h) every selection equals fp64's.  The
    selections are printed per step, head and Stack."""
    from oracle import qnet_ref as Q
    from oracle import torch_ref as T

    monkeypatch.setenv(VAR, "bf16x3")
    obs, feats, A, K, B, p, pt, batch = M.case(name)
    agent = _agent(name)
    b = _batch(name)
    for step in range(3):
        before = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        agent._learn(b)
        after = {s: agent._flat(getattr(agent, s)) for s in ("_online", "_mu", "_nu")}
        for k in range(K):
            _, grads = T.loss_and_grads(Q.head(before["_online"], k), Q.head(pt, k), batch, "impala", M.GAMMA_N)
            for si, ref in enumerate(M.stage_outputs_of(Q.head(before["_online"], k), batch[0])[0]):  # a figure, not a bar
                got = agent._debug("imp_c0_%d" % si).cpu().numpy()[k * ref.size : (k + 1) * ref.size].reshape(ref.shape)
                print(name, step, k, "imp_c0_%d" % si, "pool windows whose selection differs from fp64's:",
                      int((M.pool_selection(got) != M.pool_selection(ref)).sum()))
            for leaf, g in grads.items():
                th, m, v = Q.adam_update(before["_online"][leaf][k].astype(np.float64), g, before["_mu"][leaf][k].astype(np.float64),
                                         before["_nu"][leaf][k].astype(np.float64), step, M.LR, M.EPS)
                gm = np.abs(g).max() + 1e-300
                worst = np.unravel_index(np.abs(after["_online"][leaf][k] - th).argmax(), th.shape)
                print(name, step, k, leaf, "mu error / max |g|", np.abs(after["_mu"][leaf][k] - m).max() / gm, "worst parameter error / lr",
                      np.abs(after["_online"][leaf][k] - th)[worst] / M.LR, "where the oracle's gradient / max |g| is", g[worst] / gm)
                assert np.abs(after["_mu"][leaf][k] - m).max() <= 1e-4 * gm, (step, leaf)
                assert np.abs(after["_nu"][leaf][k] - v).max() <= 1e-4 * gm * gm, (step, leaf)
                err = np.abs(after["_online"][leaf][k] - th)
                assert err.max() <= M.LR * 1.01 + 1e-6, (step, leaf)
                assert np.median(err) <= 2e-5, (step, leaf, np.median(err))
    assert (agent._count.cpu().numpy() == 3).all()


@pytest.mark.parametrize("name", NAMES)
def test_weighted_step_and_td(name, monkeypatch):
    import torch

    from slimdqn import _hip

    monkeypatch.setenv(VAR, "bf16x3")
    obs, feats, A, K, B, p, pt, batch = M.case(name)
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
        loss, grads, td_want = M.weighted_oracle(name, k, wts)
        assert abs(losses[k] - loss) <= 1e-5 * max(1.0, abs(loss))
        assert np.abs(td[k] - td_want).max() <= 1e-5 * max(1.0, np.abs(td_want).max())
        for leaf, g in grads.items():
            assert np.abs(Gr[leaf][k] - g).max() <= _grad_bar(name, k, leaf) * (np.abs(g).max() + 1e-300), leaf


def _step_bytes(name):
    """losses and gradients of a gradient-only step, then parameters and both moments after a full step, on a fresh agent"""
    from slimdqn import _hip

    agent = _agent(name)
    losses = agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY).cpu().numpy().tobytes()
    grads = agent._grad.cpu().numpy().tobytes()
    agent._learn(_batch(name))
    out = (losses, grads) + tuple(getattr(agent, s).cpu().numpy().tobytes() for s in ("_online", "_mu", "_nu"))
    agent._destroy_handle()
    return out


@pytest.mark.parametrize("name", ["all_mx", "mixed_mx_valu", "workload"])
def test_two_fresh_handles_give_equal_bytes(name, monkeypatch):
    monkeypatch.setenv(VAR, "bf16x3")
    assert _step_bytes(name) == _step_bytes(name)


def _states(name):
    obs, feats, A, K, B, p, pt, batch = M.case(name)
    pool = [np.asarray(s) for s in list(batch[0]) + list(batch[3])]
    return [pool[i % len(pool)] for i in range(9)]


@pytest.mark.parametrize("name", ["all_mx", "mixed_valu_mx", "tile_plus"])
def test_a_states_result_does_not_depend_on_the_batch(name, monkeypatch):
    """Row e of idqn_q_values on n states = the call on state e alone; idqn_act_host_many_impala = the loop of idqn_act_host."""
    monkeypatch.setenv(VAR, "bf16x3")
    K = M.ROWS[name][3]
    agent = _agent(name)
    states = _states(name)
    for which in (0, 1):
        q = agent._q_values(which, K - 1, np.stack(states)).cpu().numpy().copy()
        for e, s in enumerate(states):
            assert agent._q_values(which, K - 1, s[None]).cpu().numpy().tobytes() == q[e].tobytes(), (which, e)
    agent.act_many_imp_sizes = (1, 2, 9)
    for n in (1, 2, 9):
        heads = [(e + n) % K for e in range(n)]
        acts = agent._best_actions(1 if n == 2 else 0, heads, states[:n])
        assert agent.__dict__.get("_act_many_imp_ok") is True, "this is the loop"
        rows = agent._q_out[:n].cpu().numpy().copy()
        for e in range(n):
            a1 = int(agent._best_action(1 if n == 2 else 0, heads[e], states[e]))
            assert agent._q_out[0].cpu().numpy().tobytes() == rows[e].tobytes() and a1 == int(acts[e]), (n, e)


def test_replay_sourced_step_is_gather_then_learn(monkeypatch):
    import test_gpu_fc_learn_on_replay as R  # its buffers, seed choice and byte comparison, on a configuration of this file

    monkeypatch.setenv(VAR, "bf16x3")
    R.CONFIGS.setdefault("impala_mx_12x10x2", ("impala", (12, 10), np.uint8, 2, (12, 10, 2), [16, 32, 32, 15], 2, 3, 5, "iDQN"))
    assert M.mx_layers((12, 10, 2), [16, 32, 32, 15])
    R._identity("impala_mx_12x10x2", R._buffer)


def test_ineligible_layers_keep_the_mode_off_bytes(monkeypatch):
    """Row mixed_valu_mx: Stack 0 is wholly ineligible and is fed the same frames in both modes, so its Conv_0 output, pool
    output and Stack output are the mode-off handle's bytes; Stack 1, on the matrix cores, is not (the test can fail)."""
    name = "mixed_valu_mx"
    from slimdqn import _hip

    out = {}
    for mode in ("valu", "bf16x3"):
        monkeypatch.setenv(VAR, mode)
        agent = _agent(name)
        agent._learn(_batch(name), flags=_hip.F_GRADS_ONLY)
        out[mode] = {nm: agent._debug(nm).cpu().numpy().tobytes() for nm in ("imp_c0_0", "imp_pool0", "imp_stack0", "imp_c0_1", "imp_stack1")}
        agent._destroy_handle()
    for nm in ("imp_c0_0", "imp_pool0", "imp_stack0"):
        assert out["valu"][nm] == out["bf16x3"][nm], nm
    assert out["valu"]["imp_c0_1"] != out["bf16x3"]["imp_c0_1"]


def mode_off_digest(name="mixed_mx_valu"):
    return hashlib.sha256(b"".join(_step_bytes(name))).hexdigest()


CHILD = r"""
import json, sys, os
assert "IDQN_IMP_CONV" not in os.environ
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "i-dqn_amd")]
import test_gpu_impala_mx as X
print("RESULT" + json.dumps(X.mode_off_digest()))
"""


def test_valu_is_the_unset_path(monkeypatch):
    """IDQN_IMP_CONV=valu here against a child process that never had the variable: the same bytes of a full step, and the
    launches of the vector-ALU path only."""
    env = dict(os.environ)
    for s in (VAR, "IDQN_HIP_LIB"):
        env.pop(s, None)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    unset = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])
    monkeypatch.setenv(VAR, "valu")
    assert mode_off_digest() == unset
    got, _ = _conv_launches(_agent("mixed_mx_valu"), _batch("mixed_mx_valu"))
    assert got and not any("_mx" in n for n in got), got
    monkeypatch.setenv(VAR, "bf16x3")
    assert mode_off_digest() != unset  # the mode changes the bytes: the comparison above can fail


def test_a_used_handle_equals_a_fresh_one(monkeypatch):
    """step, Q-values, acting (one state and nine), target update, target sync, a second step on ONE mode-on handle; each op
    is repeated on a fresh agent given the used agent's arenas from just before it.  Results and arenas: the same bytes."""
    import torch

    monkeypatch.setenv(VAR, "bf16x3")
    name = "all_mx"
    K = M.ROWS[name][3]
    states = _states(name)

    def learn(a):
        return a._learn(_batch(name)).cpu().numpy().tobytes()

    def q_values(a):
        return a._q_values(0, 1, np.stack(states[:3])).cpu().numpy().tobytes()

    def act_host(a):
        act = int(a._best_action(1, K - 1, states[3]))
        return a._q_out[0].cpu().numpy().tobytes() + bytes([act])

    def act_many(a):
        a.act_many_imp_sizes = (9,)
        acts = a._best_actions(0, [e % K for e in range(9)], states)
        assert a.__dict__.get("_act_many_imp_ok") is True
        return a._q_out[:9].cpu().numpy().tobytes() + acts.tobytes()

    def target_update(a):
        a._local_target_update()
        return b""

    def target_sync(a):
        a._local_target_sync()
        return b""

    used = _agent(name)
    used._ensure_handle(32)
    for i, op in enumerate([learn, q_values, act_host, act_many, target_update, act_host, target_sync, q_values, learn, act_many]):
        torch.cuda.synchronize()
        before = {a: getattr(used, a).clone() for a in ARENAS}
        got = op(used)
        torch.cuda.synchronize()
        fresh = _agent(name)
        fresh._ensure_handle(32)
        for a in ARENAS:
            getattr(fresh, a).copy_(before[a])
        torch.cuda.synchronize()
        want = op(fresh)
        torch.cuda.synchronize()
        assert got == want, (i, op.__name__)
        for a in ARENAS:
            assert getattr(used, a).cpu().numpy().tobytes() == getattr(fresh, a).cpu().numpy().tobytes(), (i, op.__name__, a)
        fresh._destroy_handle()
