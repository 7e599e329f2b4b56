"""GPU: every entry on a USED handle gives the bits it gives on a FRESH one (tests/handle_history.py does the driving).

The other fp tests build a new agent per case, so each of them runs on a handle whose workspaces were zeroed a moment ago and
sees one batch shape.  Here ONE handle, sized once, takes a script of calls whose shapes and kinds alternate -- gradient steps
of every launch route (one, two, three-or-more and multiples of eight 32-sample blocks, ragged and full), Q-value calls, host
and device acting, target copies, two-phase steps, weighted steps and replay-sourced steps -- and after each call a newly created
agent that was given the used agent's state from just before the call repeats it.  Outputs and all state arenas must be equal
byte for byte: the steps are deterministic, so a pad lane, a zero border, a split-K partial, a last-arriver counter, a gate word
or a sticky setting left by a call of another shape shows as a difference.  The fresh handles are what the oracle tests vouch for.

The shapes are the smallest that still reach every route, not the workload's.

Ops that differ BY DESIGN between a used and a fresh handle (a legitimate reordering, not stale state) would be listed here and
compared against ``oracle/`` at the bar of their own test file instead:

    | script | op | reason |
    |---|---|---|
    (none)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import handle_history as H
from handle_history import (act_dev, act_host, grads_then_adam, learn, learn_on_replay, q_values, target_sync, target_update,
                            weighted_learn)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-3, gamma=0.99, n=1, eps=1e-6)


@pytest.fixture(params=["bf16x3", "f32"])
def conv_mode(request, monkeypatch):
    """Conv arithmetic of the agents a test creates (read by idqn_create from IDQN_CONV), as in test_gpu_fp_path.py."""
    monkeypatch.setenv("IDQN_CONV", request.param)
    return request.param


def _idqn(obs, feats, A, K, arch="cnn"):
    from slimdqn.networks.idqn import iDQN

    return lambda: iDQN(3, obs, A, K, feats, arch, HYPER["lr"], HYPER["gamma"], HYPER["n"], 1, 10**9, 10**9, adam_eps=HYPER["eps"])


def _run(make_agent, max_batch, script):
    seen = []
    n = H.run_script(make_agent, max_batch, script, on_op=lambda i, op, out: seen.append((op.kind, out)))
    assert n == len(script) == len(seen)
    for kind, out in seen:  # the compared numbers are numbers
        for name, v in out.items():
            assert np.isfinite(v).all(), (kind, name)


PLANE = ((20, 20, 4), [32, 64, 32, 256], 5)  # J = 256: the routes of three and more blocks are open to it
# nb:           8            1r          4r          1           8r          2r          2          1r         8
PLANE_SCRIPT = [
    learn(256, 1), q_values(0, 0, 1, 101), act_host(0, 1, 102),                 # (acting graph of net (0, 1): captured)
    weighted_learn(64, 20),                                                     # sticky is_weight / td_abs, then another B
    learn(20, 2), q_values(1, 1, 5, 103), act_host(0, 1, 104, lazy=True),       # (the same net on another state: replayed)
    learn(100, 3), act_dev(1, 0, 105), target_sync(),
    learn_on_replay(32, 21),                                                    # h->rp must not stick: the same B, plain
    learn(32, 4), q_values(0, 1, 32, 106),
    grads_then_adam(100, 22),
    learn(250, 5), act_host(1, 0, 107), target_update(),                        # (another net: captured)
    learn(33, 6), q_values(1, 0, 5, 108),
    learn(64, 7), act_dev(0, 0, 109),
    learn(7, 8), act_host(0, 1, 110), q_values(0, 0, 32, 111),
    learn(256, 9), q_values(1, 1, 1, 112),
]


def test_plane_cnn_path(conv_mode):
    obs, feats, A = PLANE
    assert [op.args["B"] for op in PLANE_SCRIPT if op.kind == "learn"] == [256, 20, 100, 32, 250, 33, 64, 7, 256]
    _run(_idqn(obs, feats, A, 2), 256, PLANE_SCRIPT)


def test_odd_frame_geometry(conv_mode):
    """(9, 13, 4) -- Conv_0 pads (3, 4) on both axes, Conv_1 sees a 3x4 input, F = 128 (tests/test_gpu_conv_geometry.py) --
    with B = 33, 5, 40 in turn: pad lanes and compact slot addressing at a block size the other scripts do not have."""
    script = [learn(33, 1), q_values(0, 1, 5, 101), learn(5, 2), act_host(0, 0, 102), learn(40, 3), q_values(1, 0, 32, 103),
              learn(33, 4), act_host(1, 1, 104, lazy=True), grads_then_adam(5, 5), learn(40, 6), act_dev(0, 1, 105)]
    assert [op.args["B"] for op in script if op.kind in H.BATCH_OPS] == [33, 5, 40, 33, 5, 40]
    _run(_idqn((9, 13, 4), [32, 64, 32, 128], 4, 2), 64, script)


def test_nature_shape():
    """The conv launch plans and the fused Dense_0 update of the (84, 84, 4) / [32, 64, 64, 512] network."""
    script = [learn(64, 1), act_host(0, 0, 101), learn(20, 2), q_values(1, 1, 32, 102), learn(32, 3),
              act_host(1, 1, 103, lazy=True), learn(33, 4), q_values(0, 0, 32, 104)]
    _run(_idqn((84, 84, 4), [32, 64, 64, 512], 6, 2), 64, script)


def test_general_shape_cnn():
    """csrc/gcnn_kernels.h: one channel, no hidden dense layer, 40 actions."""
    script = [learn(33, 1), act_host(0, 2, 101), learn(5, 2), q_values(1, 0, 5, 102), target_sync(), learn(32, 3),
              q_values(0, 1, 32, 103), target_update(), learn(40, 4), act_host(1, 1, 104), learn(1, 5), q_values(0, 2, 1, 105)]
    _run(_idqn((20, 20, 1), [8, 8, 8], 40, 3), 64, script)


@pytest.mark.parametrize("obs,feats,A,K", [
    (8, [100, 100], 4, 3),        # the one-launch kernel (B <= 32) and the MFMA step behind it
    (12, [512, 300, 64], 6, 2),   # the LDS kernels, 8-sample blocks
    (10, [700, 33], 3, 2),        # the generic kernel
], ids=["one_launch", "lds_8_sample_blocks", "generic"])
def test_mlp(obs, feats, A, K):
    """One script per kernel family of test_gpu_fp_path.py::test_ragged_batches_and_shapes_against_oracle."""
    script = [learn(70, 1), q_values(0, 0, 5, 101), learn(7, 2), act_host(0, K - 1, 102), target_sync(), learn(32, 3),
              q_values(1, 1, 32, 103), learn(64, 4), act_dev(1, 0, 104), target_update(), learn(12, 5),
              act_host(0, 0, 105, lazy=True), learn(33, 6), q_values(0, 1, 1, 106)]
    _run(_idqn(obs, feats, A, K, arch="fc"), 70, script)


def test_dqn_without_the_head_axis():
    from slimdqn.networks.dqn import DQN

    obs, feats, A = PLANE
    script = [learn(64, 1), act_host(0, 0, 101), learn(20, 2), act_dev(1, 0, 102), learn(32, 3), act_host(0, 0, 103),
              q_values(0, 0, 5, 104)]
    _run(lambda: DQN(3, obs, A, feats, "cnn", HYPER["lr"], HYPER["gamma"], HYPER["n"], 1, 10**9, adam_eps=HYPER["eps"]), 64, script)


def test_iiqn():
    """The quantile heads: gate words, the dispatch-order plan and the GEMM routes change with NB = N x blocks; the seven-launch
    acting graph shares buffers with the batched route."""
    from oracle import make_golden as G
    from slimdqn.networks.iiqn import iIQN

    obs, A, feats, K, _, N = G.IQN_CASES["iqn_small"]
    p, pt, _, _ = G.iqn_case_inputs("iqn_small")
    hy = G.FP_HYPER

    def make():
        agent = iIQN(0, obs, A, K, feats, "cnn", hy["lr"], hy["gamma"], hy["n"], 1, 10**9, 10**9, adam_eps=hy["eps"], n_quantiles=N)
        agent._load_flat(agent._online, p)
        agent._load_flat(agent._target, pt)
        return agent

    script = [learn(96, 1), q_values(0, 0, 64, 101), act_host(0, 1, 102),
              learn(45, 2), act_host(1, 0, 103),
              weighted_learn(64, 20),
              learn(32, 3), q_values(1, 1, 1, 104),
              learn_on_replay(32, 21),
              learn(64, 4), q_values(0, 1, 33, 105), act_host(0, 1, 106, lazy=True),
              learn(33, 5), act_host(1, 1, 107)]
    assert [op.args["B"] for op in script if op.kind == "learn"] == [96, 45, 32, 64, 33]
    _run(make, 96, script)


STEP_GRAPH_CHILD = r"""
import hashlib, json, sys, os
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
import numpy as np, torch
from collections import namedtuple
from oracle import qnet_ref as Q
from slimdqn.networks.idqn import iDQN
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
obs, feats, A, K = (20, 20, 4), [32, 64, 32, 256], 5, 2
agent = iDQN(3, obs, A, K, feats, "cnn", 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-6)
agent._ensure_handle(64)
handle = agent._handle
# two sets of device-resident inputs, used in turn: the graph key is their pointers and B
def device_batch(B):  # already in the types the step reads, so that no call converts (and so moves) them
    s, a, r, s2, t = Q.synthetic_batch(40 + B, B, obs, A, "cnn")
    return Batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (s, a, r, s2, t.astype(np.uint8))))
sets = {B: device_batch(B) for B in (32, 64)}
ptrs = {B: [x.data_ptr() for x in sets[B]] for B in sets}
steps = []
for B in (32, 64, 32, 64, 32, 64):  # per key: eager, captured, replayed -- interleaved with the other key
    losses = agent._learn(sets[B]).cpu().numpy()
    assert agent._handle is handle and sorted(x.data_ptr() for x in agent._keep) == sorted(ptrs[B])  # (the step read these very tensors)
    rec = {"losses": losses.view(np.uint32).tolist()}
    for name in ("_online", "_target", "_mu", "_nu", "_count", "_cum"):
        rec[name] = hashlib.sha256(getattr(agent, name).cpu().numpy().tobytes()).hexdigest()
    steps.append(rec)
print("RESULT" + json.dumps(steps))
"""


def _child(**env):
    e = dict(os.environ)
    e.update(env)
    e.pop("IDQN_HIP_LIB", None)  # the shipped library
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + STEP_GRAPH_CHILD], env=e, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1][len("RESULT"):])


def test_step_graph_keys_interleaved():
    """IDQN_STEP_GRAPH=1 (read once per process, hence the children): two keys of different B take turns on one handle, so
    each is issued eagerly, then captured, then replayed with the other key's steps in between -- against the same steps with
    the switch off, after every step."""
    got, want = _child(IDQN_STEP_GRAPH="1"), _child(IDQN_STEP_GRAPH="0")
    assert len(got) == len(want) == 6
    for s, (a, b) in enumerate(zip(got, want)):
        for name in b:
            assert a[name] == b[name], f"step {s} (B = {(32, 64)[s % 2]}): {name} differs with IDQN_STEP_GRAPH=1"
    assert len({rec["_online"] for rec in want}) == 6  # every step moved the parameters
