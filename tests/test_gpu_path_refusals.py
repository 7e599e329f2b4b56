"""Every entry of the C ABI that refuses a handle because of the path it runs (csrc/qnet.hip derives it per entry from
``cfg.arch``, ``h->gc.on``, ``h->imp.on`` and ``h->planes``): the refusing (handle kind, entry) pairs only, with arguments that are
otherwise valid, so that the path refusal is the one reached.

Per pair: the return code and the ``idqn_last_error()`` text equal the record in tests/golden/path_refusals.json; the handle's
arenas are byte-equal before and after the call and the stream is idle; a full step, Q-values and a host-state action on the
same handle then give the bytes a fresh handle gives.

The record was written once by this table (``TABLE``, ``entries``) against the library of the commit that merged the impala
architecture, so that a later restatement of those per-entry conditions is held to the codes and texts of that commit.  It is a
fixture: nothing here writes it.

Handles are the smallest of their kind: the smallest row of tests/fc_shapes.py (by arena size), the smallest geometry of
tests/test_gpu_general_shapes.py (and, for the one entry that looks at the action count first, the smallest with A <= 32), row
``odd_even`` of tests/impala_shapes.py, and the 20 x 20 x 4 frame of ``smoke()`` in both conv modes.  The accepting pairs belong
to the suites of the entries themselves.
"""
import ctypes as C
import functools
import json
import os
from collections import namedtuple

import numpy as np
import pytest

import fc_shapes as F
import impala_shapes as S

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_refusals.json")
ARENAS = ("_online", "_target", "_mu", "_nu", "_grad", "_count", "_losses")

_FC = min(F.INSIDE, key=lambda r: (F.layout(r.d0, r.feats, r.A)[2], r.d0))
# kind: (arch, obs, features, A, K, IDQN_CONV)
KINDS = {
    "fc": ("fc", _FC.d0, _FC.feats, _FC.A, _FC.K, None),
    "gcnn": ("cnn", (20, 20, 1), [8, 8, 8], 40, 3, None),
    # idqn_act_group_create names J > 512 and A > 32 before the path: the smallest of those geometries with A <= 32
    "gcnn_a4": ("cnn", (24, 24, 4), [32, 64, 64, 96], 4, 2, None),
    "impala": ("impala",) + tuple(S.ROWS["odd_even"][:4]) + (None,),
    "plane": ("cnn", (20, 20, 4), [32, 32, 32, 128], 5, 2, "bf16x3"),
    "f32": ("cnn", (20, 20, 4), [32, 32, 32, 128], 5, 2, "f32"),
}
B = 5  # samples of the served step and of every batch argument

STOP_AFTER, STOP_BEFORE = 4, 8  # IDQN_F_STOP_AFTER_DENSE0, IDQN_F_STOP_BEFORE_DENSE0_WGRAD (include/idqn_hip.h)
_REPLAY = ("idqn_learn_on_replay", "idqn_learn_on_replay_dev")
_REPLAY_FC = ("idqn_learn_on_replay_fc", "idqn_learn_on_replay_fc_dev", "idqn_learn_steps_on_replay_fc", "idqn_learn_steps_on_replay_fc_dev")
_PER = ("idqn_per_learn_on_replay", "idqn_per_learn_steps_on_replay")
_STOPS = ("idqn_learn_on_batch[stop_after_dense0]", "idqn_learn_on_batch[stop_before_dense0_wgrad]")
_IMPALA_ONLY = ("idqn_learn_steps_on_replay_fc", "idqn_learn_steps_on_replay_fc_dev", "idqn_iqn_learn_on_replay", "idqn_iqn_learn_on_replay_dev",
                "idqn_iqn_learn_on_batch", "idqn_iqn_q_values", "idqn_iqn_act_host", "idqn_iqn_act_host_begin", "idqn_iqn_act_host_many",
                "idqn_backward_rest", "idqn_export_dense0_factors", "idqn_dense0_factors", "idqn_finish_step_factored", "idqn_act_host_many_fc")
# the refusing pairs, kind by kind (every other pair of these entries is served, or refused for a reason that is not the path)
REFUSING = {
    "fc": _REPLAY + _STOPS + ("idqn_act_host_many", "idqn_act_group_create", "idqn_dp_create"),
    "gcnn": _REPLAY + _STOPS + ("idqn_act_host_many", "idqn_group_create", "idqn_dp_create"),
    "gcnn_a4": ("idqn_act_group_create",),
    "impala": _REPLAY + _PER + _STOPS + _IMPALA_ONLY + ("idqn_act_host_many", "idqn_group_create", "idqn_act_group_create", "idqn_dp_create"),
    "plane": _REPLAY_FC + ("idqn_act_host_many_fc", "idqn_group_create"),
    "f32": _REPLAY + _REPLAY_FC + _PER + ("idqn_act_host_many_fc", "idqn_group_create"),
}
TABLE = [(kind, entry) for kind, names in REFUSING.items() for entry in names]


def make_agent(kind):
    from slimdqn.networks.idqn import iDQN

    arch, obs, feats, A, K, _ = KINDS[kind]
    agent = iDQN(3, obs, A, K, list(feats), arch, 1e-3, 0.99, 1, 1, 10**9, 10**9, adam_eps=1e-6)
    agent._ensure_handle(32)
    return agent


def batch_of(kind):
    from oracle import qnet_ref as Q

    arch, obs, feats, A, K, _ = KINDS[kind]
    return Batch(*Q.synthetic_batch(11, B, obs, A, "fc" if arch == "fc" else "cnn"))


def entries(agent):
    """name -> call, for every entry of REFUSING: ring, rows, slots, sampler record and batch pointers are all set and in range."""
    import torch

    from slimdqn import _hip

    lib, h, q = _hip.lib(), agent._handle, _hip.current_stream()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    pin = torch.zeros(1 << 14, dtype=torch.uint8).pin_memory()
    ipin = torch.zeros(64, dtype=torch.int32).pin_memory()
    d, hp, ip = _hip.ptr(buf), C.c_void_p(pin.data_ptr()), C.c_void_p(ipin.data_ptr())
    arr, g = (C.c_void_p * 1)(h.value), C.c_void_p()
    per, pers = _hip.PerStep(), _hip.PerSteps()
    for rec in (per, pers):
        for f in ("nodes_dev", "max_priority_dev", "leaves_dev", "weights_dev", "td_abs_dev", "priorities_dev", "tree_scratch_dev"):
            setattr(rec, f, buf.data_ptr())
        rec.uniforms_host, rec.depth, rec.n_items = pin.data_ptr(), 4, 8
    uid = (C.c_char * 128)()
    fac, n1, n2 = C.c_void_p(), C.c_int64(), C.c_int64()
    obs = agent._obs
    fb, stack = (int(obs[0]) * int(obs[1]), int(obs[2])) if len(obs) == 3 else (4 * int(obs[0]), 1)  # frame bytes, frames per state
    calls = {
        "idqn_learn_on_replay": lambda: lib.idqn_learn_on_replay(h, d, 64, fb, d, ip, B, stack, B, 0, q),
        "idqn_learn_on_replay_dev": lambda: lib.idqn_learn_on_replay_dev(h, d, 64, fb, d, d, B, stack, B, 0, q),
        "idqn_learn_on_replay_fc": lambda: lib.idqn_learn_on_replay_fc(h, d, 64, fb, d, ip, B, stack, B, 0, q),
        "idqn_learn_on_replay_fc_dev": lambda: lib.idqn_learn_on_replay_fc_dev(h, d, 64, fb, d, d, B, stack, B, 0, q),
        "idqn_learn_steps_on_replay_fc": lambda: lib.idqn_learn_steps_on_replay_fc(h, d, 64, fb, d, ip, 2, B, stack, B, 0, q),
        "idqn_learn_steps_on_replay_fc_dev": lambda: lib.idqn_learn_steps_on_replay_fc_dev(h, d, 64, fb, d, d, 2, B, stack, B, 0, q),
        "idqn_per_learn_on_replay": lambda: lib.idqn_per_learn_on_replay(h, C.byref(per), d, 64, fb, d, B, stack, B, 0, q),
        "idqn_per_learn_steps_on_replay": lambda: lib.idqn_per_learn_steps_on_replay(h, C.byref(pers), d, 64, fb, d, 2, B, stack, B, 0, q),
        "idqn_learn_on_batch[stop_after_dense0]": lambda: lib.idqn_learn_on_batch(h, d, d, d, d, d, B, B, STOP_AFTER, q),
        "idqn_learn_on_batch[stop_before_dense0_wgrad]": lambda: lib.idqn_learn_on_batch(h, d, d, d, d, d, B, B, STOP_BEFORE, q),
        "idqn_iqn_learn_on_replay": lambda: lib.idqn_iqn_learn_on_replay(h, d, 64, fb, d, ip, d, B, stack, 0, q),
        "idqn_iqn_learn_on_replay_dev": lambda: lib.idqn_iqn_learn_on_replay_dev(h, d, 64, fb, d, d, d, B, stack, 0, q),
        "idqn_iqn_learn_on_batch": lambda: lib.idqn_iqn_learn_on_batch(h, d, d, d, d, d, d, B, 0, q),
        "idqn_iqn_q_values": lambda: lib.idqn_iqn_q_values(h, 0, 0, d, 1, d, d, None, q),
        "idqn_iqn_act_host": lambda: lib.idqn_iqn_act_host(h, 0, 0, hp, hp, d, ip, q),
        "idqn_iqn_act_host_begin": lambda: lib.idqn_iqn_act_host_begin(h, 0, 0, hp, hp, d, ip, q),
        "idqn_iqn_act_host_many": lambda: lib.idqn_iqn_act_host_many(h, 0, ip, hp, hp, 2, d, ip, q),
        "idqn_backward_rest": lambda: lib.idqn_backward_rest(h, q),
        "idqn_export_dense0_factors": lambda: lib.idqn_export_dense0_factors(h, d, d, q),
        "idqn_dense0_factors": lambda: lib.idqn_dense0_factors(h, C.byref(fac), C.byref(n1), C.byref(n2)),
        "idqn_finish_step_factored": lambda: lib.idqn_finish_step_factored(h, d, d, 1, 1, 0, 0, 0, 0, 0, 0, 3, q),
        "idqn_act_host_many": lambda: lib.idqn_act_host_many(h, 0, ip, hp, 2, d, ip, q),
        "idqn_act_host_many_fc": lambda: lib.idqn_act_host_many_fc(h, 0, ip, hp, 2, d, ip, q),
        "idqn_group_create": lambda: lib.idqn_group_create(arr, 1, C.byref(g)),
        "idqn_act_group_create": lambda: lib.idqn_act_group_create(arr, 1, C.byref(g)),
        "idqn_dp_create": lambda: lib.idqn_dp_create(h, uid, 0, 1, 0, C.byref(g)),
    }
    return calls, g, (buf, pin, ipin, uid)


def refuse(agent, entry):
    """(return code, error text, the out-handle of the create entries) of one refused call."""
    from slimdqn import _hip

    import torch

    calls, g, keep = entries(agent)
    torch.cuda.synchronize()  # (the buffers' fills are done: what the stream holds afterwards is the entry's)
    rc = calls[entry]()
    return int(rc), _hip.lib().idqn_last_error().decode(errors="replace"), g.value


def arenas(agent):
    import torch

    torch.cuda.synchronize()
    return {s: getattr(agent, s).cpu().numpy().tobytes() for s in ARENAS}


def served(agent, kind):
    """A full step, the Q-values of both nets and a host-state action on `agent`, as bytes."""
    b = batch_of(kind)
    agent._learn(b)
    out = arenas(agent)
    out["q"] = agent.q_values(agent.params, b.state[:3], 0).cpu().numpy().tobytes()
    out["q_target"] = agent.q_values(agent.target_params, b.next_state[:3], agent._K - 1).cpu().numpy().tobytes()
    out["action"] = int(agent._best_action(0, 0, np.asarray(b.state[1])))
    return out


@functools.lru_cache(maxsize=None)
def fresh(kind):
    return served(make_agent(kind), kind)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("kind,entry", TABLE)
def test_path_refusal(kind, entry, monkeypatch):
    import torch

    if KINDS[kind][5]:
        monkeypatch.setenv("IDQN_CONV", KINDS[kind][5])  # (read by idqn_create)
    else:
        monkeypatch.delenv("IDQN_CONV", raising=False)
    want = golden()[kind + "/" + entry]
    agent = make_agent(kind)
    before = arenas(agent)
    rc, text, out = refuse(agent, entry)
    print(kind, entry, rc, text)
    assert rc == want["rc"] and rc != 0, (rc, want["rc"])
    assert text == want["text"]
    assert out is None
    assert torch.cuda.current_stream().query(), "a refused entry left work on the stream"
    assert arenas(agent) == before
    assert served(agent, kind) == fresh(kind)


def test_the_record_covers_the_table_and_nothing_else():
    assert sorted(golden()) == sorted(k + "/" + e for k, e in TABLE)
