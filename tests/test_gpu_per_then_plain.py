"""GPU: a plain replay-sourced step behind prioritized calls on the same handle takes nothing of them -- the solo counterpart of
tests/test_gpu_group_per.py's "none may leak into the plain step".

``idqn_per_learn_on_replay`` and ``idqn_per_learn_steps_on_replay`` hand every inner step its own rows of importance weights and
|TD|; none of that may still be in force when the call has returned.  One handle runs a prioritized step, a prioritized call of
two steps and then a plain ``idqn_learn_on_replay*`` step on explicit slots; a twin handle whose six arenas are copies of the
first handle's as they stood just before the plain step runs only that plain step.  Everything is ``tobytes()`` equality.
The learner builders, the families and the smallest batch (1) are tests/test_gpu_per_steps.py's; the larger batch of each family
is there because a batch of one sample has the importance weight 1.0, which a leaked weight pointer would not show in the arenas.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_per_steps as P

pytestmark = pytest.mark.gpu


def _plain_step(learner, family, ring, slots, B):
    from slimdqn import _hip

    lib = _hip.lib()
    entry = lib.idqn_learn_on_replay_fc if P.FAMILIES[family][0] == "fc" else lib.idqn_learn_on_replay
    frames, n_frames, frame_bytes, rows, stack = ring
    _hip.check(entry(learner.agent._handle, _hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows), slots.ctypes.data, B, int(stack), B, 0,
                     _hip.current_stream()), "the plain step")


@pytest.mark.parametrize("family,B", [("lunar", 1), ("lunar", 5), ("plane_small", 1), ("plane_small", 32)])
def test_a_plain_step_after_prioritized_calls_equals_a_twin(family, B):
    import torch

    from slimdqn import _hip

    K = P.FAMILIES[family][6]
    used, twin = P._learner(family, B), P._learner(family, B)
    ring = used.rb.ring_view()[:5]
    rng = np.random.default_rng(31 + B)
    one, two = P._Rows(1, K, B), P._Rows(2, K, B)  # (sentinels: -7)
    U1, U2 = P._uniforms(rng, 1, B), P._uniforms(rng, 2, B)
    p = _hip.PerStep()
    P._fill(p, used, one, 0)
    p.uniforms_host, p.tau_dev = U1[0].ctypes.data, None
    _hip.check(_hip.lib().idqn_per_learn_on_replay(used.agent._handle, C.byref(p), _hip.ptr(ring[0]), int(ring[1]), int(ring[2]), _hip.ptr(ring[3]), B,
                                                   int(ring[4]), B, 0, _hip.current_stream()), "idqn_per_learn_on_replay")
    P._steps_call_checked(used, U2, two, B)
    torch.cuda.synchronize()
    rows_before = {k: v.clone() for r, tag in ((one, "1"), (two, "2")) for k, v in ((tag + n, t) for n, t in r.all().items())}
    assert (one.td >= 0).all().item() and (two.td >= 0).all().item(), "the prioritized calls wrote no |TD|"
    assert (used.agent._count.cpu().numpy() == 3).all()
    # the twin: the used handle's arenas as they stand now (in place: the twin's handle keeps its pointers)
    for n in P.AGENT_STATE:
        getattr(twin.agent, n).copy_(getattr(used.agent, n))
    slots = np.ascontiguousarray(two.leaves[1].cpu().numpy(), np.int32)  # explicit slots: valid elements of the ring
    _plain_step(used, family, ring, slots, B)
    _plain_step(twin, family, ring, slots, B)
    torch.cuda.synchronize()
    for n in P.AGENT_STATE:
        a, b = getattr(used.agent, n).cpu().numpy(), getattr(twin.agent, n).cpu().numpy()
        assert a.tobytes() == b.tobytes(), (family, B, n)
    assert (used.agent._count.cpu().numpy() == 4).all() and np.isfinite(used.agent._losses.cpu().numpy()).all()
    rows_after = {k: v for r, tag in ((one, "1"), (two, "2")) for k, v in ((tag + n, t) for n, t in r.all().items())}
    for k, v in rows_before.items():  # weights and |TD| of the earlier calls: not read into, not written by, the plain step
        assert v.cpu().numpy().tobytes() == rows_after[k].cpu().numpy().tobytes(), (family, B, k)
