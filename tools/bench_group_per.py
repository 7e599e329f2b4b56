"""What the prioritized step of a seed group costs as one call (``idqn_group_per_learn_on_replay_fc``: k_per_group_draw, the group
step, k_per_group_write_back -- csrc/per_group_kernels.h, csrc/per_phases.h) against its members stepped one after the other, on the LunarLander
net (fc, obs 8, [100, 100], A = 4, K = 3, B = 32) at S = 1, 2, 4, 8, 16, 32 members:

  group   one ``PrioritizedGroupLearner.step()`` through the group call (S host draws, one C call, three launches)
  solo    S ``PrioritizedLearner.step()`` calls (S host draws, S ``idqn_per_learn_on_replay`` calls, three launches each)

Both legs run on the SAME handles, trees and rings in one process; regions of ``--calls`` steps alternate between the legs
``--rounds`` times after a warm-up region each, timed on the host clock with a device synchronisation at both ends; per leg
the median and [min, max] of the regions, microseconds per prioritized step of all S members.  ``group_is_default`` is the
project's rule: the group's median lies below the solo leg's minimum; ``group_per_sizes`` collects those S.  One run on one
box.  Writes ``profiles/group_per.json`` (keeps a ``parent_comparison`` entry that is already there).
Usage: ``python tools/bench_group_per.py [--calls 200] [--rounds 7] [--out profiles/group_per.json]``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
SIZES, B = (1, 2, 4, 8, 16, 32), 32


def summary(v):
    s = sorted(v)
    return {"median": s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), "min": s[0], "max": s[-1], "n": len(s)}


def group_learner(S):
    import numpy as np

    from slimdqn.networks.group import AgentGroup
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.per import PrioritizedGroupLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement

    agents, rbs = [], []
    for g in range(S):
        rb = ReplayBuffer(SlotPrioritizedSampler(g, 2000), batch_size=B, max_capacity=2000, stack_size=1, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(g)
        for i in range(2500):
            rb.add(TransitionElement(rng.standard_normal(8).astype(np.float32), int(rng.integers(4)), float(rng.normal()), i % 200 == 199,
                                     i % 200 == 199))
        rb.reuse_sample_buffers = True
        agents.append(iDQN(g, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 10**9, 10**9))
        rbs.append(rb)
    group = AgentGroup(agents)
    group.group_sizes = frozenset(range(1, 33))  # the route itself at every size, whatever the defaults
    gl = PrioritizedGroupLearner(group, rbs, beta=0.4, eps=1e-3, reduce="mean")
    gl.group_per_sizes = frozenset(range(1, 33))
    return gl


def at(S, calls, rounds):
    import torch

    gl = group_learner(S)

    def solo():
        for lr in gl.learners:
            lr.step()

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    region(gl.step), region(solo)  # warm-up: allocations
    assert gl.__dict__.get("_group_per_ok") is True, "the group call did not run"
    assert all(lr.__dict__.get("_fused_ok") is True for lr in gl.learners), "the members' one-call step did not run"
    reg = {"group": [], "solo": []}
    for _ in range(rounds):
        reg["group"].append(region(gl.step))
        reg["solo"].append(region(solo))
    gl.group.close()
    g, s = summary(reg["group"]), summary(reg["solo"])
    return {"group": g, "solo": s, "solo_over_group": s["median"] / g["median"], "group_is_default": g["median"] < s["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_per.json"))
    a = ap.parse_args()
    res = {"method": {"calls": a.calls, "rounds": a.rounds, "batch": B, "net": "fc obs 8 [100, 100] A 4 K 3", "capacity": 2000,
                      "unit": "us per prioritized step of all S members", "note": "one run on one box"}, "S": {}}
    for S in SIZES:
        res["S"][str(S)] = at(S, a.calls, a.rounds)
        print("RESULT" + json.dumps({"S": S, **res["S"][str(S)]}), flush=True)
    res["group_per_sizes"] = [int(S) for S, r in res["S"].items() if r["group_is_default"]]
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "parent_comparison" in old:
            res["parent_comparison"] = old["parent_comparison"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
