"""What n prioritized steps of a seed group cost as one call (``idqn_group_per_learn_steps_on_replay_fc``: one upload,
k_per_group_draw, then the group step / k_per_group_turn alternating, k_per_group_write_back -- csrc/per_group_kernels.h) against
the two chains a user has without it, on the LunarLander net (fc, obs 8, [100, 100], A = 4, K = 3, B = 32) at S = 1, 2, 4, 8,
16, 32 members and n = 1, 2, 5, 8, 32 steps per call:

  steps   ``PrioritizedGroupLearner.steps(n)`` through the n-step group call (S x n host draws, one C call, 2 n + 1 launches)
  chain   n ``PrioritizedGroupLearner.step()`` calls (n ``idqn_group_per_learn_on_replay_fc`` calls, 3 n launches, n uploads)
  solo    S ``PrioritizedLearner.steps(n)`` calls (S ``idqn_per_learn_steps_on_replay`` calls, S (2 n + 1) launches)

All legs run on the SAME handles, trees and rings in one process; regions of about ``--steps`` gradient steps alternate between
the legs ``--rounds`` times after a warm-up region each, timed on the host clock with a device synchronisation at both ends; per
leg the median and [min, max] of the regions, microseconds per gradient step of all S members.  ``steps_is_default`` is the
project's rule: the call's median lies below the minimum of the chain of n single group calls; ``group_per_steps_sizes`` /
``group_per_steps_min`` are the S at which that holds for every measured n from the smallest such n on, and that n.  One run on
one box.  Writes ``profiles/group_per_steps.json`` (keeps ``trainer`` and ``headline`` entries that are already there).
Usage: ``python tools/bench_group_per_steps.py [--steps 192] [--rounds 7] [--out profiles/group_per_steps.json]``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
SIZES, STEPS, B, CAPACITY = (1, 2, 4, 8, 16, 32), (1, 2, 5, 8, 32), 32, 1024


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
        rb = ReplayBuffer(SlotPrioritizedSampler(g, CAPACITY), batch_size=B, max_capacity=CAPACITY, stack_size=1, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(g)
        for i in range(CAPACITY + 200):
            rb.add(TransitionElement(rng.standard_normal(8).astype(np.float32), int(rng.integers(4)), float(rng.normal()), i % 200 == 199,
                                     i % 200 == 199))
        rb.reuse_sample_buffers = True
        agents.append(iDQN(g, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 10**9, 10**9))
        rbs.append(rb)
    group = AgentGroup(agents)
    group.group_sizes = frozenset(range(1, 33))  # the routes themselves at every size, whatever the defaults
    gl = PrioritizedGroupLearner(group, rbs, beta=0.4, eps=1e-3, reduce="mean")
    gl.group_per_sizes = gl.group_per_steps_sizes = frozenset(range(1, 33))
    gl.group_per_steps_min = 1
    for lr in gl.learners:
        lr.per_steps_min = 1
    return gl


def at(gl, n, steps, rounds):
    import torch

    reps = max(1, steps // n)

    def call():
        gl.steps(n)

    def chain():
        for _ in range(n):
            gl.step()

    def solo():
        for lr in gl.learners:
            lr.steps(n)

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / (reps * n)

    legs = {"steps": call, "chain": chain, "solo": solo}
    for fn in legs.values():  # warm-up: allocations, first launches
        region(fn)
    assert gl.__dict__.get("_group_per_steps_ok") is True, "the n-step group call did not run"
    assert gl.__dict__.get("_group_per_ok") is True, "the single group call did not run"
    assert all(lr.__dict__.get("_steps_ok") is True for lr in gl.learners), "the members' n-step call did not run"
    reg = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            reg[k].append(region(fn))
    out = {k: summary(v) for k, v in reg.items()}
    out["chain_over_steps"] = out["chain"]["median"] / out["steps"]["median"]
    out["solo_over_steps"] = out["solo"]["median"] / out["steps"]["median"]
    out["steps_is_default"] = out["steps"]["median"] < out["chain"]["min"]
    out["steps_below_solo"] = out["steps"]["median"] < out["solo"]["min"]
    return out


def defaults(res):
    """(sizes, minimum n): the smallest measured n from which on the call is the default at some S, and the S where it is the
    default at every measured n >= that n."""
    for n_min in STEPS:
        sizes = [S for S in SIZES if S >= 2 and all(res[str(S)][str(n)]["steps_is_default"] for n in STEPS if n >= n_min)]
        if sizes:
            return sizes, n_min
    return [], STEPS[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=192)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_per_steps.json"))
    a = ap.parse_args()
    res = {"method": {"steps_per_region": a.steps, "rounds": a.rounds, "batch": B, "net": "fc obs 8 [100, 100] A 4 K 3", "capacity": CAPACITY,
                      "unit": "us per gradient step of all S members", "note": "one run on one box"}, "S": {}}
    for S in SIZES:
        gl = group_learner(S)
        res["S"][str(S)] = {}
        for n in STEPS:
            res["S"][str(S)][str(n)] = at(gl, n, a.steps, a.rounds)
            print("RESULT" + json.dumps({"S": S, "n": n, **res["S"][str(S)][str(n)]}), flush=True)
        gl.group.close()
    sizes, n_min = defaults(res["S"])
    res["group_per_steps_sizes"], res["group_per_steps_min"] = sizes, n_min
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        for keep in ("trainer", "headline"):
            if keep in old:
                res[keep] = old[keep]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
