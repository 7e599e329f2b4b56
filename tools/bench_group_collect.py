"""What the S replay adds of a lock-step iteration cost as one ``GroupCollector.add_many`` call (``replay_group_add_step``,
csrc/replay_group_kernels.h) against S ``rb.add`` calls, each leg followed by the S ``sample_slots()`` + ``ring_view()`` that a
learner step makes (the solo leg's element rows travel there: ``_flush_meta``):

  collect  LunarLander-shaped frames (8 float32), S = 1, 2, 4, 8, 16, 32; one line for 84 x 84 uint8 frames at S = 8
  trainer  ``SeedTrainer`` on S = 4 and 16 seeds (summed env-steps/s), collector forced on against forced off -- forced off is
           the parent's sequence of device calls (every buffer's own ``add``); the harness of tools/bench_seed_group.py

Both legs of a pair run on twin buffers in one process; regions of ``--calls`` collections alternate between the legs
``--rounds`` times, each timed on the host clock with a device synchronisation at both ends; per leg the median and [min, max]
of the regions, microseconds per lock-step collection.  ``group_is_default`` is the project's rule: the group's median lies
below the solo chain's minimum.  Writes ``profiles/group_collect.json``.
Usage: ``python tools/bench_group_collect.py [--calls 200] [--rounds 7] [--no-trainer] [--out profiles/group_collect.json]``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd"), os.path.join(ROOT, "tools")]
SIZES, B = (1, 2, 4, 8, 16, 32), 32


def collect_at(S, shape, dtype, stack, calls, rounds):
    import numpy as np

    from bench_seed_group import pair
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    mk = lambda: [ReplayBuffer(UniformSamplingDistribution(g), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1, gamma=0.99)
                  for g in range(S)]
    solo, group = mk(), mk()
    col = GroupCollector(group, force=True)
    rng = np.random.default_rng(0)
    pool = [(rng.integers(0, 256, shape, dtype=np.uint8) if np.dtype(dtype) == np.uint8 else rng.standard_normal(shape).astype(dtype))
            for _ in range(64)]
    n = {"solo": 0, "group": 0}

    def row(leg):  # the S transitions of one iteration: episodes of 200 steps, as the trainer harness
        n[leg] += 1
        last = n[leg] % 200 == 0
        return [TransitionElement(pool[(n[leg] + g) % 64], (n[leg] + g) % 4, 0.5, last, last) for g in range(S)]

    def learner_side(rbs):
        for rb in rbs:
            rb.sample_slots()
            rb.ring_view()

    def solo_fn():
        for rb, tr in zip(solo, row("solo")):
            rb.add(tr)
        learner_side(solo)

    def group_fn():
        col.add_many(row("group"))
        learner_side(group)

    for _ in range(2):  # (the first transition of an episode makes no element: nothing to sample yet)
        for rb, tr in zip(solo, row("solo")):
            rb.add(tr)
        col.add_many(row("group"))
    out = pair(group_fn, solo_fn, calls, rounds)
    assert col.group_calls == (rounds + 1) * calls + 2, col.group_calls
    return out


def trainer_at(S, warmup, steps, reps):
    import torch

    from experiments.base.seeds import SeedTrainer
    from experiments.base.utils import NullLogger
    from bench_seed_group import summary
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.group_replay import GroupCollector
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    def triple(seed):
        p = dict(seed=seed, epsilon_end=0.01, epsilon_duration=1000, n_epochs=1, n_training_steps_per_epoch=warmup + steps,
                 n_initial_samples=1000, horizon=1000, wandb=NullLogger())
        rb = ReplayBuffer(UniformSamplingDistribution(seed), batch_size=B, max_capacity=10_000, stack_size=1, update_horizon=1, gamma=0.99)
        rb.reuse_sample_buffers = True
        return p, iDQN(seed, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 200, 10), SyntheticVector(seed, episode_length=200), rb

    rates = {"collector_on": [], "collector_off": []}
    total = S * (warmup + steps)
    for _ in range(reps):
        for leg, force in (("collector_on", True), ("collector_off", False)):
            ts = [triple(s) for s in range(S)]
            rbs = [t[3] for t in ts]
            st = SeedTrainer([prng.PRNGKey(s) for s in range(S)], [t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts], rbs,
                             collector=GroupCollector(rbs, force=force))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.run()
            torch.cuda.synchronize()
            rates[leg].append(total / (time.perf_counter() - t0))
    a, b = summary(rates["collector_on"]), summary(rates["collector_off"])
    return {"collector_on": a, "collector_off": b, "on_over_off": a["median"] / b["median"],
            "note": "summed env-steps/s over the whole run, the first 1000 steps without gradient steps included; collector_off makes the "
                    "parent commit's device calls (every buffer's own add)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_collect.json"))
    a = ap.parse_args()
    import numpy as np

    res = {"method": {"calls": a.calls, "rounds": a.rounds, "frames": "8 float32, stack 1", "unit": "us per lock-step collection of S adds + S "
                      "sample_slots/ring_view"}, "S": {}}
    for S in SIZES:
        res["S"][str(S)] = collect_at(S, (8,), np.float32, 1, a.calls, a.rounds)
        print("RESULT" + json.dumps({"S": S, **res["S"][str(S)]}), flush=True)
    res["atari_84x84_uint8_stack4_S8"] = collect_at(8, (84, 84), np.uint8, 4, a.calls, a.rounds)
    print("RESULT" + json.dumps({"atari_S": 8, **res["atari_84x84_uint8_stack4_S8"]}), flush=True)
    res["group_default_sizes"] = [int(S) for S, r in res["S"].items() if r["group_is_default"]]
    if not a.no_trainer:
        res["trainer_env_steps_per_s"] = {}
        for S in (4, 16):
            res["trainer_env_steps_per_s"][str(S)] = trainer_at(S, a.warmup, a.steps, a.reps)
            print("RESULT" + json.dumps({"trainer_S": S, **res["trainer_env_steps_per_s"][str(S)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
