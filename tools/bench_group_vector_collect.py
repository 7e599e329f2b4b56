"""What one vector step of S seeds x E time lines costs as one ``GroupVectorCollector.add_many`` call (``replay_group_add_many``,
csrc/replay_group_kernels.h) against S ``rb.add_many`` calls (``replay_add_step`` each), each leg followed by the S
``sample_slots()`` + ``ring_view()`` that a learner step makes:

  collect  LunarLander-shaped frames (8 float32, stack 1), S = 1, 2, 4, 8, 16 at E = 2 and E = 8; one line for 84 x 84 uint8 frames,
           stack 4, at S = 8, E = 8
  trainer  ``SeedVectorTrainer`` on S = 4 and 16 seeds of E = 8 environments (summed env-steps/s) against S ``VectorTrainer`` runs
           one after the other; the harness of tools/bench_seed_group.py

Both legs of a pair run on twin buffers in one process; regions of ``--calls`` vector steps alternate between the legs ``--rounds``
times, each timed on the host clock with a device synchronisation at both ends; per leg the median and [min, max] of the regions,
microseconds per vector step.  ``group_is_default`` is the project's rule: the group's median lies below the solo chain's minimum.
Writes ``profiles/group_vector_collect.json``.
Usage: ``python tools/bench_group_vector_collect.py [--calls 200] [--rounds 7] [--no-trainer] [--out profiles/group_vector_collect.json]``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd"), os.path.join(ROOT, "tools")]
SIZES, ENVS, B = (1, 2, 4, 8, 16), (2, 8), 32


def collect_at(S, E, shape, dtype, stack, calls, rounds):
    import numpy as np

    from bench_seed_group import pair
    from slimdqn.sample_collection.group_replay import GroupVectorCollector
    from slimdqn.sample_collection.replay_buffer import TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    mk = lambda: [VectorReplayBuffer(UniformSamplingDistribution(g), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1,
                                     gamma=0.99, n_envs=E) for g in range(S)]
    solo, group = mk(), mk()
    col = GroupVectorCollector(group, force=True)
    rng = np.random.default_rng(0)
    pool = [(rng.integers(0, 256, shape, dtype=np.uint8) if np.dtype(dtype) == np.uint8 else rng.standard_normal(shape).astype(dtype))
            for _ in range(64)]
    n = {"solo": 0, "group": 0}

    def rows(leg):  # the S x E transitions of one vector step: episodes of 200 steps, as the trainer harness
        n[leg] += 1
        last = n[leg] % 200 == 0
        return [[TransitionElement(pool[(n[leg] + g + 7 * e) % 64], (n[leg] + g + e) % 4, 0.5, last, last) for e in range(E)] for g in range(S)]

    def learner_side(rbs):
        for rb in rbs:
            rb.sample_slots()
            rb.ring_view()

    def solo_fn():
        for rb, row in zip(solo, rows("solo")):
            rb.add_many(row)
        learner_side(solo)

    def group_fn():
        col.add_many(rows("group"))
        learner_side(group)

    for _ in range(2):  # (the first transition of an episode makes no element: nothing to sample yet)
        for rb, row in zip(solo, rows("solo")):
            rb.add_many(row)
        col.add_many(rows("group"))
    out = pair(group_fn, solo_fn, calls, rounds)
    assert col.group_calls == (rounds + 1) * calls + 2, col.group_calls
    return out


def trainer_at(S, E, warmup, steps, reps):
    import torch

    from bench_seed_group import summary
    from experiments.base.dqn import VectorTrainer
    from experiments.base.seeds import SeedVectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    def triple(seed):
        p = dict(seed=seed, epsilon_end=0.01, epsilon_duration=1000, n_epochs=1, n_training_steps_per_epoch=warmup + steps,
                 n_initial_samples=1000, horizon=1000, wandb=NullLogger())
        rb = VectorReplayBuffer(UniformSamplingDistribution(seed), batch_size=B, max_capacity=10_000, stack_size=1, update_horizon=1, gamma=0.99,
                                n_envs=E)
        rb.reuse_sample_buffers = True
        envs = [SyntheticVector(1000 * e + seed, episode_length=200) for e in range(E)]
        return p, iDQN(seed, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 200, 10), envs, rb

    rates = {"seed_vector_trainer": [], "sequential_vector_trainers": []}
    for _ in range(reps):
        for leg in rates:
            ts = [triple(s) for s in range(S)]
            keys = [prng.PRNGKey(s) for s in range(S)]
            if leg == "seed_vector_trainer":
                trainer = SeedVectorTrainer(keys, [t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts], [t[3] for t in ts])
                runs = [trainer.run]
                counts = lambda: sum(s.total_steps for s in trainer.seeds)
            else:
                trainers = [VectorTrainer(k, *t) for k, t in zip(keys, ts)]
                runs = [t.run for t in trainers]
                counts = lambda: sum(t.total_steps for t in trainers)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for run in runs:
                run()
            torch.cuda.synchronize()
            rates[leg].append(counts() / (time.perf_counter() - t0))
    a, b = summary(rates["seed_vector_trainer"]), summary(rates["sequential_vector_trainers"])
    return {"seed_vector_trainer": a, "sequential_vector_trainers": b, "group_over_sequential": a["median"] / b["median"],
            "note": "summed env-steps/s over the whole run (the first 1000 steps without gradient steps included), the collector and "
                    "the group calls at their defaults"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--no-collect", action="store_true", help="keep the collection figures of --out, measure the trainer only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_vector_collect.json"))
    a = ap.parse_args()
    import numpy as np

    res = {"method": {"calls": a.calls, "rounds": a.rounds, "frames": "8 float32, stack 1", "unit": "us per vector step of S x E adds + S "
                      "sample_slots/ring_view"}, "E": {}}
    if a.no_collect:
        with open(a.out) as f:
            res = json.load(f)
    for E in () if a.no_collect else ENVS:
        res["E"][str(E)] = {}
        for S in SIZES:
            res["E"][str(E)][str(S)] = collect_at(S, E, (8,), np.float32, 1, a.calls, a.rounds)
            print("RESULT" + json.dumps({"E": E, "S": S, **res["E"][str(E)][str(S)]}), flush=True)
    if not a.no_collect:
        res["atari_84x84_uint8_stack4_S8_E8"] = collect_at(8, 8, (84, 84), np.uint8, 4, a.calls, a.rounds)
        print("RESULT" + json.dumps({"atari_S": 8, "E": 8, **res["atari_84x84_uint8_stack4_S8_E8"]}), flush=True)
        # a size is a default where the rule holds at every E measured
        res["group_default_sizes"] = [S for S in SIZES if all(res["E"][str(E)][str(S)]["group_is_default"] for E in ENVS)]
    if not a.no_trainer:
        res["trainer_env_steps_per_s"] = {}
        for S in (4, 16):
            res["trainer_env_steps_per_s"][str(S)] = trainer_at(S, 8, a.warmup, a.steps, a.reps)
            print("RESULT" + json.dumps({"trainer_S": S, "E": 8, **res["trainer_env_steps_per_s"][str(S)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
