"""Vector-environment collection against the single-environment loop, on one box, in one process.

Writes ``profiles/vector_collect.json`` (``--out`` to redirect):

* ``loop``: the Atari-shaped synthetic training loop in environment steps / s -- the existing ``Trainer`` on ``ReplayBuffer``
  (one environment, set up the way ``experiments/base/launch.py`` sets it up: lazy host actions, postponed replay add) and
  ``VectorTrainer`` on ``VectorReplayBuffer`` at E = 1 / 2 / 8 / 32;
* ``collect``: collection only (no acting, no gradient steps), microseconds per vector step of ``add_many`` against E calls of
  ``ReplayBuffer.add`` on the same frames, the stream synchronised at the end of the timed region.

Every leg is repeated ``--reps`` times, the legs interleaved (rep 0 of every leg, then rep 1, ...) so that drift hits all alike;
per leg the file holds every repetition, the median and the spread (min, max).  ``faster`` is stated only where the two legs'
spreads do not overlap.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "i-dqn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

OBS, ACTIONS, FEATURES, HEADS, BATCH = (84, 84, 4), 6, [32, 64, 64, 512], 5, 32
ENVS = (1, 2, 8, 32)


def _params(steps):
    from experiments.base.utils import NullLogger

    return dict(epsilon_end=0.01, epsilon_duration=1000, n_epochs=2, n_training_steps_per_epoch=steps, n_initial_samples=1000,
                horizon=27000, wandb=NullLogger())


def _agent():
    from slimdqn.networks.idqn import iDQN

    return iDQN(0, OBS, ACTIONS, HEADS, FEATURES, "cnn", 6.25e-5, 0.99, 1, 4, 2000, 30, adam_eps=1.5e-4)


def _buffer(n_envs, capacity):
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    kw = dict(batch_size=BATCH, max_capacity=capacity, stack_size=4, update_horizon=1, gamma=0.99, clipping=lambda r: np.clip(r, -1, 1))
    rb = ReplayBuffer(UniformSamplingDistribution(0), **kw) if n_envs is None else VectorReplayBuffer(UniformSamplingDistribution(0), n_envs=n_envs, **kw)
    rb.reuse_sample_buffers = True
    return rb


def loop_leg(n_envs, warmup, steps, capacity):
    """Environment steps / s of one epoch of ``steps`` steps, after a warm-up epoch that passes ``n_initial_samples``."""
    import torch

    from experiments.base.dqn import Trainer, VectorTrainer
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticAtari

    p, agent, rb = _params(warmup), _agent(), _buffer(n_envs, capacity)
    if n_envs is None:
        agent.lazy_host_actions, p["overlap_replay_add"] = True, True
        env = SyntheticAtari(0, episode_length=200)
        trainer = Trainer(prng.PRNGKey(0), p, agent, env, rb)
        env.reset()
    else:
        envs = [SyntheticAtari(e, episode_length=200) for e in range(n_envs)]
        trainer = VectorTrainer(prng.PRNGKey(0), p, agent, envs, rb)
        for env in envs:
            env.reset()
    trainer.run_epoch(0)
    torch.cuda.synchronize()
    p["n_training_steps_per_epoch"] = steps
    before, t0 = trainer.total_steps, time.perf_counter()
    trainer.run_epoch(1)
    torch.cuda.synchronize()
    return (trainer.total_steps - before) / (time.perf_counter() - t0)


def collect_leg(n_envs, vector, vector_steps, capacity):
    """Microseconds per vector step: E frames into the buffer, by one ``add_many`` or by E ``add`` calls."""
    import torch

    from slimdqn.sample_collection.replay_buffer import TransitionElement

    rng = np.random.default_rng(0)
    pool = rng.integers(0, 256, (64, 84, 84), dtype=np.uint8)
    rb = _buffer(n_envs if vector else None, capacity)

    def step(i):
        trs = [TransitionElement(pool[(i + e) % 64], (i + e) % ACTIONS, 1.0, False, (i % 200) == 199) for e in range(n_envs)]
        if vector:
            rb.add_many(trs)
        else:
            for tr in trs:
                rb.add(tr)

    for i in range(50):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(50, 50 + vector_steps):
        step(i)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / vector_steps


def _summary(values):
    return {"reps": [round(v, 2) for v in values], "median": round(float(np.median(values)), 2), "min": round(min(values), 2),
            "max": round(max(values), 2)}


def _faster(a, b, higher_is_better):
    """``a`` against ``b``: "a", "b" or None when the spreads overlap."""
    if higher_is_better:
        return "a" if a["min"] > b["max"] else "b" if b["min"] > a["max"] else None
    return "a" if a["max"] < b["min"] else "b" if b["max"] < a["min"] else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_collect.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--capacity", type=int, default=50000)
    ap.add_argument("--collect-steps", type=int, default=300)
    args = ap.parse_args()
    import torch

    loop = {"trainer": []}
    loop.update({f"vector_E{e}": [] for e in ENVS})
    collect = {f"{kind}_E{e}": [] for e in ENVS for kind in ("add_many", "add")}
    for rep in range(args.reps):
        loop["trainer"].append(loop_leg(None, args.warmup, args.steps, args.capacity))
        for e in ENVS:
            loop[f"vector_E{e}"].append(loop_leg(e, args.warmup, args.steps, args.capacity))
        for e in ENVS:
            collect[f"add_many_E{e}"].append(collect_leg(e, True, args.collect_steps, args.capacity))
            collect[f"add_E{e}"].append(collect_leg(e, False, args.collect_steps, args.capacity))
        print(f"[bench_vector_collect] rep {rep}: " + ", ".join(f"{k} {v[-1]:.0f}" for k, v in loop.items()), flush=True)
    loop = {k: _summary(v) for k, v in loop.items()}
    collect = {k: _summary(v) for k, v in collect.items()}
    result = {
        "device": torch.cuda.get_device_name(0), "config": {"obs": OBS, "heads": HEADS, "features": FEATURES, "batch": BATCH, "update_to_data": 4,
                                                           "steps": args.steps, "warmup": args.warmup, "capacity": args.capacity, "reps": args.reps},
        "loop_env_steps_per_s": loop,
        "loop_vs_trainer": {k: {"ratio_of_medians": round(v["median"] / loop["trainer"]["median"], 3),
                                "faster": {"a": k, "b": "trainer", None: None}[_faster(v, loop["trainer"], True)]}
                            for k, v in loop.items() if k != "trainer"},
        "collect_us_per_vector_step": collect,
        "collect_add_many_vs_add": {f"E{e}": {"ratio_of_medians": round(collect[f"add_E{e}"]["median"] / collect[f"add_many_E{e}"]["median"], 3),
                                             "faster": {"a": "add_many", "b": "add", None: None}[_faster(collect[f"add_many_E{e}"], collect[f"add_E{e}"], False)]}
                                    for e in ENVS},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
