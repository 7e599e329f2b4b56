"""Grad-steps/s of DataParallelLearner.update_online_params (slimdqn/networks/parallel.py) at W = 1 on RCCL, against the bare
data-parallel step on a pre-gathered shard and against the single-device loop -- uniform and prioritized, B = 32 and 256.

    python tools/bench_dp_learner.py [--steps 200] [--warmup 30] [--heads 5] [--out profiles/dp_learner_w1.json]

Prints ONE JSON line.  Per (sampler, B):
  learner     DataParallelLearner.update_online_params (idqn_dp_learn_on_replay: the draw, the shard staged from the frame
              ring inside the step, the collectives of the factored schedule; prioritized: + weights, |TD| gather, priorities,
              tree write-back)
  bare_dp     idqn_dp_step (data_parallel_step, native mode) on a shard gathered once before the timed region
  single      the single-device loop: iDQN.update_online_params (uniform) / PrioritizedLearner.step (prioritized)
and the ratios learner / bare_dp and learner / single.  Each leg is timed over `steps` calls after `warmup`, the clock read
after a device synchronisation at both ends (host-side issue included, as a trainer sees it).
"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "i-dqn_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

OBS, A, FEATS = (84, 84, 4), 18, [32, 64, 64, 512]


def rate(fn, steps, warmup):
    import torch

    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(warmup + i)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def make(kind, B, K, n=2000):
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.per import SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    cap = 1500
    sampler = UniformSamplingDistribution(1) if kind == "uniform" else SlotPrioritizedSampler(1, cap, 0.6)
    rb = ReplayBuffer(sampler, batch_size=B, max_capacity=cap, stack_size=4, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(0)
    for i in range(n):
        rb.add(TransitionElement(rng.integers(0, 256, OBS[:2], dtype=np.uint8), int(rng.integers(A)), float(rng.normal()),
                                 bool(i % 97 == 96), False), **({"priority": float(rng.random() + 0.1)} if kind != "uniform" else {}))
    rb.reuse_sample_buffers = True
    agent = iDQN(0, OBS, A, K, FEATS, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
    return rb, agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--heads", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    import torch.distributed as dist

    from slimdqn.networks.parallel import DataParallelLearner, data_parallel_step
    from slimdqn.sample_collection.per import PrioritizedLearner

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    K, rows = args.heads, []
    try:
        for kind in ("uniform", "prioritized"):
            for B in (32, 256):
                rb, agent = make(kind, B, K)
                learner = DataParallelLearner(agent, rb)
                r_learner = rate(lambda i: learner.update_online_params(i), args.steps, args.warmup)
                assert agent.__dict__.get("_dp") is not None, "the native step did not run"
                rb2, agent2 = make(kind, B, K)
                shard = rb2._gather(rb2.sample_slots(B))
                r_bare = rate(lambda i: data_parallel_step(agent2, shard, B, mode="native"), args.steps, args.warmup)
                rb3, agent3 = make(kind, B, K)
                if kind == "uniform":
                    r_single = rate(lambda i: agent3.update_online_params(i, rb3), args.steps, args.warmup)
                else:
                    pl = PrioritizedLearner(agent3, rb3)
                    r_single = rate(lambda i: pl.step(), args.steps, args.warmup)
                rows.append({"sampler": kind, "B": B, "K": K, "learner_steps_per_s": round(r_learner, 1),
                             "bare_dp_step_steps_per_s": round(r_bare, 1), "single_device_steps_per_s": round(r_single, 1),
                             "learner_over_bare_dp": round(r_learner / r_bare, 4), "learner_over_single": round(r_learner / r_single, 4)})
                del learner, agent, agent2, agent3
                torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    out = {"metric": "dp_learner_grad_steps_per_s", "world": 1, "backend": "nccl (RCCL)", "A": A, "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "rows": rows,
           "target": "learner_over_bare_dp >= 0.97 with the uniform sampler"}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
