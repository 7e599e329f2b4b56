"""i-IQN learner loops with and without the replay-sourced step and prioritized replay: BASELINE config 3 (K = 5, N = 32,
A = 6, [32, 64, 64, 512], Atari-shaped uint8 frames) at B = 32 and 256.

ms per step of five loops, timed in interleaved regions (every loop sees the same clocks), median region reported:
  (a) ``bare``                      ``iIQN._learn`` on a device-resident batch (what ``bench.py --algo iiqn`` times)
  (b) ``uniform_two_calls``         ``update_online_params``: sample, ``replay_gather_stacked``, ``idqn_iqn_learn_on_batch``
  (c) ``uniform_fused``             ``update_online_params``: ``idqn_iqn_learn_on_replay`` on the frame ring
  (d) ``prioritized_gathered``      ``PrioritizedLearner.step()``: leaves, weights, gather, weighted step, priorities, tree update
  (e) ``prioritized_replay_sourced`` the same with the leaves handed to ``idqn_iqn_learn_on_replay_dev`` (no gather)
(b) is the comparison for (c), (d) for (e).

Every batch size runs in a fresh child process under its own ``timeout``; the driver itself never opens the GPU and stops at
the first child that fails.  One JSON line per batch size.
Usage: ``python tools/bench_iiqn_per.py [--batches 32 256] [--steps 20] [--warmup 10] [--regions 7] [--limit 240] [--out FILE]``.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "i-dqn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def run(B, steps, warmup, regions, A=6, N=32):
    import torch

    from bench import FEATURES, K_HEADS, OBS, synthetic
    from slimdqn.networks.iiqn import iIQN
    from slimdqn.sample_collection.per import PrioritizedLearner, SlotPrioritizedSampler
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    agent = iIQN(0, OBS, A, K_HEADS, FEATURES, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
    batches = [Batch(*(torch.from_numpy(x).cuda() for x in synthetic(1000 + i, A, B))) for i in range(8)]
    rng = np.random.default_rng(0)
    n_el = 4096
    frames = rng.integers(0, 256, size=(512, 84, 84), dtype=np.uint8)

    def fill(rb):
        for i in range(n_el + 4):
            rb.add(TransitionElement(frames[i % 512], int(rng.integers(A)), float(rng.integers(-1, 2)), bool(i % 1000 == 999), False))
        rb.reuse_sample_buffers = True
        return rb

    rb_u = fill(ReplayBuffer(UniformSamplingDistribution(1), batch_size=B, max_capacity=n_el, stack_size=4, update_horizon=1, gamma=0.99))
    rb_p = fill(ReplayBuffer(SlotPrioritizedSampler(3, n_el, priority_exponent=0.6), batch_size=B, max_capacity=n_el, stack_size=4,
                             update_horizon=1, gamma=0.99))
    learner = PrioritizedLearner(agent, rb_p, beta=0.4, eps=1e-3, reduce="mean")
    it = [0]

    def bare():
        agent._learn(batches[it[0] % 8])
        it[0] += 1

    def unfused(fn):  # the two-call / gathered form of a loop: the agent's own switch, as bench.py's sampling legs use it
        def wrapped():
            agent.fuse_replay_sampling = False
            fn()
            agent.fuse_replay_sampling = True
        return wrapped

    legs = {"bare": bare, "uniform_two_calls": unfused(lambda: agent.update_online_params(0, rb_u)),
            "uniform_fused": lambda: agent.update_online_params(0, rb_u),
            "prioritized_gathered": unfused(learner.step), "prioritized_replay_sourced": learner.step}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    assert agent.__dict__.get("_replay_fused_ok") is True, "the replay-sourced step did not run"
    times = {n: [] for n in legs}
    for _ in range(regions):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    losses = agent._losses.cpu().numpy()
    assert np.isfinite(losses).all(), losses
    ms = {n: float(np.median(t)) for n, t in times.items()}
    return {"batch": B, "heads": K_HEADS, "quantiles": N, "actions": A, "features": FEATURES, "steps_per_region": steps,
            "regions": regions, "reported": "median region, ms per step", "ms_per_step": ms, "ms_per_step_all": times,
            "fused_over_two_calls": ms["uniform_fused"] / ms["uniform_two_calls"],
            "replay_sourced_over_gathered": ms["prioritized_replay_sourced"] / ms["prioritized_gathered"],
            "final_losses": [float(x) for x in losses]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[32, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one batch size's process, seconds")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:  # one batch size, in this process
        print(json.dumps(run(args.child, args.steps, args.warmup, args.regions)), flush=True)
        return 0
    for B in args.batches:  # a fresh process per batch size, each under its own time limit; nothing follows a failure
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(B),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--regions", str(args.regions)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            print(f"[bench_iiqn_per] B = {B}: exit status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
