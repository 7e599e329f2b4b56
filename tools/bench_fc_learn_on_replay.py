"""What ``update_online_params`` costs on MLP and general-shape cnn agents with the replay-sourced step
(``idqn_learn_on_replay_fc``: one C call, csrc/replay_src_kernels.h) against ``fuse_replay_sampling = False`` (``sample()`` =
two gather launches, then ``idqn_learn_on_batch``) on the same commit, and what the LunarLander-shaped training loops make of it
against the parent commit.

  lunar       fc, obs 8, [100, 100], A = 4, K = 3, B = 32 (the LunarLander experiment)   k_fc_step_par reads the ring itself
  fc_520      fc, obs 8, [520], A = 4, K = 3, B = 32                                     staging launch + k_fc_step_mfma / _lds
  gcnn_smoke  cnn, (84, 84, 4), [2, 3, 1, 15], A = 6, K = 1, B = 32                      staging launch + the general-shape step

``--leg update:<config>[:staged]`` (one process): two agents and two buffers of the same seeds, one per side; regions of
``--calls`` ``update_online_params`` calls alternate between the sides, ``--rounds`` times, each region timed on the host clock
with a device synchronisation at both ends (the loop is what a trainer pays: host work and GPU work overlap as they do there).
``:staged`` sets ``IDQN_FC_REPLAY_STAGE=1`` before the library loads: the one-launch batches go through the staging launch too
(the A/B of the in-kernel gather).  ``--leg trainer:<trainer|1|8|32>`` runs one leg of the synthetic LunarLander-shaped loop
(``tools/bench_fc_act_many.py``'s: a gradient step per environment step) and ``--tree DIR`` takes package, experiments and
library from another checkout (the parent commit, built by its own ``build()``).

Without ``--leg`` this is the driver: every leg in a fresh process under its own time limit, ``--reps`` repetitions of each,
trees alternating, nothing started after a failure; per measurement the median and [min, max]; ``faster`` names a side only
where the intervals do not overlap.  Writes ``profiles/fc_learn_on_replay.json``.
Usage: ``python tools/bench_fc_learn_on_replay.py [--parent DIR] [--reps 5] [--out profiles/fc_learn_on_replay.json]``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT  # before the imports
sys.path[:0] = [TREE, os.path.join(TREE, "i-dqn_amd")]
CONFIGS = {  # name: (arch, frame shape, dtype, stack, obs, A, K, features)
    "lunar": ("fc", (8,), "float32", 1, 8, 4, 3, [100, 100]),
    "fc_520": ("fc", (8,), "float32", 1, 8, 4, 3, [520]),
    "gcnn_smoke": ("cnn", (84, 84), "uint8", 4, (84, 84, 4), 6, 1, [2, 3, 1, 15]),
}
B = 32


def update_leg(name, calls, rounds):
    import numpy as np
    import torch

    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    arch, shape, dtype, stack, obs, A, K, feats = CONFIGS[name]

    def side(fuse):
        rb = ReplayBuffer(UniformSamplingDistribution(0), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(1)
        for i in range(2500):
            frame = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == "uint8" else rng.standard_normal(shape).astype(np.float32)
            rb.add(TransitionElement(frame, int(rng.integers(A)), float(rng.normal()), i % 200 == 199, i % 200 == 199))
        rb.reuse_sample_buffers = True
        agent = iDQN(0, obs, A, K, feats, arch, 3e-4, 0.99, 1, 1, 10**9, 10**9)
        agent.fuse_replay_sampling = fuse
        return agent, rb

    sides = {"fused": side(True), "two_calls": side(False)}

    def region(agent, rb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            agent.update_online_params(i, rb)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    for agent, rb in sides.values():
        region(agent, rb)
    assert sides["fused"][0].__dict__.get("_replay_fc_ok") is True, "the replay-sourced route did not run"
    assert sides["two_calls"][0].__dict__.get("_replay_fc_ok") is None
    for n in ("_online", "_mu", "_nu"):  # the same steps on both sides, bit for bit
        assert torch.equal(getattr(sides["fused"][0], n), getattr(sides["two_calls"][0], n)), n
    reg = {k: [] for k in sides}
    for _ in range(rounds):
        for k, (agent, rb) in sides.items():
            reg[k].append(region(agent, rb))
    print("RESULT" + json.dumps({"leg": "update", "config": name, "staged": os.environ.get("IDQN_FC_REPLAY_STAGE") == "1",
                                 "us_per_update": {k: float(np.median(v)) for k, v in reg.items()}, "regions": reg}), flush=True)


def trainer_leg(leg, warmup, steps):
    import torch

    from experiments.base.dqn import Trainer, VectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    p = dict(epsilon_end=0.01, epsilon_duration=1000, n_epochs=2, n_training_steps_per_epoch=warmup, n_initial_samples=1000,
             horizon=1000, wandb=NullLogger())
    agent = iDQN(0, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 200, 10)
    kw = dict(batch_size=B, max_capacity=10_000, stack_size=1, update_horizon=1, gamma=0.99)
    if leg == "trainer":
        rb = ReplayBuffer(UniformSamplingDistribution(0), **kw)
        env = SyntheticVector(0, episode_length=200)
        trainer = Trainer(prng.PRNGKey(0), p, agent, env, rb)
        env.reset()
    else:
        rb = VectorReplayBuffer(UniformSamplingDistribution(0), n_envs=int(leg), **kw)
        envs = [SyntheticVector(e, episode_length=200) for e in range(int(leg))]
        trainer = VectorTrainer(prng.PRNGKey(0), p, agent, envs, rb)
        for env in envs:
            env.reset()
    rb.reuse_sample_buffers = True
    trainer.run_epoch(0)
    torch.cuda.synchronize()
    p["n_training_steps_per_epoch"] = steps
    before, t0 = trainer.total_steps, time.perf_counter()
    trainer.run_epoch(1)
    torch.cuda.synchronize()
    rate = (trainer.total_steps - before) / (time.perf_counter() - t0)
    print("RESULT" + json.dumps({"leg": "trainer", "E": leg, "tree": "parent" if TREE != ROOT else "this", "env_steps_per_s": rate,
                                 "replay_sourced": agent.__dict__.get("_replay_fc_ok")}), flush=True)


def summary(values):
    s = sorted(values)
    return {"median": s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), "min": s[0], "max": s[-1], "n": len(s)}


def verdict(a, b, lower_is_better):
    """Which of two {median, min, max} is faster, or 'inside the spread' where the intervals overlap."""
    if a["max"] < b["min"]:
        return "first" if lower_is_better else "second"
    if b["max"] < a["min"]:
        return "second" if lower_is_better else "first"
    return "inside the spread"


def driver(a):
    def run(leg, tree=None, env=None):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(a.calls), "--rounds", str(a.rounds)]
        if tree:
            cmd += ["--tree", tree, "--out", a.out]  # (--tree is read from the middle of the argument list)
        out = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        if out.returncode or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"leg {leg} failed with status {out.returncode}: nothing more is started")
        print(line[0], flush=True)
        return json.loads(line[0][6:])

    res = {"method": {"reps": a.reps, "calls": a.calls, "rounds": a.rounds, "batch": B}, "update_online_params_us": {}, "trainer_env_steps_per_s": {}}
    for name in CONFIGS:
        r = run(f"update:{name}")
        fused, two = summary(r["regions"]["fused"]), summary(r["regions"]["two_calls"])
        res["update_online_params_us"][name] = {"fused": fused, "two_calls": two, "two_calls_over_fused": two["median"] / fused["median"],
                                                "faster": {"first": "fused", "second": "two_calls"}.get(verdict(fused, two, True), "inside the spread")}
    r = run("update:lunar:staged", env={"IDQN_FC_REPLAY_STAGE": "1"})
    staged, in_kernel = summary(r["regions"]["fused"]), res["update_online_params_us"]["lunar"]["fused"]
    res["lunar_gather_ab_us"] = {"in_kernel": in_kernel, "staging_launch": staged,
                                 "faster": {"first": "in_kernel", "second": "staging_launch"}.get(verdict(in_kernel, staged, True), "inside the spread")}
    if a.parent:
        for leg in ("trainer", "1", "8", "32"):
            rates = {"this": [], "parent": []}
            for _ in range(a.reps):
                for tree in ("this", "parent"):
                    rates[tree].append(run(f"trainer:{leg}", tree=a.parent if tree == "parent" else None)["env_steps_per_s"])
            this, parent = summary(rates["this"]), summary(rates["parent"])
            res["trainer_env_steps_per_s"]["Trainer" if leg == "trainer" else f"VectorTrainer E={leg}"] = {
                "this": this, "parent": parent, "this_over_parent": this["median"] / parent["median"],
                "faster": {"first": "this", "second": "parent"}.get(verdict(this, parent, False), "inside the spread")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose package and library a leg measures (default: this one)")
    ap.add_argument("--parent", default=None, help="driver: a built checkout of the parent commit for the trainer legs")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_learn_on_replay.json"))
    a = ap.parse_args()
    if a.leg is None:
        return driver(a)
    kind, _, rest = a.leg.partition(":")
    if kind == "update":
        return update_leg(rest.split(":")[0], a.calls, a.rounds)
    return trainer_leg(rest, a.warmup, a.steps)


if __name__ == "__main__":
    main()
