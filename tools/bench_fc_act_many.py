"""What greedy actions for E host states cost on MLP and general-shape cnn handles: ONE ``idqn_act_host_many_fc`` call
(csrc/fc_act_many_kernels.h) against a loop of E ``idqn_act_host`` calls -- what ``DeviceAgent._best_actions`` did for these
handles before -- on the same handle in the same process.  Four configurations, E in {1, 2, 4, 8, 16, 32}, two head patterns:

  lunar_k3    fc, obs 8, [100, 100], A = 4, K = 3 (the LunarLander experiment)         k_fc_act_many1
  lunar_k5    the same at K = 5
  fc_520      fc, obs 8, [520], A = 4, K = 3 (past FC_MAX_WIDTH)                       k_fc_act_many
  gcnn_smoke  cnn, (84, 84, 4), [2, 3, 1, 15], A = 6, K = 1 (the reference's smoke)    3 x k_gconv_fwd_many + k_fc_act_many

  one_head   every state on head 0;
  drawn      heads drawn uniformly (seeded) -- 16 assignments per E, used in turn by both sides.

The method is ``tools/bench_act_many.py``'s: both sides go through the C ABI with the states already in pinned memory and end
with the actions on the host (both calls block), so the host clock around a call is the whole cost.  Regions of ``--calls``
calls alternate between the two sides, ``--rounds`` times; a side's figure is the median over its regions of the region's median
call, the spread the range of the region medians.  Every (E, pattern) first checks that both sides return the same actions.
``faster`` names a side only where the two spreads do not overlap.  Writes ``profiles/fc_act_many.json``.
Usage: ``python tools/bench_fc_act_many.py [--out profiles/fc_act_many.json] [--rounds 5] [--calls 200] [--configs a,b]``.

``--trainer-leg {trainer,1,2,8,32}`` runs ONE leg of the LunarLander-shaped synthetic training loop instead (fc [100, 100],
K = 3, B = 32, the reference's update schedule: a gradient step per environment step, target update every 200, sync every
10): the single-environment ``Trainer`` or ``VectorTrainer`` at that E, and prints one JSON line with its environment steps
per second.  ``--tree DIR`` imports the package, the experiments and the built library from another checkout (one of the
parent commit, built with its own ``build()``) instead of this one: a comparison between two commits runs the legs of both
trees from this one file in alternating processes, three repetitions per leg, e.g.

    for rep in 0 1 2; do for leg in trainer 1 2 8 32; do for tree in . ../parent; do
        python tools/bench_fc_act_many.py --trainer-leg $leg --tree $tree; done; done; done
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT  # before the imports
sys.path[:0] = [TREE, os.path.join(TREE, "i-dqn_amd")]
CONFIGS = {  # name: (arch, obs, A, K, features)
    "lunar_k3": ("fc", 8, 4, 3, [100, 100]),
    "lunar_k5": ("fc", 8, 4, 5, [100, 100]),
    "fc_520": ("fc", 8, 4, 3, [520]),
    "gcnn_smoke": ("cnn", (84, 84, 4), 6, 1, [2, 3, 1, 15]),
}
SIZES, DRAWS = (1, 2, 4, 8, 16, 32), 16


def bench_config(name, a, np, torch):
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    arch, obs, A, K, feats = CONFIGS[name]
    agent = iDQN(0, obs, A, K, feats, arch, 1e-3, 0.99, 1, 1, 10**9, 10**9)
    agent._ensure_handle(32)
    lib, h, stream = _hip.lib(), agent._handle, _hip.current_stream()
    rng = np.random.default_rng(0)
    n_el = int(np.prod(obs))
    if arch == "cnn":
        pin, item = torch.from_numpy(rng.integers(0, 256, size=(32, n_el), dtype=np.uint8)).pin_memory(), 1
    else:
        pin, item = torch.from_numpy(rng.standard_normal((32, n_el)).astype(np.float32)).pin_memory(), 4
    state_ptr = [C.c_void_p(pin.data_ptr() + e * n_el * item) for e in range(32)]
    q_out = torch.zeros((32, A), dtype=torch.float32, device="cuda")
    acts_many, acts_loop = torch.zeros(32, dtype=torch.int32).pin_memory(), torch.zeros(32, dtype=torch.int32).pin_memory()
    many_np, loop_np = acts_many.numpy(), acts_loop.numpy()
    q_ptr, many_ptr = _hip.ptr(q_out), C.c_void_p(acts_many.data_ptr())
    loop_ptr = [C.c_void_p(acts_loop.data_ptr() + 4 * e) for e in range(32)]

    def many(heads):
        rc = lib.idqn_act_host_many_fc(h, 0, heads.ctypes.data, state_ptr[0], heads.size, q_ptr, many_ptr, stream)
        if rc:
            _hip.check(rc, "idqn_act_host_many_fc")

    def loop(heads):
        for e in range(heads.size):
            rc = lib.idqn_act_host(h, 0, int(heads[e]), state_ptr[e], q_ptr, loop_ptr[e], stream)
            if rc:
                _hip.check(rc, "idqn_act_host")

    def region(fn, draws):
        ts = []
        for i in range(a.calls):
            heads = draws[i % len(draws)]
            t0 = time.perf_counter()
            fn(heads)
            ts.append(time.perf_counter() - t0)
        return 1e6 * float(np.median(ts))

    res = {"config": {"arch": arch, "obs": obs, "features": feats, "A": A, "K": K}, "one_head": {}, "drawn": {}}
    for pattern in ("one_head", "drawn"):
        for E in SIZES:
            if pattern == "one_head" or K == 1:
                draws = [np.zeros(E, np.int32)]
            else:
                draws = [np.ascontiguousarray(rng.integers(0, K, size=E), np.int32) for _ in range(DRAWS)]
            for heads in draws:  # warm-up of every graph either side replays, and the same answers from both
                for _ in range(3):
                    many(heads)
                    loop(heads)
                assert (many_np[:E] == loop_np[:E]).all(), (name, pattern, E, heads, many_np[:E], loop_np[:E])
            reg = {"many": [], "loop": []}
            for _ in range(a.rounds):
                reg["many"].append(region(many, draws))
                reg["loop"].append(region(loop, draws))
            m, l = float(np.median(reg["many"])), float(np.median(reg["loop"]))
            faster = "many" if max(reg["many"]) < min(reg["loop"]) else "loop" if max(reg["loop"]) < min(reg["many"]) else None
            res[pattern][str(E)] = {
                "many_us_per_call": m, "many_us_per_action": m / E, "many_regions": reg["many"],
                "loop_us_per_call": l, "loop_us_per_action": l / E, "loop_regions": reg["loop"],
                "loop_over_many": l / m, "faster": faster}
            print(json.dumps({"config": name, "pattern": pattern, "E": E, "many_us": round(m, 1), "loop_us": round(l, 1),
                              "loop_over_many": round(l / m, 2), "faster": faster}), flush=True)
    agent._destroy_handle()
    return res


def trainer_leg(leg, warmup, steps):
    """Environment steps / s of one epoch of ``steps`` steps, after a warm-up epoch that passes ``n_initial_samples``."""
    import numpy as np  # noqa: F401
    import torch

    from experiments.base.dqn import Trainer, VectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    os.environ.setdefault("IDQN_STEP_GRAPH", "1")  # as experiments/base/launch.py
    p = dict(epsilon_end=0.01, epsilon_duration=1000, n_epochs=2, n_training_steps_per_epoch=warmup, n_initial_samples=1000,
             horizon=1000, wandb=NullLogger())
    agent = iDQN(0, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 200, 10)
    kw = dict(batch_size=32, max_capacity=10_000, stack_size=1, update_horizon=1, gamma=0.99)
    if leg == "trainer":
        rb = ReplayBuffer(UniformSamplingDistribution(0), **kw)
        rb.reuse_sample_buffers = True
        env = SyntheticVector(0, episode_length=200)
        trainer = Trainer(prng.PRNGKey(0), p, agent, env, rb)
        env.reset()
    else:
        rb = VectorReplayBuffer(UniformSamplingDistribution(0), n_envs=int(leg), **kw)
        rb.reuse_sample_buffers = True
        envs = [SyntheticVector(e, episode_length=200) for e in range(int(leg))]
        trainer = VectorTrainer(prng.PRNGKey(0), p, agent, envs, rb)
        for env in envs:
            env.reset()
    trainer.run_epoch(0)
    torch.cuda.synchronize()
    p["n_training_steps_per_epoch"] = steps
    before, t0 = trainer.total_steps, time.perf_counter()
    trainer.run_epoch(1)
    torch.cuda.synchronize()
    rate = (trainer.total_steps - before) / (time.perf_counter() - t0)
    print("RESULT" + json.dumps({"tree": TREE, "leg": leg, "env_steps_per_s": round(rate, 1), "steps": trainer.total_steps - before,
                                 "vectorised_acting": agent.__dict__.get("_act_many_fc_ok")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer-leg", default=None)
    ap.add_argument("--tree", default=ROOT, help="checkout whose package and library are measured (default: this one)")
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_act_many.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    if a.trainer_leg is not None:
        return trainer_leg(a.trainer_leg, a.warmup, a.steps)
    import numpy as np
    import torch

    res = {"method": {"rounds": a.rounds, "calls": a.calls, "draws": DRAWS, "device": torch.cuda.get_device_name(0)}}
    for name in a.configs.split(","):
        res[name] = bench_config(name, a, np, torch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
