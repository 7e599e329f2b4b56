"""What greedy actions for n host states cost on an impala handle: ONE ``idqn_act_host_many_impala`` call
(csrc/imp_act_many_kernels.h) against the loop of n ``idqn_act_host`` calls -- what ``DeviceAgent._best_actions`` does for
these handles otherwise -- on the same handle in the same process.  The n = 1 loop is the single-state ``idqn_act_host`` cost.

  workload        impala, (84, 84, 4), [32, 64, 64, 512], A = 6, K = 5
  reference_test  impala, (84, 84, 4), [3, 7, 5, 9], A = 4, K = 2 (the reference's test widths)

  one_head   every state on head 0;
  drawn      heads drawn uniformly (seeded) -- 16 assignments per n, used in turn by both sides.

The method is ``tools/bench_fc_act_many.py``'s: both sides go through the C ABI with the states already in pinned memory and end
with the actions on the host (both calls block), so the host clock around a call is the whole cost.  Regions of calls alternate
between the two sides, ``--rounds`` (7) times; a side's figure is the median over its regions of the region's median call, the
spread the range of the region medians.  Every (n, pattern) first checks that both sides return the same actions and Q rows.

THE RULE for ``DeviceAgent.act_many_imp_sizes``: n takes the one call by default when the one call's median is below the MINIMUM
of the loop's regions, in every configuration and pattern measured; every other n (SLOWER somewhere, or not measured) stays on
the loop.  The sizes the rule gives are written to ``defaults`` in ``profiles/impala_act_many.json``.
Usage: ``python tools/bench_impala_act_many.py [--out profiles/impala_act_many.json] [--rounds 7] [--sizes 1,2,8,32]``.

``--trainer-leg on|off`` runs ONE leg of a synthetic Atari-shaped training loop instead (``VectorTrainer``, E = 8, the workload's
widths, a gradient step every 4 environment steps) with the route on for every n or forced off, and prints one JSON line with
its environment steps per second.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
CONFIGS = {  # name: (obs, A, K, features)
    "workload": ((84, 84, 4), 6, 5, [32, 64, 64, 512]),
    "reference_test": ((84, 84, 4), 4, 2, [3, 7, 5, 9]),
}
DRAWS = 16


def bench_config(name, a, sizes, np, torch):
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    obs, A, K, feats = CONFIGS[name]
    agent = iDQN(0, obs, A, K, feats, "impala", 1e-3, 0.99, 1, 1, 10**9, 10**9)
    agent._ensure_handle(32)
    lib, h, stream = _hip.lib(), agent._handle, _hip.current_stream()
    rng = np.random.default_rng(0)
    n_el = int(np.prod(obs))
    pin = torch.from_numpy(rng.integers(0, 256, size=(32, n_el), dtype=np.uint8)).pin_memory()
    state_ptr = [C.c_void_p(pin.data_ptr() + e * n_el) for e in range(32)]
    q_many = torch.zeros((32, A), dtype=torch.float32, device="cuda")
    q_loop = torch.zeros((32, A), dtype=torch.float32, device="cuda")
    acts_many, acts_loop = torch.zeros(32, dtype=torch.int32).pin_memory(), torch.zeros(32, dtype=torch.int32).pin_memory()
    many_np, loop_np = acts_many.numpy(), acts_loop.numpy()
    many_q_ptr, many_ptr = _hip.ptr(q_many), C.c_void_p(acts_many.data_ptr())
    loop_q_ptr = [C.c_void_p(q_loop.data_ptr() + 4 * A * e) for e in range(32)]
    loop_ptr = [C.c_void_p(acts_loop.data_ptr() + 4 * e) for e in range(32)]

    def many(heads):
        rc = lib.idqn_act_host_many_impala(h, 0, heads.ctypes.data, state_ptr[0], heads.size, many_q_ptr, many_ptr, stream)
        if rc:
            _hip.check(rc, "idqn_act_host_many_impala")

    def loop(heads):
        for e in range(heads.size):
            rc = lib.idqn_act_host(h, 0, int(heads[e]), state_ptr[e], loop_q_ptr[e], loop_ptr[e], stream)
            if rc:
                _hip.check(rc, "idqn_act_host")

    def region(fn, draws, calls):
        ts = []
        for i in range(calls):
            heads = draws[i % len(draws)]
            t0 = time.perf_counter()
            fn(heads)
            ts.append(time.perf_counter() - t0)
        return 1e6 * float(np.median(ts))

    res = {"config": {"arch": "impala", "obs": obs, "features": feats, "A": A, "K": K}, "one_head": {}, "drawn": {}}
    for pattern in ("one_head", "drawn"):
        for E in sizes:
            calls = max(10, min(100, a.calls // E))
            if pattern == "one_head":
                draws = [np.zeros(E, np.int32)]
            else:
                draws = [np.ascontiguousarray(rng.integers(0, K, size=E), np.int32) for _ in range(DRAWS)]
            for heads in draws:  # warm-up of every graph either side replays, and the same answers from both
                for _ in range(2):
                    many(heads)
                    loop(heads)
                torch.cuda.synchronize()
                assert (many_np[:E] == loop_np[:E]).all(), (name, pattern, E, heads, many_np[:E], loop_np[:E])
                assert q_many[:E].cpu().numpy().tobytes() == q_loop[:E].cpu().numpy().tobytes(), (name, pattern, E, heads)
            reg = {"many": [], "loop": []}
            for _ in range(a.rounds):
                reg["many"].append(region(many, draws, calls))
                reg["loop"].append(region(loop, draws, calls))
            m, l = float(np.median(reg["many"])), float(np.median(reg["loop"]))
            verdict = "default" if m < min(reg["loop"]) else "SLOWER"
            res[pattern][str(E)] = {
                "many_us_per_call": m, "many_us_per_action": m / E, "many_regions": reg["many"],
                "loop_us_per_call": l, "loop_us_per_action": l / E, "loop_regions": reg["loop"],
                "loop_over_many": l / m, "rule": verdict, "calls_per_region": calls}
            print(json.dumps({"config": name, "pattern": pattern, "n": E, "many_us": round(m, 1), "loop_us": round(l, 1),
                              "loop_min_us": round(min(reg["loop"]), 1), "loop_over_many": round(l / m, 2), "rule": verdict}), flush=True)
    one = res["one_head"].get("1")
    if one:
        res["single_state_act_host_us"] = {"median": one["loop_us_per_call"], "min": min(one["loop_regions"]), "max": max(one["loop_regions"])}
    agent._destroy_handle()
    return res


def trainer_leg(leg, warmup, steps):
    """Environment steps / s of one epoch of ``steps`` steps, after a warm-up epoch that passes ``n_initial_samples``."""
    import numpy as np
    import torch

    from experiments.base.dqn import VectorTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticAtari
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution
    from slimdqn.sample_collection.vector_replay_buffer import VectorReplayBuffer

    obs, A, K, feats = CONFIGS["workload"]
    E = 8
    p = dict(epsilon_end=0.01, epsilon_duration=200, n_epochs=2, n_training_steps_per_epoch=warmup, n_initial_samples=200, horizon=1000,
             wandb=NullLogger())
    agent = iDQN(0, obs, A, K, feats, "impala", 6.25e-5, 0.99, 1, 4, 2000, 1000, adam_eps=1.5e-4)
    agent.act_many_imp_sizes = frozenset(range(1, 33)) if leg == "on" else frozenset()
    rb = VectorReplayBuffer(UniformSamplingDistribution(0), 32, 4096, stack_size=4, update_horizon=1, gamma=0.99,
                            clipping=lambda r: float(np.clip(r, -1, 1)), n_envs=E)
    rb.reuse_sample_buffers = True
    envs = [SyntheticAtari(e, n_actions=A, episode_length=100) for e in range(E)]
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
    print("RESULT" + json.dumps({"leg": leg, "E": E, "env_steps_per_s": round(rate, 1), "steps": trainer.total_steps - before,
                                 "vectorised_acting": agent.__dict__.get("_act_many_imp_ok")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer-leg", default=None, choices=["on", "off"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_act_many.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--sizes", default="1,2,8,32")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    a = ap.parse_args()
    if a.trainer_leg is not None:
        return trainer_leg(a.trainer_leg, a.warmup, a.steps)
    import numpy as np
    import torch

    sizes = [int(s) for s in a.sizes.split(",")]
    res = {"method": {"rounds": a.rounds, "calls": a.calls, "draws": DRAWS, "sizes": sizes, "device": torch.cuda.get_device_name(0)}}
    names = a.configs.split(",")
    for name in names:
        res[name] = bench_config(name, a, sizes, np, torch)
    res["defaults"] = sorted(E for E in sizes if all(res[n][pat][str(E)]["rule"] == "default" for n in names for pat in ("one_head", "drawn")))
    print(json.dumps({"defaults": res["defaults"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
