"""What a seed group costs against its members driven one after the other (``idqn_group_*``, csrc/fc_group_kernels.h), on the
LunarLander net (fc, obs 8, [100, 100], A = 4, K = 3, B = 32) at S = 1, 2, 4, 8, 16, 32 members:

  step     one ``idqn_group_learn_on_replay_fc`` call            against S ``idqn_learn_on_replay_fc`` calls
  steps    one ``idqn_group_learn_steps_on_replay_fc``, n = 10   against S ``idqn_learn_steps_on_replay_fc`` calls, n = 10
  act      one ``idqn_group_act_host_fc`` call, S states         against S ``idqn_act_host`` calls
  trainer  ``SeedTrainer`` on S seeds (summed env-steps/s)       against S ``Trainer`` runs one after the other (S = 1, 4, 16)

Both sides of a pair run on the SAME handles in one process (the solo code is the single-handle entries as they are); regions
of ``--calls`` calls alternate between the sides ``--rounds`` times, each timed on the host clock with a device synchronisation
at both ends; per side the median and [min, max] of the regions, microseconds per call.  ``group_is_default`` is the project's
rule: the group's median lies below the solo chain's minimum.  Writes ``profiles/seed_group.json``.
Usage: ``python tools/bench_seed_group.py [--calls 200] [--rounds 7] [--no-trainer] [--out profiles/seed_group.json]``.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
SIZES, B, N_STEPS = (1, 2, 4, 8, 16, 32), 32, 10


def summary(v):
    s = sorted(v)
    return {"median": s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]), "min": s[0], "max": s[-1], "n": len(s)}


def pair(group_fn, solo_fn, calls, rounds):
    import torch

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / calls

    region(group_fn), region(solo_fn)  # warm-up: allocations, graph capture
    reg = {"group": [], "solo": []}
    for _ in range(rounds):
        reg["group"].append(region(group_fn))
        reg["solo"].append(region(solo_fn))
    g, s = summary(reg["group"]), summary(reg["solo"])
    return {"group": g, "solo": s, "solo_over_group": s["median"] / g["median"], "group_is_default": g["median"] < s["min"]}


def members(S):
    import numpy as np

    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    agents, rbs = [], []
    for g in range(S):
        rb = ReplayBuffer(UniformSamplingDistribution(g), batch_size=B, max_capacity=2000, stack_size=1, update_horizon=1, gamma=0.99)
        rng = np.random.default_rng(g)
        for i in range(2500):
            rb.add(TransitionElement(rng.standard_normal(8).astype(np.float32), int(rng.integers(4)), float(rng.normal()), i % 200 == 199,
                                     i % 200 == 199))
        agents.append(iDQN(g, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 10**9, 10**9))
        agents[-1]._ensure_handle(32)
        rbs.append(rb)
    return agents, rbs


def calls_at(S, calls, rounds):
    import numpy as np
    import torch

    from slimdqn import _hip
    from slimdqn.networks.group import AgentGroup

    lib = _hip.lib()
    agents, rbs = members(S)
    views = [rb.ring_view() for rb in rbs]
    rings = AgentGroup._rings(views)
    group = C.c_void_p()
    _hip.check(lib.idqn_group_create((C.c_void_p * S)(*[a._handle.value for a in agents]), S, C.byref(group)), "idqn_group_create")
    one = np.ascontiguousarray(np.stack([rb.sample_slots() for rb in rbs]), np.int32)                                   # [S][B]
    ten = np.ascontiguousarray(np.stack([np.stack([rb.sample_slots() for _ in range(N_STEPS)]) for rb in rbs]), np.int32)  # [S][n][B]
    q = _hip.current_stream()
    ring_args = [(_hip.ptr(v[0]), int(v[1]), int(v[2]), _hip.ptr(v[3])) for v in views]

    def group_step():
        _hip.check(lib.idqn_group_learn_on_replay_fc(group, rings, one.ctypes.data, B, B, 0, q), "group step")

    def solo_step():
        for a, r, s in zip(agents, ring_args, one):
            _hip.check(lib.idqn_learn_on_replay_fc(a._handle, *r, s.ctypes.data, B, 1, B, 0, q), "solo step")

    def group_steps():
        _hip.check(lib.idqn_group_learn_steps_on_replay_fc(group, rings, ten.ctypes.data, N_STEPS, B, B, 0, q), "group steps")

    def solo_steps():
        for a, r, s in zip(agents, ring_args, ten):
            _hip.check(lib.idqn_learn_steps_on_replay_fc(a._handle, *r, s.ctypes.data, N_STEPS, B, 1, B, 0, q), "solo steps")

    pin = torch.from_numpy(np.random.default_rng(0).standard_normal((32, 8)).astype(np.float32)).pin_memory()
    q_out = torch.zeros((32, 4), dtype=torch.float32, device="cuda")
    acts = torch.zeros(32, dtype=torch.int32).pin_memory()
    member, heads = np.arange(S, dtype=np.int32), np.ascontiguousarray(np.arange(S) % 3, np.int32)
    rows = [C.c_void_p(pin[e].data_ptr()) for e in range(S)]

    def group_act():
        _hip.check(lib.idqn_group_act_host_fc(group, 0, member.ctypes.data, heads.ctypes.data, C.c_void_p(pin.data_ptr()), S, _hip.ptr(q_out),
                                              C.c_void_p(acts.data_ptr()), q), "group act")

    def solo_act():
        for e, a in enumerate(agents):
            _hip.check(lib.idqn_act_host(a._handle, 0, int(heads[e]), rows[e], _hip.ptr(q_out), C.c_void_p(acts.data_ptr()), q), "solo act")

    out = {"step_us": pair(group_step, solo_step, calls, rounds),
           f"steps_n{N_STEPS}_us": pair(group_steps, solo_steps, max(1, calls // 4), rounds),
           "act_us": pair(group_act, solo_act, calls, rounds)}
    _hip.check(lib.idqn_group_destroy(group), "idqn_group_destroy")
    return out


def trainer_at(S, warmup, steps, reps):
    import torch

    from experiments.base.dqn import Trainer
    from experiments.base.seeds import SeedTrainer
    from experiments.base.utils import NullLogger
    from slimdqn import prng
    from slimdqn.environments.synthetic import SyntheticVector
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    def triple(seed):
        p = dict(seed=seed, epsilon_end=0.01, epsilon_duration=1000, n_epochs=1, n_training_steps_per_epoch=warmup + steps,
                 n_initial_samples=1000, horizon=1000, wandb=NullLogger())
        rb = ReplayBuffer(UniformSamplingDistribution(seed), batch_size=B, max_capacity=10_000, stack_size=1, update_horizon=1, gamma=0.99)
        rb.reuse_sample_buffers = True
        return p, iDQN(seed, 8, 4, 3, [100, 100], "fc", 3e-4, 0.99, 1, 1, 200, 10), SyntheticVector(seed, episode_length=200), rb

    def timed(run, n_env_steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return n_env_steps / (time.perf_counter() - t0)

    rates = {"seed_trainer": [], "sequential_trainers": []}
    total = S * (warmup + steps)  # (episodes of 200 steps: every epoch ends exactly on its budget)
    for _ in range(reps):
        ts = [triple(s) for s in range(S)]
        st = SeedTrainer([prng.PRNGKey(s) for s in range(S)], [t[0] for t in ts], [t[1] for t in ts], [t[2] for t in ts], [t[3] for t in ts])
        rates["seed_trainer"].append(timed(st.run, total))
        ts = [triple(s) for s in range(S)]
        trainers = [Trainer(prng.PRNGKey(s), *t) for s, t in enumerate(ts)]
        rates["sequential_trainers"].append(timed(lambda: [t.run() for t in trainers], total))
    a, b = summary(rates["seed_trainer"]), summary(rates["sequential_trainers"])
    return {"seed_trainer": a, "sequential_trainers": b, "seed_over_sequential": a["median"] / b["median"],
            "note": "summed env-steps/s over the whole run, the first 1000 steps without gradient steps included"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_group.json"))
    a = ap.parse_args()
    res = {"method": {"calls": a.calls, "rounds": a.rounds, "batch": B, "n_steps": N_STEPS, "net": "fc obs 8 [100, 100] A 4 K 3"}, "S": {}}
    for S in SIZES:
        res["S"][str(S)] = calls_at(S, a.calls, a.rounds)
        print("RESULT" + json.dumps({"S": S, **res["S"][str(S)]}), flush=True)
    res["group_default_sizes"] = {k: [int(S) for S, r in res["S"].items() if r[k]["group_is_default"]] for k in res["S"]["1"]}
    if not a.no_trainer:
        res["trainer_env_steps_per_s"] = {}
        for S in (1, 4, 16):
            res["trainer_env_steps_per_s"][str(S)] = trainer_at(S, a.warmup, a.steps, a.reps)
            print("RESULT" + json.dumps({"trainer_S": S, **res["trainer_env_steps_per_s"][str(S)]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
