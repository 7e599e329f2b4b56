"""A/B of the impala f32 matrix-core Dense_0 forward (IDQN_IMP_D0=mfma, csrc/impala_d0_mx_kernels.h); writes
profiles/impala_d0.json.

    python tools/bench_impala_d0.py --parent-lib <libidqn_hip.so of the parent commit> [--regions 5] [--steps 10] [--out ...]

The way of tools/bench_impala_mx.py: every leg is a child process of its own that lives for the whole run (a library is loaded
once per process, and the mode is read when a handle is created), and the learner step is timed in alternating regions, ms
per step as median [min, max].  Six legs: ``parent`` / ``off`` / ``on`` = the parent commit's library (built into a second
directory, loaded through IDQN_HIP_LIB; the yardstick) / this tree with the variable unset / this tree with IDQN_IMP_D0=mfma,
and the same three with IDQN_IMP_CONV=bf16x3 (``parent_conv``, ``off_conv``, ``on_conv``).  Configurations: the workload's
widths at B = 32 and at B = 256, and the reference's test widths.  Verdicts by the standing rule -- a gain only where the
mode-on median lies below the parent's minimum, SLOWER in capitals where it lies above its maximum.  Also: us per launch of
k_imp_d0_fwd (``off``) against k_imp_d0_fwd_mx (``on``) from idqn_profile_table, and us per call of idqn_act_host and of
idqn_q_values at n = 32 (workload's widths), ``off`` against ``on``.  bench.py is not involved.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]

# name: (obs, features, A, K, B, steps per region relative to --steps)
CONFIGS = {
    "workload": ((84, 84, 4), [32, 64, 64, 512], 6, 5, 32, 1.0),
    "reference_test": ((84, 84, 4), [3, 7, 5, 9], 4, 2, 32, 1.0),
    "workload_b256": ((84, 84, 4), [32, 64, 64, 512], 6, 5, 256, 0.3),
}
VARS = ("IDQN_IMP_D0", "IDQN_IMP_CONV", "IDQN_IMP_WGRAD", "IDQN_HIP_LIB")
Batch = namedtuple("Batch", "state action reward next_state is_terminal")


def child():
    """One leg: answers ``region <config> <steps>``, ``table <config>``, ``drop <config>``, ``act <calls>`` and ``quit`` on stdin"""
    import numpy as np
    import torch

    from oracle import qnet_ref as Q
    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    agents = {}

    def get(name):
        if name not in agents:
            obs, feats, A, K, B, _ = CONFIGS[name]
            agent = iDQN(0, obs, A, K, feats, "impala", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4)
            agent._load_flat(agent._online, Q.init_params(0, "impala", obs, A, feats, K))
            agent._load_flat(agent._target, Q.init_params(1, "impala", obs, A, feats, K))
            batch = Q.synthetic_batch(2, B, obs, A, "cnn")
            agents[name] = (agent, Batch(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch]), batch)
        return agents[name]

    def regions_of(run, calls):
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(calls):
                run()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e6 / calls)
        return {"median": statistics.median(out), "min": min(out), "max": max(out)}

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        out = None
        if cmd[0] == "region":
            agent, dev, _ = get(cmd[1])
            n = int(cmd[2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                agent._learn(dev)
            torch.cuda.synchronize()
            out = (time.perf_counter() - t0) * 1e3 / n
        elif cmd[0] == "table":
            agent, dev, _ = get(cmd[1])
            for _ in range(3):
                agent._learn(dev, flags=_hip.F_PROFILE_ALL)
            torch.cuda.synchronize()
            table = C.create_string_buffer(1 << 16)
            _hip.check(_hip.lib().idqn_profile_table(agent._handle, table, len(table)), "idqn_profile_table")
            out = table.value.decode(errors="replace").splitlines()
            agent._learn(dev)  # (a step without the flag: the timeline is off again)
        elif cmd[0] == "drop":  # free a configuration's handle and arenas before the next one
            agent, _, _ = agents.pop(cmd[1])
            agent._destroy_handle()
            del agent
            torch.cuda.empty_cache()
        elif cmd[0] == "act":
            agent, _, batch = get("workload")
            calls = int(cmd[1])
            states = [np.asarray(s) for s in batch[0]]
            s32 = torch.from_numpy(np.stack(states[:32])).cuda()
            out = {"act_host_us_per_call": regions_of(lambda: agent._best_action(0, 1, states[0]).item(), calls),
                   "q_values_n32_us_per_call": regions_of(lambda: agent._q_values(0, 1, s32), calls)}
        print("RESULT" + json.dumps(out), flush=True)


def ask(proc, text):
    proc.stdin.write(text + "\n")
    proc.stdin.flush()
    while True:
        line = proc.stdout.readline()
        if not line:
            raise RuntimeError("a leg ended: rc %s" % proc.poll())
        if line.startswith("RESULT"):
            return json.loads(line[len("RESULT"):])


def verdict(leg, yard):
    if leg["median"] < yard["min"]:
        return "FASTER: the median lies below the yardstick's minimum (%.3fx on the medians)" % (yard["median"] / leg["median"])
    if leg["median"] > yard["max"]:
        return "SLOWER: the median lies above the yardstick's maximum (%.3fx on the medians)" % (leg["median"] / yard["median"])
    return "inside the spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--act-calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_d0.json"))
    args = ap.parse_args()
    if args.leg:
        return child()
    assert args.regions >= 5
    on, conv = {"IDQN_IMP_D0": "mfma"}, {"IDQN_IMP_CONV": "bf16x3"}
    envs = {"off": {}, "on": on, "off_conv": conv, "on_conv": {**on, **conv}}
    if args.parent_lib:
        lib = {"IDQN_HIP_LIB": os.path.abspath(args.parent_lib)}
        envs = {"parent": lib, "parent_conv": {**lib, **conv}, **envs}
    legs = {}
    for leg, extra in envs.items():
        env = {k: v for k, v in os.environ.items() if k not in VARS}
        env.update(extra)
        legs[leg] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--leg"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    result = {"what": "impala learner step, ms per step, median [min, max] of alternating regions (" + ", ".join(envs) + ", ...)",
              "legs": {leg: ", ".join("%s=%s" % (k, "<the parent commit's library>" if k == "IDQN_HIP_LIB" else v) for k, v in e.items()) or "this tree, nothing set"
                       for leg, e in envs.items()},
              "parent": "run" if args.parent_lib else "NOT RUN: no --parent-lib (the yardstick is this tree's mode-off leg)",
              "regions": args.regions, "configs": {}}
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    try:
        for name, (obs, feats, A, K, B, rel) in CONFIGS.items():
            try:
                steps = max(2, int(round(args.steps * rel)))
                ms = {leg: [] for leg in legs}
                for leg, p in legs.items():
                    ask(p, "region %s 3" % name)  # warm-up
                for _ in range(args.regions):
                    for leg, p in legs.items():
                        ms[leg].append(ask(p, "region %s %d" % (name, steps)))
                st = {leg: stat(v) for leg, v in ms.items()}
                y, yc = ("parent", "parent_conv") if "parent" in legs else ("off", "off_conv")
                row = {"obs": obs, "features": feats, "A": A, "K": K, "B": B, "steps_per_region": steps, "ms_per_step": st, "yardsticks": [y, yc],
                       "verdict_on": verdict(st["on"], st[y]), "verdict_off": verdict(st["off"], st[y]),
                       "verdict_on_conv": verdict(st["on_conv"], st[yc]), "verdict_off_conv": verdict(st["off_conv"], st[yc])}
                d0 = lambda t: [ln for ln in t if ln.startswith("k_imp_d0_fwd")]  # noqa: E731
                row["launches_on"], row["launches_off"] = ask(legs["on"], "table %s" % name), ask(legs["off"], "table %s" % name)
                row["d0_fwd_us_per_launch"] = {"off": d0(row["launches_off"]), "on": d0(row["launches_on"])}
                result["configs"][name] = row
                print(name, json.dumps(st), flush=True)
                print(name, "on:", row["verdict_on"], "| off:", row["verdict_off"], "| on_conv:", row["verdict_on_conv"], "| off_conv:", row["verdict_off_conv"], flush=True)
                print(name, "Dense_0 forward, us per launch:", row["d0_fwd_us_per_launch"], flush=True)
                if name == "workload":
                    act = {leg: ask(legs[leg], "act %d" % args.act_calls) for leg in ("off", "on")}
                    result["acting_workload"] = {**act, "verdict_act_host": verdict(act["on"]["act_host_us_per_call"], act["off"]["act_host_us_per_call"]),
                                                 "verdict_q_values_n32": verdict(act["on"]["q_values_n32_us_per_call"], act["off"]["q_values_n32_us_per_call"])}
                    print("acting", json.dumps(result["acting_workload"]), flush=True)
                for p in legs.values():
                    ask(p, "drop %s" % name)
            except Exception as e:  # (a leg that ended, e.g. out of memory at the large batch: what was measured so far is kept)
                result["configs"][name] = {"error": repr(e)}
                print(name, "FAILED:", repr(e), flush=True)
                break
    finally:
        for p in legs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
