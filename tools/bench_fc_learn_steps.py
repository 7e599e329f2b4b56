"""What a gradient step costs when n of them are issued together (``idqn_learn_steps_on_replay_fc``, csrc/fc_steps_kernels.h).

  lunar       fc, obs 8, [100, 100], A = 4, K = 3, B = 32 (the LunarLander experiment)   persistent kernel k_fc_steps_par
  fc_520      fc, obs 8, [520], A = 4, K = 3, B = 32                                     outside the one-launch plan: loop route
  gcnn_smoke  cnn, (84, 84, 4), [2, 3, 1, 15], A = 6, K = 1, B = 32                      general-shape cnn: loop route

Legs, per config and n in {1, 2, 5, 10, 32}, all on the same slots, ring and handle state:
  (a) python_loop   n ``idqn_learn_on_replay_fc`` calls from Python (the route of the parent commit)
  (b) c_loop        one ``idqn_learn_steps_on_replay_fc`` call forced onto the loop route (``IDQN_FC_LEARN_STEPS_LOOP=1``)
  (c) persistent    the same call on its own route (the persistent kernel where the handle has one; else the loop again)
A region is ``--calls`` groups of n steps, timed on the host clock with a device synchronisation at both ends; regions of the
three legs alternate, ``--rounds`` times.  Reported: microseconds per gradient step, median [min, max] over the rounds;
``faster`` names a leg of a pair only where the intervals do not overlap.  Writes ``profiles/fc_learn_steps.json``.
Usage: ``python tools/bench_fc_learn_steps.py [--rounds 7] [--calls 40] [--out profiles/fc_learn_steps.json]``.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
CONFIGS = {  # name: (arch, frame shape, dtype, stack, obs, A, K, features)
    "lunar": ("fc", (8,), "float32", 1, 8, 4, 3, [100, 100]),
    "fc_520": ("fc", (8,), "float32", 1, 8, 4, 3, [520]),
    "gcnn_smoke": ("cnn", (84, 84), "uint8", 4, (84, 84, 4), 6, 1, [2, 3, 1, 15]),
}
B, NS = 32, (1, 2, 5, 10, 32)


def _stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def _faster(x, y, nx, ny):
    return nx if x["max"] < y["min"] else ny if y["max"] < x["min"] else None


def bench(name, calls, rounds):
    import numpy as np
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN
    from slimdqn.sample_collection.replay_buffer import ReplayBuffer, TransitionElement
    from slimdqn.sample_collection.samplers import UniformSamplingDistribution

    arch, shape, dtype, stack, obs, A, K, feats = CONFIGS[name]
    rb = ReplayBuffer(UniformSamplingDistribution(0), batch_size=B, max_capacity=2000, stack_size=stack, update_horizon=1, gamma=0.99)
    rng = np.random.default_rng(1)
    for i in range(2500):
        frame = rng.integers(0, 256, shape, dtype=np.uint8) if dtype == "uint8" else rng.standard_normal(shape).astype(np.float32)
        rb.add(TransitionElement(frame, int(rng.integers(A)), float(rng.normal()), i % 200 == 199, i % 200 == 199))
    agent = iDQN(0, obs, A, K, feats, arch, 3e-4, 0.99, 1, 1, 10**9, 10**9)
    agent._ensure_handle(B)
    frames, n_frames, frame_bytes, rows, stk = rb.ring_view()[:5]
    lib, h, q = _hip.lib(), agent._handle, _hip.current_stream()
    ring = (_hip.ptr(frames), int(n_frames), int(frame_bytes), _hip.ptr(rows))
    out = {}
    for n in NS:
        slots = np.stack([np.ascontiguousarray(rb.sample_slots(), np.int32) for _ in range(n)])

        def python_loop():
            for i in range(n):
                _hip.check(lib.idqn_learn_on_replay_fc(h, *ring, slots[i].ctypes.data, B, int(stk), B, 0, q), "single")

        def many():
            _hip.check(lib.idqn_learn_steps_on_replay_fc(h, *ring, slots.ctypes.data, n, B, int(stk), B, 0, q), "many")

        def region(fn, force_loop):
            os.environ["IDQN_FC_LEARN_STEPS_LOOP"] = "1" if force_loop else "0"
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / (calls * n)

        legs = {"python_loop": (python_loop, False), "c_loop": (many, True), "persistent": (many, False)}
        times = {k: [] for k in legs}
        for _ in range(rounds):
            for k, (fn, force) in legs.items():
                times[k].append(region(fn, force))
        st = {k: _stat(v) for k, v in times.items()}
        st["faster_c_loop_vs_python_loop"] = _faster(st["c_loop"], st["python_loop"], "c_loop", "python_loop")
        st["faster_persistent_vs_c_loop"] = _faster(st["persistent"], st["c_loop"], "persistent", "c_loop")
        out[str(n)] = st
        print(name, n, {k: (round(v["median"], 2), round(v["min"], 2), round(v["max"], 2)) for k, v in st.items() if isinstance(v, dict)},
              flush=True)
    os.environ.pop("IDQN_FC_LEARN_STEPS_LOOP", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_learn_steps.json"))
    args = ap.parse_args()
    res = {"unit": "microseconds per gradient step, host clock, device synchronised at both ends of a region",
           "rounds": args.rounds, "calls_per_region": args.calls, "batch": B, "configs": {}}
    for name in args.configs.split(","):
        res["configs"][name] = bench(name, args.calls, args.rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
