"""What greedy i-IQN actions for E host states cost: ONE ``idqn_iqn_act_host_many`` call (csrc/iqn_act_many_kernels.h)
against a loop of E ``idqn_iqn_act_host`` calls -- what the parent commit offers -- on the same handle in the same process,
Atari shape (84 x 84 x 4, [32, 64, 64, 512], A = 6), K = 5, N in {32, 64}, E in {1, 2, 4, 8, 16, 32}, two head patterns:

  one_head   every state on head 0 (the Dense_0 kernel of one head is streamed once per chunk of states);
  drawn      heads drawn uniformly (seeded) -- 16 assignments per E, used in turn by both sides.

Both sides go through the C ABI with states and fractions already in pinned memory and end with the actions on the host
(both calls block), so the host clock around a call is the whole cost.  Regions of ``--calls`` calls alternate between the
two sides, ``--rounds`` times; a side's figure is the median over its regions of the region's median call, the spread the
range of the region medians relative to that figure.  Every (N, E, pattern) first checks that both sides return the same
actions.  Writes ``profiles/iiqn_act_many.json``: us per call and per action for both legs, their spreads, loop / many, and
``faster_beyond_spread``: whether loop / many of the two medians exceeds 1 + the call's spread + the loop's spread.
Usage: ``python tools/bench_iqn_act_many.py [--out profiles/iiqn_act_many.json] [--rounds 5] [--calls 100]``.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "i-dqn_amd")]
OBS, A, FEATS, K = (84, 84, 4), 6, [32, 64, 64, 512], 5
QUANTILES, SIZES, DRAWS = (32, 64), (1, 2, 4, 8, 16, 32), 16


def measure(N, a, np, torch, _hip):
    from slimdqn.networks.iiqn import iIQN

    agent = iIQN(0, OBS, A, K, FEATS, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4, n_quantiles=N)
    agent._ensure_handle(32)
    lib, h, stream = _hip.lib(), agent._handle, _hip.current_stream()
    rng = np.random.default_rng(N)
    n_bytes = int(np.prod(OBS))
    pin = torch.from_numpy(rng.integers(0, 256, size=(32, n_bytes), dtype=np.uint8)).pin_memory()
    tau = torch.from_numpy(rng.random((32, N)).astype(np.float32)).pin_memory()
    state_ptr = [C.c_void_p(pin.data_ptr() + e * n_bytes) for e in range(32)]
    tau_ptr = [C.c_void_p(tau.data_ptr() + 4 * N * e) for e in range(32)]
    q_out = torch.zeros((32, A), dtype=torch.float32, device="cuda")
    acts_many, acts_loop = torch.zeros(32, dtype=torch.int32).pin_memory(), torch.zeros(32, dtype=torch.int32).pin_memory()
    many_np, loop_np = acts_many.numpy(), acts_loop.numpy()
    q_ptr, many_ptr = _hip.ptr(q_out), C.c_void_p(acts_many.data_ptr())
    loop_ptr = [C.c_void_p(acts_loop.data_ptr() + 4 * e) for e in range(32)]

    def many(heads):
        rc = lib.idqn_iqn_act_host_many(h, 0, heads.ctypes.data, state_ptr[0], tau_ptr[0], heads.size, q_ptr, many_ptr, stream)
        if rc:
            _hip.check(rc, "idqn_iqn_act_host_many")

    def loop(heads):
        for e in range(heads.size):
            rc = lib.idqn_iqn_act_host(h, 0, int(heads[e]), state_ptr[e], tau_ptr[e], q_ptr, loop_ptr[e], stream)
            if rc:
                _hip.check(rc, "idqn_iqn_act_host")

    def region(fn, draws):
        ts = []
        for i in range(a.calls):
            heads = draws[i % len(draws)]
            t0 = time.perf_counter()
            fn(heads)
            ts.append(time.perf_counter() - t0)
        return 1e6 * float(np.median(ts))

    res = {"one_head": {}, "drawn": {}}
    for pattern in ("one_head", "drawn"):
        for E in SIZES:
            if pattern == "one_head":
                draws = [np.zeros(E, np.int32)]
            else:
                draws = [np.ascontiguousarray(rng.integers(0, K, size=E), np.int32) for _ in range(DRAWS)]
            for heads in draws:  # warm-up of every graph either side replays, and the same answers from both
                for _ in range(3):
                    many(heads)
                    loop(heads)
                assert (many_np[:E] == loop_np[:E]).all(), (N, pattern, E, heads, many_np[:E], loop_np[:E])
            reg = {"many": [], "loop": []}
            for _ in range(a.rounds):
                reg["many"].append(region(many, draws))
                reg["loop"].append(region(loop, draws))
            m, l = float(np.median(reg["many"])), float(np.median(reg["loop"]))
            sm, sl = (max(reg["many"]) - min(reg["many"])) / m, (max(reg["loop"]) - min(reg["loop"])) / l
            res[pattern][str(E)] = {
                "distinct_heads_mean": float(np.mean([np.unique(d).size for d in draws])),
                "many_us_per_call": m, "many_us_per_action": m / E, "many_regions": reg["many"], "many_spread": sm,
                "loop_us_per_call": l, "loop_us_per_action": l / E, "loop_regions": reg["loop"], "loop_spread": sl,
                "loop_over_many": l / m, "faster_beyond_spread": bool(l / m > 1.0 + sm + sl)}
            print(json.dumps({"N": N, "pattern": pattern, "E": E, "many_us": round(m, 1), "loop_us": round(l, 1),
                              "loop_over_many": round(l / m, 2), "spread_many": round(sm, 3), "spread_loop": round(sl, 3)}), flush=True)
    agent._destroy_handle()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iiqn_act_many.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    import numpy as np
    import torch

    from slimdqn import _hip

    res = {"config": {"obs": OBS, "features": FEATS, "A": A, "K": K, "rounds": a.rounds, "calls": a.calls, "draws": DRAWS,
                      "states_per_chunk": _hip.IQN_ACT_MANY_SC, "device": torch.cuda.get_device_name(0)}}
    for N in QUANTILES:
        res[f"N{N}"] = measure(N, a, np, torch, _hip)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
