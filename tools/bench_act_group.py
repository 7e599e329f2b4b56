"""What the greedy actions of S Atari-shaped agents cost in one process: ONE ``idqn_act_group_host`` call (csrc/act_many_kernels.h,
the group instantiations) against what ``AgentGroup.best_actions`` runs without it, on the same handles in the same process, Atari
shape (84 x 84 x 4, [32, 64, 64, 512], A = 6), K = 5, heads drawn uniformly (seeded; 16 assignments per size, used in turn by
both sides):

  one state per member, S in {1, 2, 4, 8, 16, 32}:  the group call  vs  the loop of S ``idqn_act_host`` calls;
  S x E in {4 x 8, 8 x 4} (a vector step):          the group call  vs  S calls of ``idqn_act_host_many`` (E states each).

Both sides go through the C ABI with the states already in pinned memory and end with the actions on the host (every call
blocks), so the host clock around a call is the whole cost.  Regions of ``--calls`` calls alternate between the two sides,
``--rounds`` (7) times; a side's figure is the median [min, max] over its regions of the region's median call.  Every size first
checks that both sides return the same actions.  The standing rule: a size is ON (``AgentGroup.act_group_sizes``) where the
group call's median lies below the other side's minimum; a size at which the call is slower is reported as SLOWER.  Writes
``profiles/act_group.json``.
Usage: ``python tools/bench_act_group.py [--out profiles/act_group.json] [--rounds 7] [--calls 200] [--sizes 1,2,4,8,16,32]``.
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
DRAWS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_group.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--vector", default="4x8,8x4")
    a = ap.parse_args()
    import numpy as np
    import torch

    from slimdqn import _hip
    from slimdqn.networks.idqn import iDQN

    sizes = [int(s) for s in a.sizes.split(",") if s]
    vector = [tuple(int(x) for x in v.split("x")) for v in a.vector.split(",") if v]
    n_agents = max(sizes + [s for s, _ in vector])
    agents = [iDQN(g, OBS, A, K, FEATS, "cnn", 6.25e-5, 0.99, 1, 1, 10**9, 10**9, adam_eps=1.5e-4) for g in range(n_agents)]
    for ag in agents:
        ag._ensure_handle(32)
    lib, stream = _hip.lib(), _hip.current_stream()
    rng = np.random.default_rng(0)
    n_bytes = int(np.prod(OBS))
    pin = torch.from_numpy(rng.integers(0, 256, size=(32, n_bytes), dtype=np.uint8)).pin_memory()
    state_ptr = [C.c_void_p(pin.data_ptr() + e * n_bytes) for e in range(32)]
    q_out = torch.zeros((32, A), dtype=torch.float32, device="cuda")
    acts_group, acts_other = torch.zeros(32, dtype=torch.int32).pin_memory(), torch.zeros(32, dtype=torch.int32).pin_memory()
    group_np, other_np = acts_group.numpy(), acts_other.numpy()
    q_ptr, group_ptr = _hip.ptr(q_out), C.c_void_p(acts_group.data_ptr())
    q_row = [C.c_void_p(q_out.data_ptr() + 4 * A * e) for e in range(32)]
    other_ptr = [C.c_void_p(acts_other.data_ptr() + 4 * e) for e in range(32)]

    def make_group(S):
        handles = (C.c_void_p * S)(*[ag._handle.value for ag in agents[:S]])
        g = C.c_void_p()
        _hip.check(lib.idqn_act_group_create(handles, S, C.byref(g)), "idqn_act_group_create")
        return g

    def measure(S, E):
        n = S * E
        members = np.ascontiguousarray(np.repeat(np.arange(S), E), np.int32)
        draws = [np.ascontiguousarray(rng.integers(0, K, size=n), np.int32) for _ in range(DRAWS)]
        g = make_group(S)
        handles = [ag._handle for ag in agents[:S]]

        def group(heads):
            rc = lib.idqn_act_group_host(g, 0, members.ctypes.data, heads.ctypes.data, state_ptr[0], n, q_ptr, group_ptr, stream)
            if rc:
                _hip.check(rc, "idqn_act_group_host")

        if E == 1:
            def other(heads):  # what AgentGroup.best_actions runs without the route
                for e in range(S):
                    rc = lib.idqn_act_host(handles[e], 0, int(heads[e]), state_ptr[e], q_ptr, other_ptr[e], stream)
                    if rc:
                        _hip.check(rc, "idqn_act_host")
        else:
            # (the address of every seed's E heads in every draw, worked out once: nothing but the S calls is timed)
            head_ptr = {id(d): [d.ctypes.data + 4 * s * E for s in range(S)] for d in draws}

            def other(heads):  # what SeedVectorTrainer runs without the route: every seed's own many-state call
                ptrs = head_ptr[id(heads)]
                for s in range(S):
                    rc = lib.idqn_act_host_many(handles[s], 0, ptrs[s], state_ptr[s * E], E, q_row[s * E], other_ptr[s * E], stream)
                    if rc:
                        _hip.check(rc, "idqn_act_host_many")

        def region(fn):
            ts = []
            for i in range(a.calls):
                heads = draws[i % len(draws)]
                t0 = time.perf_counter()
                fn(heads)
                ts.append(time.perf_counter() - t0)
            return 1e6 * float(np.median(ts))

        for heads in draws:  # warm-up of every graph either side replays, and the same answers from both
            for _ in range(2):
                group(heads)
                other(heads)
            assert (group_np[:n] == other_np[:n]).all(), (S, E, heads, group_np[:n], other_np[:n])
        reg = {"group": [], "other": []}
        for _ in range(a.rounds):
            reg["group"].append(region(group))
            reg["other"].append(region(other))
        lib.idqn_act_group_destroy(g)
        gm, om = float(np.median(reg["group"])), float(np.median(reg["other"]))
        verdict = "ON" if gm < min(reg["other"]) else ("SLOWER" if gm > om else "off (inside the other side's spread)")
        row = {"S": S, "E": E, "states": n, "other": "loop of idqn_act_host" if E == 1 else "S calls of idqn_act_host_many",
               "group_us_per_call": gm, "group_min_max": [min(reg["group"]), max(reg["group"])], "group_regions": reg["group"],
               "other_us_per_call": om, "other_min_max": [min(reg["other"]), max(reg["other"])], "other_regions": reg["other"],
               "other_over_group": om / gm, "verdict": verdict}
        print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("_regions")}), flush=True)
        return row

    res = {"config": {"obs": OBS, "features": FEATS, "A": A, "K": K, "rounds": a.rounds, "calls": a.calls, "draws": DRAWS,
                      "device": torch.cuda.get_device_name(0)},
           "one_state_per_member": {str(S): measure(S, 1) for S in sizes},
           "vector": {f"{S}x{E}": measure(S, E) for S, E in vector}}
    res["act_group_sizes"] = sorted(int(S) for S, r in res["one_state_per_member"].items() if r["verdict"] == "ON")
    print(json.dumps({"act_group_sizes": res["act_group_sizes"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
