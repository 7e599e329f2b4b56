"""Host-side checks of vectorised i-IQN acting: ``idqn_iqn_act_host_many`` is declared in the header, exported by the built
library and bound in ``_hip`` (the ABI version stays 4: an entry was added, none changed), and ``iIQN.best_actions`` on a
stub agent with no device draws each head and each fraction row from its key exactly as ``best_action`` does, stages them
for ONE C call (replaced here by a recording stub) and leaves ``_tau_rng`` alone.  No GPU needed; the device side is
``tests/test_gpu_iqn_act_many.py``."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "idqn_iqn_act_host_many"


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    assert NAME in _hip.SYMBOLS, f"{NAME} is not bound in slimdqn/_hip.py"
    # idqn_act_host_many's arguments plus the pinned fractions
    assert len(_hip.SYMBOLS[NAME][1]) == len(_hip.SYMBOLS["idqn_act_host_many"][1]) + 1 == 9
    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), f"{NAME} is not declared in include/idqn_hip.h"
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+" + NAME + r"$", exported, re.M), f"{NAME} is not exported by the library"
    assert getattr(lib, NAME).argtypes == _hip.SYMBOLS[NAME][1]
    assert lib.idqn_abi_version() == 4
    # the chunk size the binding states is the header's
    kernels = open(os.path.join(ROOT, "i-dqn_amd", "csrc", "iqn_act_many_kernels.h")).read()
    assert int(re.search(r"^#define IQN_ACT_MANY_SC (\d+)", kernels, re.M).group(1)) == _hip.IQN_ACT_MANY_SC


K, N, A, OBS = 3, 5, 4, (6, 6, 4)


def _stub_agent():
    """An iIQN that never touched a device: the attributes ``best_actions`` reads, ordinary host tensors for the staging
    blocks, and a recording stub in place of the C call (it answers with action i = head i)."""
    import torch

    from slimdqn.networks.iiqn import iIQN

    agent = iIQN.__new__(iIQN)
    agent.n_networks, agent._K, agent._n_quantiles, agent._obs = K, K, N, OBS
    agent.params, agent.target_params = object(), object()
    agent._tau_rng = np.random.Generator(np.random.PCG64(7))
    agent._ensure_handle = lambda batch: None
    size = int(np.prod(OBS))
    agent._iacts_pin = torch.zeros((32, size), dtype=torch.uint8)
    agent._iacts_pin_np = agent._iacts_pin.numpy()
    agent._iacts_tau_pin = torch.zeros((32, N), dtype=torch.float32)
    agent._iacts_tau_np = agent._iacts_tau_pin.numpy()
    agent._iacts_out = torch.zeros(32, dtype=torch.int32)
    agent._iacts_out_np = agent._iacts_out.numpy()
    agent.calls = []

    def call(which, heads, n):
        agent.calls.append((which, heads.copy(), n, agent._iacts_pin_np[:n].copy(), agent._iacts_tau_np[:n].copy()))
        agent._iacts_out_np[:n] = heads
        return 0

    agent._iqn_act_many_call = call
    return agent


def test_best_actions_draws_heads_and_fractions_from_the_keys():
    from slimdqn import prng

    agent = _stub_agent()
    rng = np.random.default_rng(3)
    keys = prng.split(prng.PRNGKey(77), 9)
    states = [rng.integers(0, 256, OBS, dtype=np.uint8) for _ in keys]
    want_heads = [prng.randint(k, 0, K) for k in keys]
    assert len(set(want_heads)) == K
    before = json.dumps(agent._tau_rng.bit_generator.state, default=str)
    for params, which in ((agent.params, 0), (agent.target_params, 1)):
        agent.calls.clear()
        got = agent.best_actions(params, states, keys)
        assert len(agent.calls) == 1, "best_actions issues ONE C call"
        w, heads, n, staged, taus = agent.calls[0]
        assert (w, n) == (which, 9) and heads.dtype == np.int32 and heads.tolist() == want_heads
        assert got.dtype == np.int64 and got.tolist() == want_heads  # (the stub's actions)
        for i, k in enumerate(keys):
            # what _act_host draws for this key
            want = prng.generator(prng.split(k, 2)[1]).random((N, 1)).astype(np.float32)
            assert taus[i].tobytes() == want[:, 0].tobytes()
            assert staged[i].tobytes() == states[i].tobytes()
    assert agent._iqn_act_many_ok is True
    assert json.dumps(agent._tau_rng.bit_generator.state, default=str) == before  # keyed acting leaves the training stream alone
    # fractions handed in override the draw
    given = rng.random((2, N)).astype(np.float32)
    agent.calls.clear()
    agent.best_actions(agent.params, states[:2], keys[:2], taus=given)
    assert agent.calls[0][4].tobytes() == given.tobytes()


def test_best_actions_refuses_bad_input():
    from slimdqn import prng

    agent = _stub_agent()
    keys = prng.split(prng.PRNGKey(5), 33)
    states = [np.zeros(OBS, np.uint8)] * 33
    for s, k in ((states[:0], keys[:0]), (states, keys), (states[:3], keys[:2]), (states[:2], keys[:3])):
        with pytest.raises(ValueError):
            agent.best_actions(agent.params, s, k)
    assert not agent.calls
