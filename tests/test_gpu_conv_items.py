"""GPU: the conv launches that read their work item from a host-built table (csrc/convp_items.h).

Two small geometries where a wrong strip origin, column count or slot index in a descriptor shows at once -- the
``cnn_small`` golden frame (20x20: 5x5 -> 3x3 -> 3x3, items of a few positions that cross output rows) and a 36x28 frame
(9x7 -> 5x4 -> 5x4: not square, odd x even, four unequal parity variants in the Conv_1 data gradient), K = 2, B = 32:

* one step in both conv modes against the fp64 oracle: per-head loss within 1e-5, every stage within 2e-5 of the stage's
  largest entry (the bars of test_gpu_fp_path.py);
* the same step after the plan changed under the handle (B = 32, then 64, then 32 again: a table is built for the second
  plan, the first plan's table is reused) equals a fresh handle's bit for bit -- losses and the whole gradient arena.

The oracle reference of a geometry is computed once and shared by both modes.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import cnn_stages as S
from test_gpu_conv_geometry import GAMMA_N, LOSS_ATOL, STAGE_BAR, _agent, _inputs
from test_gpu_fp_path import conv_mode  # noqa: F401  (fixture: both conv arithmetic modes)

pytestmark = pytest.mark.gpu
Batch = namedtuple("Batch", "state action reward next_state is_terminal")
GEOMS = {"cnn_small": ((20, 20, 4), [32, 32, 32, 128], 5), "36x28": ((36, 28, 4), [32, 64, 64, 128], 4)}
K, B = 2, 32


@functools.lru_cache(maxsize=None)
def _reference(name):
    obs, feats, A = GEOMS[name]
    p, pt, batch = _inputs(obs, feats, A, K, 64)  # 64 samples: the first 32 are the step under test
    b32 = tuple(x[:B] for x in batch)
    return p, pt, batch, b32, S.oracle_heads(p, pt, b32, K, GAMMA_N)


@pytest.mark.parametrize("name", list(GEOMS))
def test_step_against_oracle(name, conv_mode):  # noqa: F811
    import torch

    from slimdqn import _hip

    obs, feats, A = GEOMS[name]
    p, pt, _, b32, heads = _reference(name)
    agent = _agent(obs, feats, A, K, p, pt)
    losses = agent._learn(Batch(*b32), flags=_hip.F_GRADS_ONLY).cpu().numpy()
    torch.cuda.synchronize()
    errs = S.stage_errors(agent, p, pt, b32, obs, feats, A, K, B, GAMMA_N, conv_mode, oracle=heads)
    S.print_stage_errors(errs)
    for k in range(K):
        print(f"head {k}: loss {losses[k]:.8f} oracle {heads[k][0]:.8f}")
    agent._destroy_handle()
    assert all(abs(losses[k] - heads[k][0]) <= LOSS_ATOL for k in range(K)), losses
    assert all(e < STAGE_BAR for e in errs.values()), errs


@pytest.mark.parametrize("name", list(GEOMS))
def test_plan_change_and_back_equals_a_fresh_handle(name, conv_mode):  # noqa: F811
    import torch

    from slimdqn import _hip

    obs, feats, A = GEOMS[name]
    p, pt, b64, b32, _ = _reference(name)

    def step(agent, batch):
        losses = agent._learn(Batch(*batch), flags=_hip.F_GRADS_ONLY).cpu().numpy().copy()
        torch.cuda.synchronize()
        return losses, agent._grad.cpu().numpy().copy()

    used = _agent(obs, feats, A, K, p, pt)
    used._ensure_handle(64)  # one handle for all three steps
    handle = used._handle.value
    first = step(used, b32)
    step(used, b64)
    again = step(used, b32)
    assert used._handle.value == handle
    used._destroy_handle()
    fresh = _agent(obs, feats, A, K, p, pt)
    fresh._ensure_handle(64)
    want = step(fresh, b32)
    fresh._destroy_handle()
    assert np.abs(want[1]).max() > 0
    for got in (first, again):
        assert got[0].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
