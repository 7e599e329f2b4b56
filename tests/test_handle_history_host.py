"""The handle-history harness (tests/handle_history.py) on two numpy stubs, no library and no GPU: a history-free agent passes,
an agent that keeps ONE stale pad lane of the previous batch when B shrinks fails -- and the message names the op and the op
in front of it.  The harness that guards the kernels (tests/test_gpu_handle_history.py) can fail, and says where."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

import handle_history as H


class StubAgent:
    """A 'network' of two heads with a 32-lane-per-block workspace that lives as long as the handle, like the library's scratch."""

    leaky = False

    def __init__(self):
        K, P = 2, 12
        self._K, self._P, self._arch, self._obs = K, P, "fc", (4, 1, 1)
        self.network = SimpleNamespace(n_actions=3)
        self._leaves = [("Dense_0/kernel", 0, (4, 2)), ("Dense_0/bias", 8, (2,)), ("Dense_1/bias", 10, (2,))]
        self._online = np.linspace(-1.0, 1.0, K * P, dtype=np.float32).reshape(K, P)
        self._target = self._online.copy()
        self._mu, self._nu = np.zeros((K, P), np.float32), np.zeros((K, P), np.float32)
        self._count, self._cum = np.zeros(K, np.int32), np.zeros(K, np.float64)
        self._handle = self._ws = None
        self.created = 0

    def _ensure_handle(self, batch):
        if self._handle is None or batch > self._ws.size:
            self._handle, self._ws = object(), np.zeros(-(-max(batch, 32) // 32) * 32, np.float32)  # zeroed once, at creation
            self.created += 1

    def _destroy_handle(self):
        self._handle = None

    def _learn(self, batch, flags=0):
        B = len(batch.action)
        self._ensure_handle(B)
        lanes = -(-B // 32) * 32
        per_sample = batch.reward + np.asarray(batch.state, np.float32).reshape(B, -1).sum(1)
        stale = self._ws[B] if B < lanes else 0.0
        self._ws[:B] = per_sample
        self._ws[B:lanes] = 0.0  # the pad lanes of the ragged block are masked ...
        if self.leaky and B < lanes:
            self._ws[B] = stale  # ... except one, which keeps what the previous batch left there
        g = np.float32(self._ws[:lanes].sum() / B)
        losses = (g * g * np.arange(1, self._K + 1)).astype(np.float32)
        self._mu += np.float32(0.1) * (g - self._mu)
        self._nu += np.float32(0.001) * (g * g - self._nu)
        self._online -= np.float32(1e-3) * self._mu / (np.sqrt(self._nu) + np.float32(1e-6))
        self._count += 1
        self._cum += losses
        return losses

    def _local_target_update(self):
        self._target[...] = self._online
        self._online[:-1] = self._online[1:].copy()

    def _local_target_sync(self):
        self._target[1:] = self._online[:-1]


class LeakyStubAgent(StubAgent):
    leaky = True


SCRIPT = [H.learn(70, 1), H.learn(64, 2), H.learn(20, 3), H.target_update(), H.learn(32, 4), H.target_sync(), H.learn(33, 5),
          H.learn(7, 6)]


def test_history_free_stub_passes():
    made = []

    def make():
        made.append(StubAgent())
        return made[-1]

    assert H.run_script(make, 70, SCRIPT) == len(SCRIPT)
    assert len(made) == 1 + len(SCRIPT)  # the used agent and one fresh agent per op
    assert all(a.created == 1 and a._handle is None for a in made)  # one handle each, every one destroyed


def test_stale_pad_lane_is_caught_and_named():
    with pytest.raises(AssertionError) as e:
        H.run_script(LeakyStubAgent, 70, SCRIPT)
    msg = str(e.value)
    # B = 64 fills both blocks; B = 20 leaves lane 20 of the first block holding sample 20 of that batch
    assert msg.startswith("op 2 learn(B=20, seed=3, flags=0) after learn(B=64, seed=2, flags=0): "), msg
    assert re.search(r"differs between the used and the fresh handle in \d+ of \d+ elements, first at flat index \d+", msg), msg
    assert "losses" in msg or "head 0, Dense_0/kernel[0]" in msg, msg


def test_the_batch_in_front_of_a_ragged_one_is_boosted():
    """Rewards x 1000 and no terminals in the minibatch that precedes a ragged B, acting and target ops in between or not."""
    script = [H.learn(64, 1), H.q_values(0, 0, 5, 2), H.learn(20, 3), H.learn(32, 4), H.target_sync(), H.weighted_learn(33, 5),
              H.learn_on_replay(32, 6), H.learn(7, 7), H.learn(64, 8)]
    # ragged: ops 2 (B = 20), 5 (33) and 7 (7); in front of them ops 0, 3 and 6 -- and op 6 draws its batch from the replay
    # buffer: nothing of the harness's to scale
    assert H._boosted(script) == {0, 3}
    agent = StubAgent()
    plain = H._prepare(agent, script[0], False, {})["batch"]
    big = H._prepare(agent, script[0], True, {})["batch"]
    assert np.array_equal(big.reward, plain.reward * np.float32(1000.0)) and not big.is_terminal.any()
    assert np.array_equal(big.state, plain.state) and np.array_equal(big.action, plain.action)
    assert np.abs(big.reward).max() == 1000.0


def test_a_script_that_does_not_move_the_state_is_refused():
    class Frozen(StubAgent):
        def _learn(self, batch, flags=0):
            return np.zeros(self._K, np.float32)

    with pytest.raises(AssertionError, match="does not move the parameters"):
        H.run_script(Frozen, 32, [H.learn(32, 1)])


def test_a_rebuilt_handle_is_refused():
    with pytest.raises(AssertionError, match="exceeds max_batch 32"):
        H.run_script(StubAgent, 32, [H.learn(70, 1)])  # nothing in a script may exceed max_batch

    class Rebuilds(StubAgent):
        def _learn(self, batch, flags=0):
            self._handle = object()
            return super()._learn(batch, flags)

    with pytest.raises(AssertionError, match="rebuilt the used handle"):
        H.run_script(Rebuilds, 32, [H.learn(32, 1)])
