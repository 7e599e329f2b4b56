"""Host-side checks of vectorised acting: ``idqn_act_host_many`` is declared in the header, exported by the built library
and bound in ``_hip`` (the ABI version stays 4: an entry was added, none changed), and ``select_actions`` over E environments
is ``select_action`` per environment -- same actions, same keys handed on, ONE ``best_actions`` call for all the greedy ones.
No GPU needed; the device side is ``tests/test_gpu_act_many.py``."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_bound():
    from slimdqn import _hip

    name = "idqn_act_host_many"
    assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
    assert len(_hip.SYMBOLS[name][1]) == 8
    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
    assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
    assert lib.idqn_abi_version() == 4


class _StubAgent:
    """``best_action`` / ``best_actions`` of a made-up agent: the action is a hash of the state and the key, the calls are recorded."""

    def __init__(self, n_actions):
        self.A, self.single, self.many = n_actions, [], []

    def _act(self, state, key):
        from slimdqn import prng

        return (prng.randint(key, 0, 1 << 20) + 7 * int(state)) % self.A

    def best_action(self, params, state, key):
        from slimdqn.sample_collection.utils import HostAction

        self.single.append((state, key))
        return HostAction(self._act(state, key))

    def best_actions(self, params, states, keys):
        self.many.append((list(states), list(keys)))
        return [self._act(s, k) for s, k in zip(states, keys)]


@pytest.mark.parametrize("epsilon", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("E", [1, 5, 32])
def test_select_actions_is_select_action_per_environment(E, epsilon):
    from slimdqn import prng
    from slimdqn.sample_collection.utils import select_action, select_actions

    A = 6
    keys = prng.split(prng.PRNGKey(1234 + E), E)  # a fixed seed: at epsilon = 0.5 both branches occur for E > 1
    states = list(range(100, 100 + E))
    a, b = _StubAgent(A), _StubAgent(A)
    want = [select_action(a.best_action, None, states[i], keys[i], A, lambda n: epsilon, 17).item() for i in range(E)]
    got = select_actions(b.best_actions, None, states, keys, A, lambda n: epsilon, 17)
    assert list(got) == want and all(isinstance(x, int) for x in got)
    n_greedy = len(a.single)
    if epsilon == 0.0:
        assert n_greedy == E
    if epsilon == 1.0:
        assert n_greedy == 0
    if epsilon == 0.5 and E > 1:
        assert 0 < n_greedy < E
    # one call for all the greedy environments, none when every environment explores; the states and keys it is handed
    # are the ones select_action hands to best_action, in environment order
    assert len(b.many) == (1 if n_greedy else 0)
    assert not b.single
    if n_greedy:
        assert b.many[0][0] == [s for s, _ in a.single]
        assert b.many[0][1] == [k for _, k in a.single]
