"""Host-side checks of the single-state i-IQN acting path: ``idqn_iqn_act_host`` and ``idqn_iqn_act_host_begin`` are
declared in the header, exported by the built library and bound in ``_hip``; the ABI version stays 4 (entries added
only).  No GPU needed; the device side is ``tests/test_gpu_iqn_acting.py``."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("idqn_iqn_act_host", "idqn_iqn_act_host_begin")


def test_acting_entries_are_declared_exported_and_bound():
    from slimdqn import _hip

    header = open(os.path.join(ROOT, "include", "idqn_hip.h")).read()
    lib = _hip.lib()
    nm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    exported = subprocess.run([nm if os.path.exists(nm) else "nm", "-D", "--defined-only", _hip.LIB_PATH], check=True,
                              capture_output=True, text=True).stdout
    for name in NEW_ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, re.M), f"{name} is not declared in include/idqn_hip.h"
        assert name in _hip.SYMBOLS, f"{name} is not bound in slimdqn/_hip.py"
        assert re.search(r"\sT\s+" + name + r"$", exported, re.M), f"{name} is not exported by the library"
        assert getattr(lib, name).argtypes == _hip.SYMBOLS[name][1]
        # idqn_act_host's arguments plus the pinned fractions
        assert len(_hip.SYMBOLS[name][1]) == len(_hip.SYMBOLS["idqn_act_host"][1]) + 1
    assert lib.idqn_abi_version() == 4
