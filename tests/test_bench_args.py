"""CPU: bench.py's option contract, checked before anything touches torch or a GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_full_and_dump_outputs_are_options():
    out = _run("--help")
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_is_refused_outside_the_i_dqn_step(tmp_path):
    for mode in (("--algo", "iiqn"), ("--learner",), ("--emulate-ranks", "2"), ("--heads", "1,2")):
        out = _run(*mode, "--dump-outputs", str(tmp_path / "out"))
        assert out.returncode == 2 and "--dump-outputs" in out.stderr, (mode, out.stderr[-500:])
        assert not os.path.exists(tmp_path / "out")
