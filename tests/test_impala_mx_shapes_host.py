"""Host side of the impala matrix-core conv mode (no GPU): the coverage conditions of tests/impala_mx_shapes.py, its
restatement of the eligibility rule and the launch plan against csrc/imp_mx_args.h (through tools/probes/imp_mx_args_probe.cpp),
the exact three-term bf16 split, and the condition that makes the device comparison meaningful -- on every row, both the
vector-ALU kernel's blocked float32 sum and the matrix-core kernel's select the same element of every pool window as the
fp64 oracle does."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import impala_mx_shapes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dqn_amd", "csrc")


def _cxx():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)


def test_table_covers_what_the_kernel_can_get_wrong():
    rows = {n: (obs, feats, M.conv_layers(obs, feats), set(M.mx_layers(obs, feats))) for n, (obs, feats, A, K, B) in M.ROWS.items()}
    for n, (obs, feats, A, K, B) in M.ROWS.items():
        if n != "workload":
            assert obs[0] <= 33 and obs[1] <= 33 and K <= 2 and B <= 5, n
    # every conv but the uint8 one eligible
    assert len(rows["all_mx"][3]) == 14 and (0, 0) not in rows["all_mx"][3]
    # mixed nets, in both orders; a width of 32 + 1
    order = lambda n: "".join("m" if (s, i) in rows[n][3] else "v" for s, i, *_ in rows[n][2])  # noqa: E731
    assert re.fullmatch(r"v+m+", order("mixed_valu_mx")) and order("mixed_valu_mx").startswith("vvvvvm")
    assert re.fullmatch(r"vm+v+m+", order("mixed_mx_valu"))
    assert 33 in M.ROWS["mixed_mx_valu"][1]
    mx = [(ci, co, h, w) for obs, feats, layers, on in rows.values() for s, i, ci, co, h, w in layers if (s, i) in on]
    assert {16, 32, 64} <= {ci for ci, *_ in mx}          # one k-step, two, the workload's largest
    assert {32, 64} <= {co for _, co, *_ in mx}           # one and two N tiles
    assert any(ci == 16 and co == 32 for ci, co, *_ in mx)  # the data gradient of this one writes half an N tile
    frames = {(h, w) for *_, h, w in mx}
    assert {(16, 16), (17, 17), (15, 15)} <= frames       # exactly the tile, one row and one column more, one less
    assert any(h == 1 for h, w in frames)
    # both SAME pad classes of the pool (even / odd extent) at every Stack, on both axes
    for s in range(3):
        ext = [(h, w) for obs, feats, layers, on in rows.values() for ss, i, ci, co, h, w in layers if ss == s and i == 0]
        assert {h % 2 for h, w in ext} == {0, 1} and {w % 2 for h, w in ext} == {0, 1}, s
    assert M.ROWS["workload"] == ((84, 84, 4), [32, 64, 64, 512], 6, 2, 2)
    fwd, bwd = M.expected_launches(*M.ROWS["workload"][:2])
    assert sum("_mx" in n for n in fwd) == 14 and sum("_mx" in n for n in bwd) == 14 and fwd[0] == "k_imp_conv<u8>"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("probe") / "imp_mx_args_probe"
    subprocess.run([cc, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tools", "probes", "imp_mx_args_probe.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_probe_reports_no_failures_and_the_constants(probe):
    out = subprocess.run([probe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "constants %d %d %d %d" % (M.TH, M.TW, M.KC, M.NB)
    m = re.search(r"^ok: (\d+) checks, 0 failures$", lines[-1])
    assert m and int(m.group(1)) > 1000, out.stdout[-500:]


def test_eligibility_restatement_equals_the_host_function(probe):
    pairs = [(ci, co) for ci in (0, 1, 4, 15, 16, 17, 31, 32, 33, 48, 64, 96) for co in (0, 1, 16, 31, 32, 33, 48, 64, 96, 512)]
    pairs += [(ci, co) for obs, feats, *_ in M.ROWS.values() for _, _, ci, co, _, _ in M.conv_layers(obs, feats)]
    got = subprocess.run([probe] + [str(v) for p in pairs for v in p], check=True, capture_output=True, text=True).stdout.split()
    assert [int(g) for g in got] == [int(M.eligible(ci, co)) for ci, co in pairs]
    for h, w, co, n in ((16, 16, 32, 4), (17, 17, 64, 3), (15, 15, 16, 1), (1, 10, 32, 4), (42, 42, 64, 20), (11, 11, 33, 2)):
        got = subprocess.run([probe, "plan", str(h), str(w), str(co), str(n)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(g) for g in got] == [-(-h // M.TH) * -(-w // M.TW), -(-co // M.NB), n]


def test_three_term_split_is_exact():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096), rng.standard_normal(4096) * 1e-20, rng.standard_normal(4096) * 1e20,
                        rng.integers(0, 256, 512) / 255.0, [0.0, -0.0, 1.0, -1.0, 2.0**-100, -1.2345678 * 2.0**-100, 3.0e38, 3.38e38, 1.0 + 2.0**-23,
                                                            1.0 - 2.0**-24, 255.0 / 256.0]]).astype(np.float32)
    # exact wherever no term leaves bfloat16's range: the third term of |x| < 2^-117 falls under its smallest subnormal
    # (2^-133), and a float32 above bfloat16's largest finite value (3.39e38) rounds to infinity
    x0, x1, x2 = M.split3(x)
    for t in (x0, x1, x2):
        assert ((t.view(np.uint32) & 0xFFFF) == 0).all()  # each term is a bfloat16
    assert ((x0.astype(np.float64) + x1 + x2) == x.astype(np.float64)).all()
    assert (np.abs(x1) <= np.abs(x0) * 2.0**-8 + 1e-45).all() and (np.abs(x2) <= np.abs(x1) * 2.0**-8 + 1e-45).all()
    n0, n1, n2 = M.split3(np.array([np.nan, np.inf, -np.inf], np.float32))
    assert np.isnan(n0[0]) and np.isnan(n1[0]) and np.isnan(n2[0])
    assert n0[1] == np.inf and n0[2] == -np.inf
    # ties to even, and the carry into the exponent
    assert M.bf16_rne(np.float32(1.0 + 2.0**-8)) == 1.0 and M.bf16_rne(np.float32(1.0 + 3 * 2.0**-8)) == np.float32(1.0 + 2.0**-6)
    assert M.bf16_rne(np.float32(2.0 - 2.0**-9)) == 2.0


def test_restated_convs_agree_with_the_fp64_conv():
    from oracle import qnet_ref as Q

    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 5, 7, 32)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 32, 32)) / 17).astype(np.float32)
    b = rng.standard_normal(32).astype(np.float32)
    want = Q.conv_fwd(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64), 1)[0]
    for got in (M.conv_valu(x, w, b), M.conv_mx(x, w, b)):
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()
    assert M.ORDER == ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


@pytest.mark.parametrize("name", list(M.ROWS))
def test_both_kernels_select_the_oracles_pool_elements(name):
    """The max-pool is discontinuous: a row is only worth comparing on the device if float32 rounding, in either kernel's
    summation order, moves no window's maximum to another element than fp64's.  Online nets: the ones whose pools run backward."""
    obs, feats, A, K, B, *_ = M.case(name)
    for k in range(K):
        want = [M.pool_selection(c0) for c0 in M.stage_outputs(name, k)[0]]
        for mode in ("valu", "bf16x3"):
            got = [M.pool_selection(c0) for c0 in M.conv0_outputs_f32(name, k, mode)]
            for s in range(3):
                assert (got[s] == want[s]).all(), (name, k, mode, s, int((got[s] != want[s]).sum()))
