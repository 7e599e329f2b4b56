"""Host checks of the impala f32 matrix-core Dense_0 forward (IDQN_IMP_D0=mfma): what the shape table of
tests/impala_d0_mx_shapes.py covers (computed from the rows, not asserted by hand), the plan, the switch and the rule of
csrc/imp_d0_mx_args.h through its stand-alone probe against the Python restatement, and the kernel's constants against the
default kernel's.  No GPU.

The kernel's arithmetic has no restatement here: its claim is byte equality with k_imp_d0_fwd on the device, and numpy has no
fused multiply-add (emulating one through float64 rounds twice)."""
import os
import re
import shutil
import subprocess

import pytest

import impala_d0_mx_shapes as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dqn_amd", "csrc")
NAMES = list(D.ROWS)


def _cxx():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)


def _plans():
    """{name: (B, F, D, plan of the learner step's launch)} of the rows that launch a Dense_0 forward"""
    out = {}
    for n, (obs, feats, A, K, B) in D.ROWS.items():
        F, Dh, _ = D.dense0(n)
        if D.applies(n):
            out[n] = (B, F, Dh, D.plan(B, F, Dh, 2 * K))
    return out


def test_table_covers_what_the_kernel_can_get_wrong():
    plans = _plans()
    own = {n: v for n, v in plans.items() if n != "workload"}
    for n, (obs, feats, A, K, B) in D.ROWS.items():
        if n != "workload":
            assert obs[0] <= 16 and obs[1] <= 16 and K <= 2 and B <= 33 and max(feats) <= 448, n
    Fs = {v[1] for v in own.values()}
    assert {63, 64, 65, 256, 257, 320, 448} <= Fs
    by_f = {v[1]: v[3] for v in own.values()}
    assert by_f[63][:3] == (1, 1, 1) and 63 % D.PASS, "one ragged pass"
    assert by_f[64][:3] == (1, 1, 1) and 64 % D.PASS == 0, "exactly one pass"
    assert by_f[65][:3] == (2, 1, 2) and 65 % D.PASS == 1 and 65 % 2 == 1, "a second pass of one feature: its MFMA is half padding"
    assert by_f[256][:3] == (4, 1, 4), "exactly one round"
    assert by_f[257][:3] == (5, 2, 1) and 257 % D.PASS == 1, "a round of one pass"
    assert by_f[320][:3] == (5, 2, 1) and 320 % D.PASS == 0, "five whole passes"
    assert by_f[448][:3] == (7, 2, 3), "the last round holds three"
    assert {v[3][2] for v in plans.values()} >= {1, 2, 3, 4}, "every size of the last round"
    assert any(v[1] % 2 for v in own.values()) and any(v[1] % 2 == 0 and v[1] % D.PASS for v in own.values()), "odd and even ragged F"
    # F from more than one position
    obs, feats, *_ = D.ROWS["positions"]
    assert D.pooled(obs[0]) * D.pooled(obs[1]) > 1 and D.dense0("positions")[0] == D.pooled(obs[0]) * D.pooled(obs[1]) * feats[2]
    assert all(D.pooled(D.ROWS[n][0][0]) * D.pooled(D.ROWS[n][0][1]) == 1 for n in own if n not in ("positions", D.CROSS_MODES_ROW))
    # D on each side of the tile and of the default kernel's 64-unit block; B on each side of the sample block
    assert {1, D.TILE - 1, D.TILE, D.TILE + 1, 64, 65} <= {v[2] for v in own.values()}
    assert {1, D.TILE - 1, D.TILE, D.TILE + 1} <= {v[0] for v in own.values()}
    assert any(v[3][4] == 2 and v[0] % D.TILE == 1 for v in own.values()), "two sample blocks, one sample in the second"
    assert any(v[3][3] >= 3 for v in own.values()), "more than two unit tiles"
    assert {D.ROWS[n][3] for n in own} == {1, 2}
    assert any(D.dense0(n)[2] == 3 for n in NAMES), "a second hidden layer"
    assert [n for n in NAMES if not D.applies(n)] == ["no_hid"], "one row without a hidden layer"
    # the workload's widths, as the issue states them
    assert plans["workload"][1:3] == (7744, 512) and D.plan(32, 7744, 512, 10)[:6] == (121, 31, 1, 16, 1, 10)
    assert D.plan(1, 7744, 512, 1)[3:6] == (16, 1, 1)
    assert D.ROWS[D.HISTORY_ROW][4] == 33 and D.ORACLE_ROW in own and D.CROSS_MODES_ROW in own


def test_kernel_constants_are_the_default_kernels_blocks():
    kernels = open(os.path.join(CSRC, "impala_kernels.h")).read()
    args = open(os.path.join(CSRC, "imp_d0_mx_args.h")).read()
    assert re.search(r"^#define IMP_D0_IC %d\b" % D.PASS, kernels, re.M), "a pass is a block of k_imp_d0_fwd's sum"
    for nm, v in (("PASS", D.PASS), ("TILE", D.TILE), ("WAVES", D.WAVES), ("XP", D.XP)):
        assert re.search(r"^#define IMPD0X_%s %d\b" % (nm, v), args, re.M), nm
    assert D.LDS_BYTES == 50176 and D.LDS_BYTES <= 64 * 1024
    mx = open(os.path.join(CSRC, "impala_d0_mx_kernels.h")).read()
    assert "atomic" not in mx.split("#pragma once")[1], "no atomics"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("probe") / "imp_d0_mx_args_probe"
    subprocess.run([cc, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tools", "probes", "imp_d0_mx_args_probe.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_probe_reports_no_failures_and_the_constants(probe):
    out = subprocess.run([probe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "constants %d %d %d %d" % (D.PASS, D.TILE, D.WAVES, D.XP)
    m = re.search(r"^ok: (\d+) checks, 0 failures$", lines[-1])
    assert m and int(m.group(1)) > 1000, out.stdout[-500:]


def test_restated_plan_equals_the_host_function(probe):
    grid = [(B, F, Dh, nets) for B in (1, 2, 31, 32, 33, 64, 65, 256) for F in (1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 320, 448, 511, 513, 7744)
            for Dh in (1, 31, 32, 33, 63, 64, 65, 512) for nets in (1, 2, 10)]
    grid += [(0, 64, 64, 1), (1, 0, 64, 1), (1, 64, 0, 1), (1, 64, 64, 0), (1, 64, 64, 65536), (1, 1 << 20, 1 << 10, 1), (1 << 15, 1 << 15, 32, 1)]  # refused
    for n, (B, F, Dh, p) in _plans().items():
        K = D.ROWS[n][3]
        grid += [(B, F, Dh, 2 * K)] + [(nq, F, Dh, 1) for nq in (1, 2, 32)]  # the learner step, and idqn_q_values
    got = subprocess.run([probe] + [str(v) for g in grid for v in g], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(grid)
    for g, line in zip(grid, got):
        ok = D.shape_ok(*g)
        vals = [int(v) for v in line.split()]
        assert vals[-1] == ok, (g, line)
        if ok:
            assert vals[:-1] == list(D.plan(*g)), (g, line)


def test_the_refusal_rule(probe):
    values = ["valu", "mfma", "bf16x3", "", "MFMA", "mfma ", "f32", "1", "on"]
    got = subprocess.run([probe, "mode"] + values, check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got] == [D.mode_of(None)] + [D.mode_of(v) for v in values]
    assert [D.mode_of(v) for v in (None, "valu", "mfma", "bf16x3")] == [0, 0, 1, -1]
    # the library refuses before anything is allocated, with the issue's message, and only on impala handles
    src = open(os.path.join(CSRC, "qnet.hip")).read()
    m = re.search(r'IDQN_REQUIRE\(cfg->arch != IDQN_ARCH_IMPALA \|\| impd0_mode_of\((\w+)\) != IMPD0_MODE_BAD, "IDQN_IMP_D0 must be valu or mfma, got \'%s\'", \1\);', src)
    assert m, "the refusal and its message"
    assert m.start() < src.index("idqn_handle_s* h = new idqn_handle_s();", src.index('extern "C" int idqn_create')), "before the handle exists"
    # one statement of the launch: both kernels are launched in one host function and nowhere else
    assert src.count("hipLaunchKernelGGL(k_imp_d0_fwd,") == 1 and src.count("hipLaunchKernelGGL(k_imp_d0_fwd_mx,") == 1
    assert src.count("imp_d0_forward(h, d0,") == 2
