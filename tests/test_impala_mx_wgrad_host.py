"""Host checks of the impala matrix-core weight gradient (IDQN_IMP_WGRAD=bf16x3): the shape table's coverage, the plan of
csrc/imp_mx_wgrad_args.h against its stand-alone probe, and the numpy restatement of the kernel's summation order
(tests/impala_mx_wgrad_shapes.py ``wgrad_mx``) against the fp64 weight gradient on every eligible layer of every row, at the
device test's own bar (tests/test_gpu_impala.py ``_grad_bar``, evaluated on this table).  No GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import impala_mx_wgrad_shapes as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dqn_amd", "csrc")
NAMES = list(W.ROWS)


def _cxx():
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or (rocm_clang if os.path.exists(rocm_clang) else None)


def _grad_bar(name, k, leaf):
    """tests/test_gpu_impala.py's own bar (2e-5, or 4 x the float32 autograd's error), evaluated on this file's table"""
    import test_gpu_impala as G  # imported for the bar alone; nothing of it runs here

    table, G.S = G.S, W
    try:
        return G._grad_bar(name, k, leaf)
    finally:
        G.S = table


def _mx_plans(name):
    """[(stack, conv, B, H, W, ci, co, plan)] of the row's eligible layers"""
    obs, feats, A, K, B = W.ROWS[name]
    mx = set(W.mx_layers(obs, feats))
    return [(s, i, B, h, w, ci, co, W.plan(B, h, w, ci, co)) for s, i, ci, co, h, w in W.conv_layers(obs, feats) if (s, i) in mx]


def test_table_covers_what_the_kernel_can_get_wrong():
    assert set(W.M.ROWS) < set(W.ROWS)
    for n, (obs, feats, A, K, B) in W.ROWS.items():
        if n in W.OWN_ROWS:
            assert obs[0] <= 33 and obs[1] <= 33 and K <= 2 and B <= 6, n
    plans = [(n,) + p for n in NAMES for p in _mx_plans(n)]
    n_tiles = lambda p: p[-1][2]  # noqa: E731
    n_chunks = lambda p: p[-1][3]  # noqa: E731
    assert any(n_tiles(p) == W.TILES for p in plans), "a step whose work is exactly one chunk"
    assert any(n_tiles(p) == W.TILES + 1 for p in plans), "one chunk plus one tile"
    assert any(n_tiles(p) % W.TILES and n_chunks(p) > 1 for p in plans), "a ragged last chunk"
    assert any(n_chunks(p) >= 4 and (p[-1][0] * p[-1][1]) % W.TILES for p in plans), "chunks cut inside images"
    assert any(p[3] == 1 for p in plans), "B = 1"
    assert {16, 32, 64} <= {p[6] for p in plans}, "CI of one, two and four 16-channel steps"
    assert {32, 64} <= {p[7] for p in plans}, "CO of one and two N tiles"
    assert any(p[5] < W.TW for p in plans), "a frame narrower than a k-step"
    assert any(p[5] == W.TW + 1 for p in plans), "a frame one column wider than a k-step"
    assert any(p[4] == 1 for p in plans), "the one-row frame"
    assert any(p[4] % W.TH == 1 and p[4] > W.TH for p in plans), "a frame one row higher than the tiles"
    # an eligible layer directly after an ineligible one, and before one (in the order of the net)
    after = before = False
    for n, (obs, feats, A, K, B) in W.ROWS.items():
        mx = set(W.mx_layers(obs, feats))
        order = [(s, i) for s, i, *_ in W.conv_layers(obs, feats)]
        for a, b in zip(order, order[1:]):
            after |= a not in mx and b in mx and a != (0, 0)
            before |= a in mx and b not in mx
    assert after and before
    assert W.expected_wgrad_launches(*W.ROWS["workload"][:2]) == (14, 1) and W.expected_wgrad_launches(*W.ROWS["all_mx"][:2]) == (14, 1)
    # the uint8 conv is never eligible, whatever its channels
    assert all((0, 0) not in W.mx_layers(obs, feats) for obs, feats, *_ in W.ROWS.values())


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cc = _cxx()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("probe") / "imp_mx_wgrad_args_probe"
    subprocess.run([cc, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tools", "probes", "imp_mx_wgrad_args_probe.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_probe_reports_no_failures_and_the_constants(probe):
    out = subprocess.run([probe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "constants %d %d %d %d %d" % (W.TH, W.TW, W.MB, W.NB, W.TILES)
    m = re.search(r"^ok: (\d+) checks, 0 failures$", lines[-1])
    assert m and int(m.group(1)) > 1000, out.stdout[-500:]


def test_restated_plan_equals_the_host_function(probe):
    grid = [(B, H, Wd, ci, co) for B in (1, 2, 3, 5, 6, 32) for H in (1, 8, 9, 16, 17, 42) for Wd in (3, 15, 16, 17, 33, 42)
            for ci in (16, 32, 48, 64) for co in (32, 64)]
    grid += [(4, 11, 11, 4, 32), (4, 11, 11, 33, 32), (4, 11, 11, 32, 33), (4, 11, 11, 16, 16)]  # ineligible: the flag
    grid += [tuple(p[2:7]) for n in NAMES for p in _mx_plans(n)]
    got = subprocess.run([probe] + [str(v) for g in grid for v in g], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(grid)
    for g, line in zip(grid, got):
        assert [int(v) for v in line.split()] == list(W.plan(*g)) + [int(W.eligible(g[3], g[4]))], (g, line)
    # the workspace holds the larger plan: the matrix-core plan has the vector-ALU kernel's tile and half its chunk
    for B, H, Wd, ci, co in grid:
        assert W.valu_chunks(B, H, Wd) <= W.plan(B, H, Wd, ci, co)[3] <= 2 * W.valu_chunks(B, H, Wd)


def _errors(name, **wrong):
    """{(k, leaf): (kernel error, bias error) / max |g|} of the restatement on the row's eligible layers"""
    obs, feats, A, K, B = W.ROWS[name]
    want = W.oracle(name)
    out = {}
    for k in range(K):
        io = W.conv_io(name, k)
        for s, i in W.mx_layers(obs, feats):
            x, dy = io[(s, i)]
            g, b = W.wgrad_mx(x.astype(np.float32), dy.astype(np.float32), **wrong)
            gw, gb = want[k]["grads"][W.leaf_name(s, i) + "/kernel"], want[k]["grads"][W.leaf_name(s, i) + "/bias"]
            out[(k, W.leaf_name(s, i))] = (np.abs(g - gw).max() / (np.abs(gw).max() + 1e-300), np.abs(b - gb).max() / (np.abs(gb).max() + 1e-300))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_restated_order_stays_inside_the_device_bar(name):
    """The chunk is the block of the sum: one small and one main chain of at most 64 k-steps, no inner blocking.  This is the
    showing that it need not be blocked further: every eligible leaf of every row, at the bar the device test uses."""
    for (k, leaf), (eg, eb) in _errors(name).items():
        print(name, k, leaf, "kernel error / max |g|", eg, "bar", _grad_bar(name, k, leaf + "/kernel"), "bias", eb, "bar", _grad_bar(name, k, leaf + "/bias"))
    for (k, leaf), (eg, eb) in _errors(name).items():
        assert eg <= _grad_bar(name, k, leaf + "/kernel"), (k, leaf, eg)
        assert eb <= _grad_bar(name, k, leaf + "/bias"), (k, leaf, eb)


@pytest.mark.parametrize("wrong, rows", [({"mirror": True}, ("all_mx", "one_row")), ({"col_off": 1}, ("all_mx", "tile_plus")),
                                         ({"drop_ragged": True}, ("many_chunks", "chunk_plus_tile"))])
def test_a_wrong_restatement_is_caught(wrong, rows):
    caught = 0
    for name in rows:
        errs = _errors(name, **wrong)
        worst = max(errs, key=lambda kl: errs[kl][0])
        print(wrong, name, worst, errs[worst], "bar", _grad_bar(name, worst[0], worst[1] + "/kernel"))
        caught += any(eg > _grad_bar(name, k, leaf + "/kernel") for (k, leaf), (eg, eb) in errs.items())
    assert caught >= 1, wrong
