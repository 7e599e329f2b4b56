"""CPU (no GPU): the host-built item tables of the one-item plane conv launches (csrc/convp_items.h).

``idqn_debug_conv_items`` runs the library's table builder on launch parameters handed in from here; the test restates,
in Python, the arithmetic a workgroup of ``k_cfwd`` used to do on its index (net- or range-major slot, variant by range,
balanced cut of the variant's positions, strips per output row, byte origins) and asks for equality field by field.
For every case it also checks that the items partition every (net, block, variant, position) exactly once, that there
are no more items than the 256-workgroup grid of a one-item launch, and that every strip an item reads lies inside its
input slot and every kernel it reads inside its net's packed block.

The launch parameters are rebuilt from the frame geometry as csrc/qnet.hip builds them (SAME padding as zero borders,
three planes per activation, Conv_0 reading one plane of 4-pixel chunks).  Ranges per slot: the headline rows carry the
counts the library's planner prints for K = 5, B = 32 (25 / 21 / 21); the other rows take 256 // slots, raised until no
range spans more than four output rows -- the table code is the same whatever the count.  The data-gradient rows (several
output-parity variants per launch) are checked for the partition and the restated fields; their input is the padded
gradient buffer, whose extent is not rebuilt here.
"""
import ctypes as C

import numpy as np
import pytest

KS = [(8, 4), (4, 2), (3, 1)]
MAX_STRIPS = 4
DESC = np.dtype([("in_off", "<i8"), ("w_off", "<i8"), ("net", "<i4"), ("out_slot", "<i4"), ("var", "<i4"), ("p0", "<i4"),
                 ("np", "<i4"), ("oh0", "<i4"), ("c0", "<u2", 4), ("ncol", "<u2", 4), ("bb", "<i4"), ("pad", "<i4")])

CASES = {
    # name: (obs, conv widths, K, B, ranges per slot of the three forward roles or None)
    "headline": ((84, 84, 4), [32, 64, 64], 5, 32, [25, 21, 21]),
    "cnn_small": ((20, 20, 4), [32, 32, 32], 2, 32, None),
    "ragged_36x28": ((36, 28, 4), [32, 64, 64], 2, 32, None),
    "k1": ((84, 84, 4), [32, 64, 64], 1, 32, None),
    "b64": ((84, 84, 4), [32, 64, 64], 5, 64, None),
}


def _same_pad(i, k, s):
    o = -(-i // s)
    pad = max((o - 1) * s + k - i, 0)
    return o, pad // 2, pad - pad // 2


def _layers(obs, widths):
    ih, iw, ci = obs
    out = []
    for (k, s), co in zip(KS, widths):
        oh, lo_h, hi_h = _same_pad(ih, k, s)
        ow, lo_w, hi_w = _same_pad(iw, k, s)
        out.append(dict(K=k, S=s, CI=ci, CO=co, OH=oh, OW=ow, Hp=lo_h + ih + hi_h, Wp=lo_w + iw + hi_w))
        ih, iw, ci = oh, ow, co
    return out


def _rows_ok(npos, OW, R):
    p0 = 0
    for r in range(R):
        n = npos // R + (1 if r < npos % R else 0)
        if n and (p0 + n - 1) // OW - p0 // OW >= MAX_STRIPS:
            return False
        p0 += n
    return True


def _fwd_params(obs, widths, K, B, ranges, role):
    """Launch parameters of the forward role of Conv_<role> for the training set (2K nets, two input sets)."""
    l = _layers(obs, widths)[role]
    nb, n_nets = -(-B // 32), 2 * K
    npos = l["OH"] * l["OW"]
    R = ranges[role] if ranges else min(npos, max(1, 256 // (n_nets * nb)))
    while not _rows_ok(npos, l["OW"], R):
        R += 1
    npa = 1 if role == 0 else 3
    pix = npa * l["CI"] * 64
    wq = [0]
    for x in _layers(obs, widths):
        wq.append(wq[-1] + x["K"] * x["K"] * x["CI"] * x["CO"] * 6)
    par = dict(items_per_slot=R, range_major=int(role == 0), nb=nb, n_var=1, in_split=K if role == 0 else 0, S=l["S"],
               row_bytes=l["Wp"] * pix, pix_bytes=pix, in_slot=l["Hp"] * l["Wp"] * pix, wq_stride=(2 * wq[3] + 1023) // 1024 * 1024,
               var=[dict(r_begin=0, r_cnt=R, OH=l["OH"], OW=l["OW"], in_off_h=0, in_off_w=0, w_off=wq[role])])
    geom = dict(KH=l["K"], KW=l["K"], n_in_slots=(2 if role == 0 else n_nets) * nb, w_bytes=wq[role + 1] - wq[role])
    return par, R * n_nets * nb, n_nets, geom


def _dgrad_params(obs, widths, K, B):
    """The Conv_1 data gradient's shape of launch: four output-parity variants of unequal size over Conv_1's input grid."""
    l = _layers(obs, widths)[1]
    nb, IH, IW = -(-B // 32), _layers(obs, widths)[0]["OH"], _layers(obs, widths)[0]["OW"]
    var, begin = [], 0
    for vi in range(4):
        rh, rw = vi // 2, vi % 2
        OH, OW = (IH - rh + 1) // 2, (IW - rw + 1) // 2
        if OH * OW == 0:
            continue
        R = max(1, min(OH * OW, 128 // (4 * K * nb)))
        while not _rows_ok(OH * OW, OW, R):
            R += 1
        var.append(dict(r_begin=begin, r_cnt=R, OH=OH, OW=OW, in_off_h=1 - rh, in_off_w=1 - rw, w_off=vi * 4 * l["CO"] * l["CI"] * 6))
        begin += R
    pix = 3 * l["CO"] * 64
    par = dict(items_per_slot=begin, range_major=0, nb=nb, n_var=len(var), in_split=0, S=1, row_bytes=(l["OW"] + 3) * pix, pix_bytes=pix,
               in_slot=(l["OH"] + 3) * (l["OW"] + 3) * pix, wq_stride=1 << 22, var=var)
    return par, begin * K * nb, K, None


def _library_table(par, n_items):
    from slimdqn import _hip

    flat = [par[k] for k in ("items_per_slot", "range_major", "nb", "n_var", "in_split", "S", "row_bytes", "pix_bytes", "in_slot", "wq_stride")]
    for v in range(4):
        d = par["var"][v] if v < len(par["var"]) else dict(r_begin=0, r_cnt=1, OH=0, OW=0, in_off_h=0, in_off_w=0, w_off=0)
        flat += [d[k] for k in ("r_begin", "r_cnt", "OH", "OW", "in_off_h", "in_off_w", "w_off")]
    arr = (C.c_int64 * len(flat))(*flat)
    out = np.zeros(n_items, DESC)
    _hip.check(_hip.lib().idqn_debug_conv_items(arr, len(flat), n_items, out.ctypes.data_as(C.c_void_p)), "idqn_debug_conv_items")
    return out


def _restated(par, n_items, b):
    """Item b as a workgroup derived it from its index (csrc/convp_fwd_body.h before the table)."""
    ips, nb = par["items_per_slot"], par["nb"]
    if par["range_major"]:
        n_slots = n_items // ips
        rr, slot = b // n_slots, b % n_slots
    else:
        slot, rr = b // ips, b % ips
    vi = 0
    for i in range(1, par["n_var"]):
        if rr >= par["var"][i]["r_begin"]:
            vi = i
    v = par["var"][vi]
    net, bb = slot // nb, slot % nb
    r, npos, R = rr - v["r_begin"], v["OH"] * v["OW"], v["r_cnt"]
    base, rem = npos // R, npos % R
    p0, n = r * base + min(r, rem), base + (1 if r < rem else 0)
    OW, oh0 = v["OW"], p0 // v["OW"]
    c0, ncol = [0] * 4, [0] * 4
    for s in range(MAX_STRIPS):
        row = oh0 + s
        lo, hi = max(p0, row * OW), min(p0 + n, (row + 1) * OW)
        if hi > lo:
            c0[s], ncol[s] = lo - row * OW, hi - lo
    in_slot = ((1 if net >= par["in_split"] else 0) if par["in_split"] > 0 else net) * nb + bb
    in_off = in_slot * par["in_slot"] + (oh0 * par["S"] + v["in_off_h"]) * par["row_bytes"] + (c0[0] * par["S"] + v["in_off_w"]) * par["pix_bytes"]
    return dict(in_off=in_off, w_off=net * par["wq_stride"] + v["w_off"], net=net, out_slot=slot, var=vi, p0=p0, np=n, oh0=oh0,
                c0=c0, ncol=ncol, bb=bb, pad=0), in_slot


def _check(par, n_items, n_nets, geom):
    tab = _library_table(par, n_items)
    assert n_items <= 256, "a one-item launch is at most one workgroup per CU"
    seen = {}
    for b in range(n_items):
        want, in_slot = _restated(par, n_items, b)
        got = tab[b]
        for k, w in want.items():
            assert np.array_equal(np.asarray(got[k]), np.asarray(w)), (b, k, got[k], w)
        v = par["var"][want["var"]]
        assert sum(want["ncol"]) == want["np"] > 0  # the strips hold every position of the item: none spans a fifth row
        for p in range(want["p0"], want["p0"] + want["np"]):
            key = (want["net"], want["bb"], want["var"], p)
            assert key not in seen, (key, seen[key], b)
            seen[key] = b
        if geom:  # every byte the item's strips and kernels cover lies in its input slot / its net's packed kernels
            lo, hi = in_slot * par["in_slot"], (in_slot + 1) * par["in_slot"]
            assert in_slot < geom["n_in_slots"]
            for s in range(MAX_STRIPS):
                if not want["ncol"][s]:
                    continue
                first = want["in_off"] + s * par["S"] * par["row_bytes"] + (want["c0"][s] - want["c0"][0]) * par["S"] * par["pix_bytes"]
                last = first + (geom["KH"] - 1) * par["row_bytes"] + ((want["ncol"][s] - 1) * par["S"] + geom["KW"]) * par["pix_bytes"]
                assert lo <= first and last <= hi, (b, s, first, last, lo, hi)
            assert want["w_off"] + geom["w_bytes"] <= (want["net"] + 1) * par["wq_stride"]
    total = sum(v["OH"] * v["OW"] for v in par["var"]) * n_nets * par["nb"]
    assert len(seen) == total  # ... and every (net, block, variant, position) exactly once


@pytest.mark.parametrize("role", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_table_is_the_index_arithmetic(name, role):
    obs, widths, K, B, ranges = CASES[name]
    _check(*_fwd_params(obs, widths, K, B, ranges, role))


@pytest.mark.parametrize("name", list(CASES))
def test_data_gradient_table_with_parity_variants(name):
    obs, widths, K, B, _ = CASES[name]
    _check(*_dgrad_params(obs, widths, K, B))


def test_an_item_over_five_rows_is_refused():
    par, n, _, _ = _fwd_params((84, 84, 4), [32, 64, 64], 5, 32, [25, 21, 21], 0)
    par["items_per_slot"] = par["var"][0]["r_cnt"] = 2  # 441 positions in 2 ranges: 11 rows each
    with pytest.raises(Exception):
        _library_table(par, 2 * 10)
