// Item tables of the plane conv launches -- CFwdDesc for the one-item kernels, CItem for the persistent one -- built on the
// host where a launch plan is made (host code only: no device call, so the stand-alone check tools/probes/conv_items_check.hip
// and idqn_debug_conv_items run it without a GPU).  Both tables list the items in ONE launch order: convp_item_index.
// Entry b of a table is what workgroup b of k_cfwd (or of the data-gradient role of k_cpair) used to derive from its
// index with divisions and modulos in front of its first LDS-DMA copy; the index -> item order is unchanged:
//   net-major    slot = b / items_per_slot, range = b % items_per_slot     (an XCD walks the ranges of one net)
//   range-major  range = b / n_slots, slot = b % n_slots                   (Conv_0: the nets share the staged minibatch)
//   slot = net * nb + batch block; range -> variant by r_begin[], then the balanced cut of the variant's OH * OW positions.
// The persistent kernel's ranges are (output row, column part) pairs: row_parts balanced parts per row, never across rows.
#pragma once
#include "convp.h"

// launch index b -> (slot, variant, range inside the variant) for the launch order and ranges of `a`
static inline void convp_item_index(const CFwdArgs& a, int n_items, int b, int& slot, int& vi, int& r) {
    const int n_slots = n_items / a.items_per_slot;
    const int rr = a.range_major ? b / n_slots : b % a.items_per_slot;
    slot = a.range_major ? b % n_slots : b / a.items_per_slot;
    vi = 0;
    for (int i = 1; i < 4; ++i)
        if (i < a.n_var && rr >= a.r_begin[i]) vi = i;
    r = rr - a.r_begin[vi];
}

// Fills out[0 .. n_items) from the launch arguments (the plan's ranges and the role's geometry).
// Returns false when an item does not fit the descriptor (more than CP_MAX_STRIPS rows, a count past 16 bits).
static inline bool convp_fill_fwd_items(const CFwdArgs& a, int n_items, CFwdDesc* out) {
    if (a.items_per_slot <= 0 || n_items % a.items_per_slot) return false;
    for (int b = 0; b < n_items; ++b) {
        int slot, vi, r;
        convp_item_index(a, n_items, b, slot, vi, r);
        const CVar& v = a.var[vi];
        const int net = slot / a.nb, bb = slot - net * a.nb;
        const int npos = v.OH * v.OW, R = a.r_cnt[vi];
        const int base = npos / R, rem = npos - base * R;
        const int p0 = r * base + (r < rem ? r : rem), np = base + (r < rem ? 1 : 0);
        if (np <= 0 || v.OW > 0xffff || v.OH > 0x7fff || (p0 + np - 1) / v.OW - p0 / v.OW >= CP_MAX_STRIPS) return false;
        CFwdDesc d;
        memset(&d, 0, sizeof(d));
        d.net = net; d.bb = bb; d.out_slot = slot; d.var = vi; d.p0 = p0; d.np = np; d.oh0 = p0 / v.OW;
        for (int s = 0; s < CP_MAX_STRIPS; ++s) {
            const int row = d.oh0 + s;
            const int lo = p0 > row * v.OW ? p0 : row * v.OW, hi = p0 + np < (row + 1) * v.OW ? p0 + np : (row + 1) * v.OW;
            if (hi > lo) { d.c0[s] = (unsigned short)(lo - row * v.OW); d.ncol[s] = (unsigned short)(hi - lo); }
        }
        const long in_slot = (long)(a.in_split > 0 ? (net >= a.in_split ? 1 : 0) : net) * a.nb + bb;
        d.in_off = in_slot * a.in_slot + (long)(d.oh0 * a.S + v.in_off_h) * a.row_bytes + (long)(d.c0[0] * a.S + v.in_off_w) * a.pix_bytes;
        d.w_off = (long)net * a.wq_stride + v.w_off;
        out[b] = d;
    }
    return true;
}

// The persistent kernel's table (a.row_parts > 0, r_cnt[v] = OH * row_parts): range r of a variant = part r % row_parts of
// output row r / row_parts.  Returns false when the ranges of `a` are not such a cut.
static inline bool convp_fill_pp_items(const CFwdArgs& a, int n_items, CItem* out) {
    if (a.items_per_slot <= 0 || a.row_parts <= 0 || n_items % a.items_per_slot) return false;
    for (int b = 0; b < n_items; ++b) {
        int slot, vi, r;
        convp_item_index(a, n_items, b, slot, vi, r);
        const int OW = a.var[vi].OW, row = r / a.row_parts, part = r % a.row_parts, base = OW / a.row_parts, rem = OW % a.row_parts;
        if (a.r_cnt[vi] != a.var[vi].OH * a.row_parts || base <= 0) return false;
        CItem it;
        memset(&it, 0, sizeof(it));
        it.net = slot / a.nb; it.bb = slot % a.nb; it.var = vi;
        it.row = row; it.col0 = part * base + (part < rem ? part : rem);
        it.p0 = row * OW + it.col0; it.np = base + (part < rem ? 1 : 0);
        out[b] = it;
    }
    return true;
}
