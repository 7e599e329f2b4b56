// impala architecture: the head's Dense_0 forward on the f32 matrix cores (IDQN_IMP_D0=mfma; the plan and the constants
// are in imp_d0_mx_args.h).  Same tensors, same arguments (ImpD0Args) and THE SAME BYTES as k_imp_d0_fwd (impala_kernels.h):
//
//   pa_p = fmaf chain from +0 over the features 64 p .. min(64 p + 63, F - 1), ascending, of x[b][i] W[i][o]
//   acc  = bias[o];  acc = acc + pa_p for p = 0 .. P - 1 ascending;  hid[b][o] = fmaxf(acc, 0)
//
// Why the bytes are equal.  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain, one rounding per product
// (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)); common.h), so 32 chained MFMAs from a zero accumulator over the feature pairs
// (64 p + 2 j, 64 p + 2 j + 1), j ascending, are pass p's chain.  The pass sums do not depend on each other; only their
// addition to the bias is ordered, and that is done here in pass order by one lane per output element.
//
// Padding.  A pass that ends behind F (a ragged last pass, or an odd F whose last MFMA holds one feature) is filled up with
// x = +0 and W = -0: the product is -0, and s + (-0) = s in round-to-nearest for EVERY s, either zero included (+0 + -0 = +0,
// -0 + -0 = -0), so the chain leaves the pad with the bits it had at feature F - 1, where k_imp_d0_fwd's loop stops.
// Samples behind B are staged as zeros and units behind D take W = -0; their rows and columns of the tile are never stored.
// Nothing is read outside the leaf or the activation buffer.
//
// A workgroup (256 lanes) owns one tile of 32 samples x 32 hidden units of one net: grid (D / 32, sample blocks, nets).  The
// passes are dealt to the four waves in rounds, pass p to wave p % 4.  Per round: the round's 256 features of the 32 samples
// lie in LDS as [feature][sample] (33-float pitch); wave w takes its A fragments from there (lane l: sample l & 31, feature
// 2 j + (l >> 5)) and its B fragments straight from the leaf (lane l: W[64 p + 2 j + (l >> 5)][o0 + (l & 31)], two 128-byte
// row segments per load).  The next round's W and x are loaded into registers before the round's MFMAs, so they are in flight
// under them.  Then the four pass sums go through LDS and lane t adds, in pass order, those of the four tile elements it owns
// (unit t & 31, samples (t >> 5) + 8 q) to their running sums.  No atomics, no scratch, no partial in HBM.
#pragma once
#include "imp_d0_mx_args.h"
#include "impala_kernels.h"

static_assert(IMPD0X_PASS == IMP_D0_IC, "a pass is the block of k_imp_d0_fwd's sum");
static_assert(IMPD0X_TILE == 32 && IMPD0X_WAVES == 4, "one 32x32x2 accumulator per wave, four waves");

// A wave whose pass and tile lie wholly inside the leaf (a workgroup whose round and block lie inside the activations) loads
// without a condition.  At an edge the loads are still unconditional, from an index clamped into the buffer, and the pad
// value is selected once they have arrived: no lane mask lives across the loads and nothing outside the buffers is addressed.

// Addresses are a wave-uniform base plus a 32-bit byte offset per lane (impd0x_shape_ok bounds F D and B F), so a pass's 32
// loads need 32 offsets in vector registers and no scalar address each.
__device__ __forceinline__ float impd0x_at(const float* base, unsigned byte_off) { return *(const float*)((const char*)base + byte_off); }

// the 32 B operands of wave `wv`'s pass in round `round`: W[i][o] for i = 64 p + 2 j + hh, or -0 behind F / D / the last pass
__device__ __forceinline__ void impd0x_load_w(float (&w)[IMPD0X_PASS / 2], const float* W, int round, int wv, int hh, int o0, int c, const ImpD0Args& a) {
    const int p0 = (round * IMPD0X_WAVES + wv) * IMPD0X_PASS, i0 = p0 + hh, o = o0 + c;
    if (p0 + IMPD0X_PASS <= a.F && o0 + IMPD0X_TILE <= a.D) {  // (wave-uniform)
        unsigned off = 4u * ((unsigned)i0 * (unsigned)a.D + (unsigned)o);
#pragma unroll
        for (int j = 0; j < IMPD0X_PASS / 2; ++j, off += 8u * (unsigned)a.D) w[j] = impd0x_at(W, off);
        return;
    }
    int F = a.F;
    asm volatile("" : "+s"(F));  // (what follows is formed where it is used, not kept in scalar registers across the rounds)
    const unsigned oc = (unsigned)min(o, a.D - 1);
#pragma unroll
    for (int j = 0; j < IMPD0X_PASS / 2; ++j) w[j] = impd0x_at(W, 4u * ((unsigned)min(i0 + 2 * j, F - 1) * (unsigned)a.D + oc));
#pragma unroll
    for (int j = 0; j < IMPD0X_PASS / 2; ++j) asm volatile("" : "+v"(w[j]));  // (the loads stay loads: not sunk into branches)
    const int n = o < a.D ? F - i0 : 0;  // features i0 + 2 j with 2 j < n are the leaf's
#pragma unroll
    for (int j = 0; j < IMPD0X_PASS / 2; ++j) w[j] = 2 * j < n ? w[j] : -0.f;
}

// lane tid's share of the round's x tile: feature 256 round + tid of the block's 32 samples, zeros behind F / B
__device__ __forceinline__ void impd0x_load_x(float (&v)[IMPD0X_TILE], const float* x, int round, int tid, int b0, const ImpD0Args& a) {
    const int r0 = round * (IMPD0X_WAVES * IMPD0X_PASS), i = r0 + tid;
    if (r0 + IMPD0X_WAVES * IMPD0X_PASS <= a.F && b0 + IMPD0X_TILE <= a.B) {  // (workgroup-uniform)
        unsigned off = 4u * ((unsigned)b0 * (unsigned)a.F + (unsigned)i);
#pragma unroll
        for (int t = 0; t < IMPD0X_TILE; ++t, off += 4u * (unsigned)a.F) v[t] = impd0x_at(x, off);
        return;
    }
    int B = a.B;
    asm volatile("" : "+s"(B));  // (as above)
    const unsigned ic = (unsigned)min(i, a.F - 1);
#pragma unroll
    for (int t = 0; t < IMPD0X_TILE; ++t) v[t] = impd0x_at(x, 4u * ((unsigned)min(b0 + t, B - 1) * (unsigned)a.F + ic));
#pragma unroll
    for (int t = 0; t < IMPD0X_TILE; ++t) asm volatile("" : "+v"(v[t]));
    const int n = i < a.F ? B - b0 : 0;  // samples b0 + t with t < n are the batch's
#pragma unroll
    for (int t = 0; t < IMPD0X_TILE; ++t) v[t] = t < n ? v[t] : 0.f;
}

// grid (D / 32, sample blocks, nets)
__global__ __launch_bounds__(256) void k_imp_d0_fwd_mx(ImpD0Args a) {
    __shared__ float xs[IMPD0X_WAVES * IMPD0X_PASS * IMPD0X_XP];     // [feature of the round][sample]
    __shared__ float ps[IMPD0X_WAVES * IMPD0X_TILE * IMPD0X_TILE];   // [wave][sample][unit]: the round's pass sums
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, c = lane & 31, hh = lane >> 5;
    const int o0 = blockIdx.x * IMPD0X_TILE, b0 = blockIdx.y * IMPD0X_TILE, net = blockIdx.z;
    const float* P = a.wbase[net];
    const float* W = P + a.w_off;
    const float* x = a.x + (long)net * a.B * a.F;
    const int passes = (a.F + IMPD0X_PASS - 1) / IMPD0X_PASS, rounds = (passes + IMPD0X_WAVES - 1) / IMPD0X_WAVES;
    // the sums this lane owns: unit o0 + (tid & 31), samples b0 + (tid >> 5) + 8 q
    const int oc = tid & 31, orow = tid >> 5;
    const float bias = o0 + oc < a.D ? P[a.b_off + o0 + oc] : 0.f;
    float acc[4] = {bias, bias, bias, bias};
    float wcur[IMPD0X_PASS / 2], wnext[IMPD0X_PASS / 2], xv[IMPD0X_TILE];
    impd0x_load_w(wcur, W, 0, wv, hh, o0, c, a);
    impd0x_load_x(xv, x, 0, tid, b0, a);
    for (int r = 0; r < rounds; ++r) {
#pragma unroll
        for (int t = 0; t < IMPD0X_TILE; ++t) xs[tid * IMPD0X_XP + t] = xv[t];
        const int in_round = min(IMPD0X_WAVES, passes - r * IMPD0X_WAVES);
        if (r + 1 < rounds) {  // (wave-uniform) the next round's operands, in flight under this round's MFMAs
            impd0x_load_w(wnext, W, r + 1, wv, hh, o0, c, a);
            impd0x_load_x(xv, x, r + 1, tid, b0, a);
        }
        __syncthreads();
        if (wv < in_round) {
            f32x16 pa;
#pragma unroll
            for (int i = 0; i < 16; ++i) pa[i] = 0.f;
            const float* xa = xs + (wv * IMPD0X_PASS + hh) * IMPD0X_XP + c;
#pragma unroll
            for (int j = 0; j < IMPD0X_PASS / 2; ++j) pa = mfma32(xa[2 * j * IMPD0X_XP], wcur[j], pa);
#pragma unroll
            for (int i = 0; i < 16; ++i) ps[(wv * IMPD0X_TILE + mfma_row(i, hh)) * IMPD0X_TILE + c] = pa[i];
        }
        __syncthreads();
        for (int w = 0; w < in_round; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = acc[q] + ps[(w * IMPD0X_TILE + orow + 8 * q) * IMPD0X_TILE + oc];
        if (r + 1 < rounds)
#pragma unroll
            for (int j = 0; j < IMPD0X_PASS / 2; ++j) wcur[j] = wnext[j];
    }
    if (o0 + oc >= a.D) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = b0 + orow + 8 * q;
        if (b < a.B) a.hid[((long)net * a.B + b) * a.D + o0 + oc] = fmaxf(acc[q], 0.f);
    }
}
