// The phases of the one-launch MLP ("fc") step, each stated ONCE: fc_step_par (fc_par_kernels.h: one step per launch) and
// fc_steps_par (fc_steps_kernels.h: n steps per launch) are sequences of these calls plus what is their own -- when a load is
// requested, the step loop and its prefetch, which stores only the last step makes.  Six kernels run the two sequences
// (k_fc_step_par<3 sources>, k_fc_steps_par, k_fc_group_step, k_fc_group_steps), so a phase cannot differ between them: same
// tiles on the same waves, same k order, same floating-point expressions in the same order.
//
// One workgroup of FCM_T threads per head.  `tv` and `d0` are the thread index and the input width as the caller wants them
// seen by the index arithmetic of a phase: fc_steps_par passes copies that went through an empty asm so that the arithmetic is
// redone every step instead of being hoisted out of its step loop into registers (fc_steps_kernels.h).  PROF stamps thread 0's
// shader clock at the phase boundaries into a.ws (IDQN_FC_PROF, debug build): the single step only, fc_steps_par has none.
// Everything is forced inline: the register / occupancy table of the six kernels is kept by tools/probes/fc_step_resources.hip.
#pragma once
#include "dense0_update.h"
#include "fc_kernels.h"

// A workgroup's LDS, in floats (fc_par_plan / fc_steps_plan fill it)
struct FcParPlan {
    long floats;                  // LDS floats (0: the net does not fit this kernel)
    int drows;                    // rows of a target / delta buffer
    long act_row[FC_MAX_LAYERS + 1];  // first row of the online activations of layer input l
    long buf_off, wo_off, wt_off, misc_off;  // wo / wt: the two nets' parameters in ARENA order; wt later holds the gradient
};

template <bool PROF>
__device__ __forceinline__ void fcp_stamp(const FcArgs& a, int k, int i) {
    if (PROF && threadIdx.x == 0) reinterpret_cast<long long*>(a.ws)[k * 16 + i] = clock64();
}

// Two arenas' slices of this thread, requested together in 16-byte pieces (element 4 (t + 512 j); zeros past the head's end)
template <int NV>
__device__ __forceinline__ void fcp_load2(const float* x, const float* y, long P, float4 (&x4)[NV], float4 (&y4)[NV]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        x4[j] = e < P ? *reinterpret_cast<const float4*>(x + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        y4[j] = e < P ? *reinterpret_cast<const float4*>(y + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// A minibatch out of the replay ring, slot -> element row -> frame (two dependent loads ahead of the frames'): element
// e = t + 512 j of [32][d0] (d0 <= 128), and sample t's action, reward and terminal on the first 32 threads
template <class Src>
__device__ __forceinline__ void fcp_ring_minibatch(const Src& src, int B, int d0, float (&xin)[8], float (&xin2)[8], float& r_b, int& a_b, int& t_b) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = t + FCM_T * j;
        xin[j] = xin2[j] = 0.f;
        if (e < B * d0) {
            const int b = e / d0, i = e - b * d0;
            const int32_t* m = src.row(b);
            xin[j] = src.feature(m, 0, i);
            xin2[j] = src.feature(m, 1, i);
        }
    }
    if (t < 32 && t < B) {
        const int32_t* m = src.row(t);
        a_b = m[4]; r_b = __int_as_float(m[5]); t_b = (int)(uint8_t)m[6];
    }
}

// LDS zeroed, the inputs transposed into it, both nets' parameters staged out of the registers
template <bool PROF, int NV>
__device__ __forceinline__ void fcp_stage(const FcArgs& a, const FcParPlan& p, float* fl, int k, int tv, int d0, const float (&xin)[8],
                                          const float (&xin2)[8], const float4 (&th4)[NV], const float4 (&tt4)[NV]) {
    const int t = threadIdx.x;
    const long P = a.P;
    float* dA = fl + p.buf_off;
    float* misc = fl + p.misc_off;
    // nothing but finite numbers ever lives in this LDS (edge tiles multiply junk rows by zeros / their results are dropped)
    for (long e = tv; e < p.wo_off / 4; e += FCM_T) reinterpret_cast<float4*>(fl)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < 32) { fl[p.wo_off + P + t] = 0.f; fl[p.wt_off + P + t] = 0.f; }
    if (t < 128) misc[t] = 0.f;
    __syncthreads();
    fcp_stamp<PROF>(a, k, 1);
    // ---- inputs, transposed (rows past the batch end are zero inputs; they carry no loss weight)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = tv + FCM_T * j;
        if (e < 32 * d0) {
            const int b = e / d0, i = e - b * d0;
            dA[i * FCM_BSP + b] = xin2[j];
            fl[i * FCM_BSP + b] = xin[j];
        }
    }
    // ---- both nets' parameters to LDS as they are (arena order, 16 bytes per lane): a forward tile reads a matrix along its rows
    // (conflict-free for any pitch), a data-gradient tile down its columns (pitch dout: a few-way conflict on a read that is far
    // from the bottleneck) -- no index arithmetic, no padding to maintain
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (tv + FCM_T * j);
        if (e < P) {
            *reinterpret_cast<float4*>(fl + p.wo_off + e) = th4[j];
            *reinterpret_cast<float4*>(fl + p.wt_off + e) = tt4[j];
        }
    }
    __syncthreads();
    fcp_stamp<PROF>(a, k, 2);
}

// This wave's column tile of layer l of its net (waves 0-3: the online net, waves 4-7: the target net), outT = act(inT W + b):
// both operands of an MFMA step are one conflict-free ds_read_b32 per lane
__device__ __forceinline__ void fcp_forward_tile(const FcNet& n, int l, const float* Wn, const float* inT, float* outT) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, bl = lane & 31, h = lane >> 5;
    const int half = wave >> 2, wsub = wave & 3;
    const int din = n.d[l], dout = n.d[l + 1], ks = (din + 1) / 2, ldw = dout;
    const bool relu = l != n.L - 1;
    // column tile ct on wave (ct + half) % 4 of the group: a one-tile layer (the Q head) then runs its two nets on two
    // different SIMDs instead of queueing both chains on SIMD 0
    const int ct = (wsub - half) & 3;
    if (ct * 32 < dout) {
        const int col = ct * 32 + bl;
        const float bv = Wn[n.b_off[l] + min(col, dout - 1)];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* Ap = inT + h * FCM_BSP + bl;             // A[b = bl][k = 2 s + h]
        const float* Bp = Wn + n.w_off[l] + h * ldw + col;    // B[k = 2 s + h][col] (steps past din masked)
        if (din & 1) {  // (an odd input width: the second half-wave's last step has no row)
            for (int s0 = 0; s0 < ks; ++s0) acc = mfma32(Ap[2 * s0 * FCM_BSP], 2 * s0 + h < din ? Bp[2 * s0 * ldw] : 0.f, acc);
        } else {
#pragma unroll 2
            for (int s0 = 0; s0 < ks; ++s0) acc = mfma32(Ap[2 * s0 * FCM_BSP], Bp[2 * s0 * ldw], acc);
        }
        if (col < dout) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[r] + bv;
                outT[col * FCM_BSP + mfma_row(r, h)] = relu ? fmaxf(v, 0.f) : v;
            }
        }
    }
}

// Reciprocal Adam bias corrections of optax step number `step_no` (= count + 1; two double pows) -> bc[0..1], and to a.bcinv
// where `publish`.  One thread calls this, on a wave that has no tile of the Q head's layer.
__device__ __forceinline__ void fcp_bias_corrections(const FcArgs& a, int k, int step_no, float* bc, bool publish) {
    const double tt = (double)step_no;
    const float r1 = 1.0f / (1.0f - (float)pow((double)a.adam_b1, tt)), r2 = 1.0f / (1.0f - (float)pow((double)a.adam_b2, tt));
    bc[0] = r1; bc[1] = r2;
    if (publish) { a.bcinv[2 * k] = r1; a.bcinv[2 * k + 1] = r2; }
}

// Both nets' forwards, side by side, one barrier per layer; the thread that no tile of the Q head's layer keeps busy computes
// the bias corrections of step `step_no` meanwhile instead of holding the first barrier back.  Returns the target net's Q
// [A][BSP] (in dA or dB); the online net's is the activation block of layer input L.
template <bool PROF>
__device__ __forceinline__ const float* fcp_forwards(const FcArgs& a, const FcParPlan& p, float* fl, int k, int step_no, float* bc, bool publish) {
    const int t = threadIdx.x, half = t >> 8;
    const FcNet& n = a.net;
    const float* Wn = fl + (half == 0 ? p.wo_off : p.wt_off);
    float* cur = fl + p.buf_off;
    float* nxt = cur + (long)p.drows * FCM_BSP;
    for (int l = 0; l < n.L; ++l) {
        fcp_forward_tile(n, l, Wn, half == 0 ? fl + p.act_row[l] * FCM_BSP : cur, half == 0 ? fl + p.act_row[l + 1] * FCM_BSP : nxt);
        if (l == n.L - 1 && t == FCM_T - 1) fcp_bias_corrections(a, k, step_no, bc, publish);
        float* tmp = cur; cur = nxt; nxt = tmp;
        __syncthreads();
        fcp_stamp<PROF>(a, k, 3 + l);
    }
    return cur;
}

// The Q rows [2K][B][A] of the target net (tq) and the online net (q), both [A][BSP] in LDS
__device__ __forceinline__ void fcp_store_q(const FcArgs& a, int k, int A, const float* tq, const float* q) {
    const int B = a.B;
    for (int e = threadIdx.x; e < B * A; e += FCM_T) {
        a.q_dbg[((long)(a.K + k) * B) * A + e] = tq[(e % A) * FCM_BSP + e / A];
        a.q_dbg[((long)k * B) * A + e] = q[(e % A) * FCM_BSP + e / A];
    }
}

// TD error, loss, dL/dq (idqn.py:111-124) of sample t on the first 32 threads: max over actions in action order; the squared
// error to sq[t], dL/dq of the taken action returned.  PER: the importance weight w_b scales both and |TD| goes to a.td_abs
// (prioritized replay); without it the weight is the literal 1 and neither is compiled.
template <bool PER>
__device__ __forceinline__ float fcp_td(const FcArgs& a, int k, int A, const float* tq, const float* q, float r_b, int a_b, int t_b, float w_b, float* sq) {
    const int b = threadIdx.x, B = a.B;
    const float w = PER ? w_b : 1.0f;
    float g = 0.f;
    if (b < 32) {
        float m = -INFINITY;
        for (int ac = 0; ac < A; ++ac) m = fmaxf(m, tq[ac * FCM_BSP + b]);
        float sqv = 0.f;
        if (b < B) {
            const float tgt = r_b + (float)(1 - t_b) * a.gamma_n * m;
            const float td = q[a_b * FCM_BSP + b] - tgt;
            if (PER && a.td_abs) a.td_abs[(long)k * B + b] = fabsf(td);
            sqv = w * td * td;
            g = 2.0f * w * td / (float)a.Bdiv;
        }
        sq[b] = sqv;
    }
    return g;
}

// delta = dL/dq, transposed [A rows][32 samples], goes into the buffer that does NOT hold the target's Q (still being read): its
// rows up to the next multiple of 32 past A zero (activations were there; every one of them, not the first 32: A may be 128).
// A barrier follows (every wave done with the target net's matrices and with delta's old contents), then fcp_delta_set.
__device__ __forceinline__ void fcp_delta_zero(float* delta, int A) {
    for (int e = threadIdx.x; e < 32 * ((A + 31) & ~31); e += FCM_T) delta[(e >> 5) * FCM_BSP + (e & 31)] = 0.f;  // (A <= 128 rows <= drows)
}
// ... the target net's LDS copy, dead now, becomes the zeroed gradient arena Gs, and sample t's dL/dq lands in delta.  A barrier follows.
__device__ __forceinline__ void fcp_delta_set(float* Gs, long P, int tv, float* delta, int B, int a_b, float g_b) {
    const int t = threadIdx.x;
    for (long e = tv; e < P / 4; e += FCM_T) reinterpret_cast<float4*>(Gs)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < 32 && t < B) delta[a_b * FCM_BSP + t] = g_b;
}

// The batch's squared-error sum in sample order (thread 0's is the one used)
__device__ __forceinline__ float fcp_loss_sum(const float* sq) {
    float loss_sum = 0.f;
    if (threadIdx.x == 0)
        for (int b = 0; b < 32; ++b) loss_sum += sq[b];
    return loss_sum;
}

// Backward, top down; per layer the data-gradient tiles first, then the weight-gradient tiles, round-robin over the waves;
// every gradient lands in Gs, the LDS copy of the arena.  delta holds dL/dq on entry; delta and dprev swap per layer.
template <bool PROF>
__device__ __forceinline__ void fcp_backward(const FcArgs& a, const FcParPlan& p, float* fl, int k, float* Gs, float* delta, float* dprev) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, bl = lane & 31, h = lane >> 5;
    const FcNet& n = a.net;
    for (int l = n.L - 1; l >= 0; --l) {
        const int din = n.d[l], dout = n.d[l + 1];
        const float* inT = fl + p.act_row[l] * FCM_BSP;
        const int nti = (din + 31) / 32, nto = (dout + 31) / 32, nd = l > 0 ? nti : 0;
        // tasks round-robin over the waves: waves w and w + 4 share a SIMD, so with the data-gradient tiles (the long chains) on
        // waves 0-3 every SIMD ends up with the same number of MFMAs (a split by per-wave load left SIMDs idle: +4 k cycles)
        for (int task = wave; task < nd + nti * nto; task += FCM_T / 64) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            if (task < nd) {
                // dprev[i][b] = relu'(in[i][b]) * sum_o delta[o][b] * W[i][o]: 32 columns i, k = o in pairs
                const int ti = task, ks = (dout + 1) / 2, ldw = dout;
                const float* Ap = delta + h * FCM_BSP + bl;                                                          // A[b = bl][k = o = 2 s + h]
                const float* Bp = fl + p.wo_off + n.w_off[l] + (long)min(ti * 32 + bl, din - 1) * ldw + h;            // B[k = o][i = bl] (steps past dout masked)
                if (dout & 1) {
                    for (int s0 = 0; s0 < ks; ++s0) acc = mfma32(Ap[2 * s0 * FCM_BSP], 2 * s0 + h < dout ? Bp[2 * s0] : 0.f, acc);
                } else {
#pragma unroll 2
                    for (int s0 = 0; s0 < ks; ++s0) acc = mfma32(Ap[2 * s0 * FCM_BSP], Bp[2 * s0], acc);
                }
                const int i = ti * 32 + bl;
                if (i < din) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int b = mfma_row(r, h);
                        dprev[i * FCM_BSP + b] = inT[i * FCM_BSP + b] > 0.f ? acc[r] : 0.f;
                    }
                }
            } else {
                // gW[i][o] = sum_b inT[i][b] * delta[o][b]: 32 rows i x 32 columns o, k = the 32 samples
                const int tile = task - nd, ti = tile / nto, to = tile - ti * nto;
                const int o = to * 32 + bl;
                const float* Ap = inT + (long)(ti * 32 + bl) * FCM_BSP + h;    // A[i = bl][k = b = 2 s + h]
                const float* Bp = delta + (long)(to * 32 + bl) * FCM_BSP + h;  // B[k = b][o = bl]
                float av[16], bv[16];
#pragma unroll
                for (int s0 = 0; s0 < 16; ++s0) { av[s0] = Ap[2 * s0]; bv[s0] = Bp[2 * s0]; }
#pragma unroll
                for (int s0 = 0; s0 < 16; ++s0) acc = mfma32(av[s0], bv[s0], acc);
                if (o < dout) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int i = ti * 32 + mfma_row(r, h);
                        if (i < din) Gs[n.w_off[l] + (long)i * dout + o] = acc[r];
                    }
                }
            }
        }
        for (int o = FCM_T - 1 - t; o < dout; o += FCM_T) {  // bias gradient, in sample order (the last waves: the shortest task lists)
            float s = 0.f;
            for (int b = 0; b < 32; ++b) s += delta[o * FCM_BSP + b];
            Gs[n.b_off[l] + o] = s;
        }
        __syncthreads();
        fcp_stamp<PROF>(a, k, 9 + (n.L - 1 - l));
        float* tmp = delta; delta = dprev; dprev = tmp;
    }
}

// optax.adam on four consecutive arena elements
__device__ __forceinline__ void fcp_adam4(const AdamConsts& ad, float rbc1, float rbc2, const float4& g, float4& th, float4& m, float4& v) {
    adam_elem(ad, rbc1, rbc2, g.x, th.x, m.x, v.x);
    adam_elem(ad, rbc1, rbc2, g.y, th.y, m.y, v.y);
    adam_elem(ad, rbc1, rbc2, g.z, th.z, m.z, v.z);
    adam_elem(ad, rbc1, rbc2, g.w, th.w, m.w, v.w);
}
