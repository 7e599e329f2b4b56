// The body of k_fc_steps_par (fc_steps_kernels.h), included INSIDE a kernel's braces -- not a header of its own.  In scope at
// the point of inclusion: a (FcArgs), p (FcParPlan), ad (AdamConsts), theta / mu / nu (float*), n_steps (int), src; blockIdx.x
// is the head.  k_fc_steps_par supplies them as its kernel arguments, k_fc_group_steps (fc_group_kernels.h) as references
// into record blockIdx.y of a device table.
    extern __shared__ __attribute__((aligned(16))) float fl[];
    const int k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, bl = lane & 31, h = lane >> 5;
    const int half = wave >> 2, wsub = wave & 3;  // waves 0-3: the online net, waves 4-7: the target net
    const FcNet& n = a.net;
    const int B = a.B, A = n.d[n.L];
    const long P = a.P;
    auto act = [&](int l) { return fl + p.act_row[l] * FCM_BSP; };
    float* dA = fl + p.buf_off;
    float* dB = dA + (long)p.drows * FCM_BSP;
    float* Gs = fl + p.wt_off;
    float* misc = fl + p.misc_off;
    float *sq = misc + 32, *bc = misc + 64;
    int32_t* rowsL = reinterpret_cast<int32_t*>(misc + 128);  // [32][8]: the element rows of the next step's samples (16-byte aligned)
    const float* pt = a.target + (long)k * P;
    float* G = a.grad + (long)k * P;
    float* TH = theta + (long)k * P;
    float* MU = mu + (long)k * P;
    float* NU = nu + (long)k * P;
    const int32_t* slots = src.sl.slot;  // [n_steps][B]
    // ---- the four arenas, once
    constexpr int NV = FCP_NPT / 4;
    float4 th4[NV], tt4[NV], mm4[NV], vv4[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        th4[j] = e < P ? *reinterpret_cast<const float4*>(TH + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        tt4[j] = e < P ? *reinterpret_cast<const float4*>(pt + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- the first step's minibatch: slot -> element row -> frame
    float xin[8], xin2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = t + FCM_T * j;
        xin[j] = xin2[j] = 0.f;
        if (e < B * n.d[0]) {
            const int b = e / n.d[0], i = e - b * n.d[0];
            const int32_t* m = src.row(b);
            xin[j] = src.feature(m, 0, i);
            xin2[j] = src.feature(m, 1, i);
        }
    }
    float r_b = 0.f;
    int a_b = 0, t_b = 1;
    if (t < 32 && t < B) {
        const int32_t* m = src.row(t);
        a_b = m[4]; r_b = __int_as_float(m[5]); t_b = (int)(uint8_t)m[6];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        mm4[j] = e < P ? *reinterpret_cast<const float4*>(MU + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        vv4[j] = e < P ? *reinterpret_cast<const float4*>(NU + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int32_t count0 = a.count[k];
    double cum = a.cum[k];  // (thread 0's copy is the one written back)
    float loss_last = 0.f;
    for (int step = 0; step < n_steps; ++step) {
        const bool last = step == n_steps - 1;
        // the per-thread index arithmetic below is redone every step: hoisted out of the step loop its results (a few dozen
        // addresses per lane) would sit in registers beside the four arenas and spill
        int tv = t, d0 = n.d[0];
        asm volatile("" : "+v"(tv));
        asm volatile("" : "+s"(d0));
        // (next minibatch, 1 of 3) the slot of sample t of step + 1
        int sl_b = 0;
        if (!last && t < 32 && t < B) sl_b = slots[(long)(step + 1) * B + t];
        // nothing but finite numbers ever lives in this LDS (edge tiles multiply junk rows by zeros / their results are dropped)
        for (long e = tv; e < p.wo_off / 4; e += FCM_T) reinterpret_cast<float4*>(fl)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < 32) { fl[p.wo_off + P + t] = 0.f; fl[p.wt_off + P + t] = 0.f; }
        if (t < 128) misc[t] = 0.f;
        __syncthreads();
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
        // ---- both nets' parameters to LDS out of the registers, arena order: theta as the last step left it
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const long e = 4L * (tv + FCM_T * j);
            if (e < P) {
                *reinterpret_cast<float4*>(fl + p.wo_off + e) = th4[j];
                *reinterpret_cast<float4*>(fl + p.wt_off + e) = tt4[j];
            }
        }
        __syncthreads();
        // (next minibatch, 2 of 3) its element row (32 bytes, 32-byte aligned): back by the end of the forwards
        int4 rw0 = make_int4(0, 0, 0, 0), rw1 = make_int4(0, 0, 0, 1);
        if (!last && t < 32 && t < B) {
            const int4* m = reinterpret_cast<const int4*>(src.rows + (long)sl_b * 8);
            rw0 = m[0]; rw1 = m[1];
        }
        const float* tq = nullptr;  // the target net's Q
        float g_b = 0.f;
        // ---- forwards: one column tile per wave and layer
        {
            const float* Wn = fl + (half == 0 ? p.wo_off : p.wt_off);
            float *cur = dA, *nxt = dB;
            for (int l = 0; l < n.L; ++l) {
                const int din = n.d[l], dout = n.d[l + 1], ks = (din + 1) / 2, ldw = dout;
                const bool relu = l != n.L - 1;
                const float* inT = half == 0 ? act(l) : cur;
                float* outT = half == 0 ? act(l + 1) : nxt;
                const int ct = (wsub - half) & 3;
                if (ct * 32 < dout) {
                    const int col = ct * 32 + bl;
                    const float bv = Wn[n.b_off[l] + min(col, dout - 1)];
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                    const float* Ap = inT + h * FCM_BSP + bl;             // A[b = bl][k = 2 s + h]
                    const float* Bp = Wn + n.w_off[l] + h * ldw + col;    // B[k = 2 s + h][col] (steps past din masked)
                    if (din & 1) {
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
                if (l == n.L - 1 && t == FCM_T - 1) {
                    // reciprocal Adam bias corrections of this step (optax: t = count + 1; two double pows)
                    const double tt = (double)(count0 + step + 1);
                    const float r1 = 1.0f / (1.0f - (float)pow((double)a.adam_b1, tt)), r2 = 1.0f / (1.0f - (float)pow((double)a.adam_b2, tt));
                    bc[0] = r1; bc[1] = r2;
                    if (last) { a.bcinv[2 * k] = r1; a.bcinv[2 * k + 1] = r2; }
                }
                float* tmp = cur; cur = nxt; nxt = tmp;
                __syncthreads();
            }
            // cur = the target net's Q [A][BSP]
            const float* q = act(n.L);  // the online net's
            if (last) {
                for (int e = t; e < B * A; e += FCM_T) {
                    a.q_dbg[((long)(a.K + k) * B) * A + e] = cur[(e % A) * FCM_BSP + e / A];
                    a.q_dbg[((long)k * B) * A + e] = q[(e % A) * FCM_BSP + e / A];
                }
            }
            // ---- TD error, loss, dL/dq  (idqn.py:111-124): max over actions in action order
            tq = cur;
            if (t < 32) {
                const int b = t;
                float m = -INFINITY;
                for (int ac = 0; ac < A; ++ac) m = fmaxf(m, cur[ac * FCM_BSP + b]);
                float sqv = 0.f, g = 0.f;
                if (b < B) {
                    const float tgt = r_b + (float)(1 - t_b) * a.gamma_n * m;
                    const float td = q[a_b * FCM_BSP + b] - tgt;
                    sqv = td * td;
                    g = 2.0f * td / (float)a.Bdiv;
                }
                sq[b] = sqv;
                g_b = g;  // dL/dq of the taken action
            }
        }
        float* delta = tq == dA ? dB : dA;
        float* dprev = tq == dA ? dA : dB;
        for (int e = t; e < 32 * ((A + 31) & ~31); e += FCM_T) delta[(e >> 5) * FCM_BSP + (e & 31)] = 0.f;  // (A <= 128 rows <= drows)
        if (!last && t < 32 && t < B) {  // the next step's rows to LDS: every thread needs the rows of its elements' samples
            reinterpret_cast<int4*>(rowsL)[2 * t] = rw0;
            reinterpret_cast<int4*>(rowsL)[2 * t + 1] = rw1;
        }
        __syncthreads();  // (every wave is done with the target net's matrices and with delta's old contents)
        for (long e = tv; e < P / 4; e += FCM_T) reinterpret_cast<float4*>(Gs)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < 32 && t < B) delta[a_b * FCM_BSP + t] = g_b;
        // (next minibatch, 3 of 3) the frames of step + 1, in flight while the backward runs; this step's inputs are in LDS
        if (!last) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = tv + FCM_T * j;
                xin[j] = xin2[j] = 0.f;
                if (e < B * d0) {
                    const int b = e / d0, i = e - b * d0;
                    const int4 rw = reinterpret_cast<const int4*>(rowsL)[2 * b];  // {newest, valid} of state and next_state
                    const int pix = i / src.stack, back = src.stack - 1 - (i - pix * src.stack);
                    if (back < rw.y) xin[j] = src.frames[rps_ring_slot(rw.x, back, src.n_frames) * src.frame_elems + pix];
                    if (back < rw.w) xin2[j] = src.frames[rps_ring_slot(rw.z, back, src.n_frames) * src.frame_elems + pix];
                }
            }
            if (t < 32 && t < B) { a_b = rw1.x; r_b = __int_as_float(rw1.y); t_b = (int)(uint8_t)rw1.z; }
        }
        __syncthreads();
        float loss_sum = 0.f;
        if (t == 0)
            for (int b = 0; b < 32; ++b) loss_sum += sq[b];
        // ---- backward, top down; every gradient lands in the LDS copy of the arena
        for (int l = n.L - 1; l >= 0; --l) {
            const int din = n.d[l], dout = n.d[l + 1];
            const float* inT = act(l);
            const int nti = (din + 31) / 32, nto = (dout + 31) / 32, nd = l > 0 ? nti : 0;
            for (int task = wave; task < nd + nti * nto; task += FCM_T / 64) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                if (task < nd) {
                    const int ti = task, ks = (dout + 1) / 2, ldw = dout;
                    const float* Ap = delta + h * FCM_BSP + bl;
                    const float* Bp = fl + p.wo_off + n.w_off[l] + (long)min(ti * 32 + bl, din - 1) * ldw + h;
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
                    const int tile = task - nd, ti = tile / nto, to = tile - ti * nto;
                    const int o = to * 32 + bl;
                    const float* Ap = inT + (long)(ti * 32 + bl) * FCM_BSP + h;
                    const float* Bp = delta + (long)(to * 32 + bl) * FCM_BSP + h;
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
            for (int o = FCM_T - 1 - t; o < dout; o += FCM_T) {  // bias gradient, in sample order
                float s = 0.f;
                for (int b = 0; b < 32; ++b) s += delta[o * FCM_BSP + b];
                Gs[n.b_off[l] + o] = s;
            }
            __syncthreads();
            float* tmp = delta; delta = dprev; dprev = tmp;
        }
        // ---- optax.adam on the registers; the gradient leaves LDS for HBM behind the last step only
        {
            const float rbc1 = bc[0], rbc2 = bc[1];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const long e = 4L * (tv + FCM_T * j);
                if (e < P) {
                    const float4 g = *reinterpret_cast<const float4*>(Gs + e);
                    if (last) *reinterpret_cast<float4*>(G + e) = g;
                    adam_elem(ad, rbc1, rbc2, g.x, th4[j].x, mm4[j].x, vv4[j].x);
                    adam_elem(ad, rbc1, rbc2, g.y, th4[j].y, mm4[j].y, vv4[j].y);
                    adam_elem(ad, rbc1, rbc2, g.z, th4[j].z, mm4[j].z, vv4[j].z);
                    adam_elem(ad, rbc1, rbc2, g.w, th4[j].w, mm4[j].w, vv4[j].w);
                }
            }
        }
        loss_last = loss_sum / (float)a.Bdiv;
        cum = cum + (double)(loss_sum / (float)a.Bdiv);
        __syncthreads();  // (bc and the gradient arena are read; the next step rewrites them)
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const long e = 4L * (t + FCM_T * j);
        if (e < P) {
            *reinterpret_cast<float4*>(TH + e) = th4[j];
            *reinterpret_cast<float4*>(MU + e) = mm4[j];
            *reinterpret_cast<float4*>(NU + e) = vv4[j];
        }
    }
    if (t == 0) {
        a.losses[k] = loss_last;
        a.count[k] = count0 + n_steps;
        a.cum[k] = cum;
    }
