// The body of k_fc_act_many1 (fc_act_many_kernels.h), included INSIDE a kernel's braces -- not a header of its own.  In scope at
// the point of inclusion: a (FcActManyArgs) and the macro FC_ACT_MANY1_PARAMS(e), the parameter base of state e = blockIdx.x:
// the handle's arena by the table's head (k_fc_act_many1: after preprocessing its tokens are what they were) or an entry of the
// group's table of bases (k_fc_group_act_many1, fc_group_kernels.h).
    __shared__ float x[2][FC_MAX_WIDTH];
    __shared__ float part[8][FC_MAX_WIDTH];
    const FcNet& n = a.net;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, e = blockIdx.x;
    const float* params = FC_ACT_MANY1_PARAMS(e);
    const float* s_in = a.s + (long)e * a.s_ld;
    for (int i = t; i < n.d[0]; i += 512) x[0][i] = s_in[i];
    __syncthreads();
    int cur = 0;
    for (int l = 0; l < n.L; ++l) {
        const int din = n.d[l], dout = n.d[l + 1];
        const float* W = params + n.w_off[l];
        const int per = (din + 7) / 8, i0 = wave * per, i1 = min(din, i0 + per);  // per <= 64 (widths <= 512)
        for (int o = lane; o < dout; o += 64) {
            float s = 0.f;
            for (int ib = i0; ib < i1; ib += 16) {
                float w[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) w[u] = ib + u < i1 ? W[(long)(ib + u) * dout + o] : 0.f;
#pragma unroll
                for (int u = 0; u < 16; ++u) s = fmaf(ib + u < i1 ? x[cur][ib + u] : 0.f, w[u], s);
            }
            part[wave][o] = s;
        }
        __syncthreads();
        for (int o = t; o < dout; o += 512) {
            float s = params[n.b_off[l] + o];
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) s += part[w8][o];
            x[cur ^ 1][o] = l != n.L - 1 ? fmaxf(s, 0.f) : s;
        }
        __syncthreads();
        cur ^= 1;
    }
    const int A = n.d[n.L];
    for (int i = t; i < A; i += 512) a.q_out[(long)e * A + i] = x[cur][i];
    if (t == 0) fc_act_many_tail(a, e, x[cur], A);
