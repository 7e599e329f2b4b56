// The body of k_per_write_back (per_step_kernels.h), included between the braces of that kernel and of k_per_group_write_back
// (per_group_kernels.h): one text, so a member of a group is written back by the statements a solo launch runs.  Names it
// expects in scope: nodes, depth, leaves, td_abs, K, n, m, reduce_max, eps, alpha, priorities_out, max_dev, delta_scratch.
    __shared__ unsigned long long key[PER_STEP_MAX_N];
    __shared__ unsigned int cur[PER_STEP_MAX_N];
    __shared__ double pri[PER_STEP_MAX_N];
    __shared__ unsigned long long pmax;
    const int tid = threadIdx.x;
    if (tid == 0) pmax = 0ull;
    __syncthreads();
    if (tid < n) {
        const double pr = per_priority(td_abs + tid, K, n, reduce_max, eps, alpha);
        pri[tid] = pr;
        if (priorities_out) priorities_out[tid] = pr;
        atomicMax(&pmax, (unsigned long long)__double_as_longlong(pr));
    }
    __syncthreads();
    if (tid == 0 && max_dev) atomicMax(reinterpret_cast<unsigned long long*>(max_dev), pmax);
    sumtree_set_body(nodes, depth, leaves, StValuesLds{pri}, n, m, delta_scratch, key, cur);
