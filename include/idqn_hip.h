/*
 * idqn_hip.h -- C ABI of the MI355X-native i-DQN hot path (libidqn_hip.so, gfx950 only).
 *
 * Plain pointers and sizes only; every pointer marked "dev" is a device (HBM) address, every
 * `stream` is a hipStream_t passed as void*.  All functions return 0 on success or a negative
 * IDQN_E_* code; nothing here falls back to a host implementation.
 *
 * The reference (theovincent/i-DQN) has no FFI: its seam is the Python object protocol used by
 * experiments/base/dqn.py.  Each entry point below names the reference operation it replaces
 * (file:line under the reference root); the Python mirror in i-dqn_amd/slimdqn binds them with
 * ctypes.
 */
#ifndef IDQN_HIP_H
#define IDQN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDQN_OK 0
#define IDQN_E_INVALID (-1)     /* bad argument / unsupported shape (message via idqn_last_error) */
#define IDQN_E_HIP (-2)         /* a HIP runtime call failed */
#define IDQN_E_RANGE (-3)       /* sumtree_query: a target is outside [0, root)   -> ValueError   */
#define IDQN_E_ASSERT (-4)      /* reference `assert` would have fired            -> AssertionError */

#define IDQN_ARCH_CNN 0         /* slimdqn/networks/architectures/dqn.py:39-53 */
#define IDQN_ARCH_FC 1          /* slimdqn/networks/architectures/dqn.py:61-63 */
#define IDQN_ARCH_IMPALA 2      /* slimdqn/networks/architectures/dqn.py:7-29,54-60: three residual Stacks + dense head.
                                   Served by idqn_learn_on_batch, idqn_learn_on_replay_fc(_dev), idqn_q_values / idqn_best_action,
                                   idqn_act_host(_begin / _end), the target operations, idqn_apply_adam, idqn_set_per_buffers and the
                                   debug / profile reads; every other entry answers IDQN_E_INVALID, nothing enqueued.  Its
                                   gradient arena has no second region (gP = head_stride).  Debug buffers: imp_pool<s>,
                                   imp_stack<s> (s = 0..2; imp_stack2 is the head's input, after the final ReLU).           */
#define IDQN_MAX_FEATURES 8
/* impala: 3 Stacks x 5 convs x 2 + the dense leaves.  This was 24 before the impala architecture and idqn_abi_version did
 * not change: a caller of idqn_layout must size its leaves array by THIS constant (recompile against this header); an array
 * of 24 overflows on an impala configuration.                                                                          */
#define IDQN_MAX_LEAVES 48

const char* idqn_last_error(void);
int idqn_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Q-network / agent state.  Replaces iDQN.__init__ (slimdqn/networks/idqn.py:28-63) and
 * DQN.__init__ (slimdqn/networks/dqn.py:14-39) as far as device state goes.
 * ---------------------------------------------------------------------------------------- */
typedef struct idqn_config {
    int32_t arch;                         /* IDQN_ARCH_*                                        */
    int32_t n_heads;                      /* K  (n_networks, idqn.py:44; 1 for DQN)              */
    int32_t n_actions;                    /* A <= 32                                            */
    int32_t obs_h, obs_w, obs_c;          /* cnn: (84, 84, 4); fc: (dim, 1, 1)                    */
    int32_t n_features;
    int32_t features[IDQN_MAX_FEATURES];  /* cnn: [F0, F1, F2, F3]; fc: hidden widths; impala: Stack widths, then dense */
    int32_t max_batch;                    /* largest minibatch a call may pass                   */
    /* doubles: folded to f32 inside exactly like the reference's Python floats are by jit        */
    double learning_rate;                 /* optax.adam(lr, eps=adam_eps), idqn.py:52            */
    double adam_b1, adam_b2, adam_eps;
    double gamma_n;                       /* gamma ** update_horizon (a Python double), idqn.py:122 */
    int32_t n_quantiles;                  /* 0: i-DQN heads.  N > 0: i-IQN heads (extension, see idqn_iqn_learn_on_batch): N
                                             quantile fractions per sample for the online, the action-selection and the
                                             target pass; cnn only; adds the leaves Embed_0/kernel [64][F], Embed_0/bias [F] */
    int32_t reserved;
} idqn_config_t;

typedef struct idqn_leaf {
    char name[32];        /* flax leaf path, e.g. "Conv_0/kernel" (idqn.py:48-50 pytree)        */
    int64_t offset;       /* float offset of the leaf inside one head's slice of an arena        */
    int32_t ndim;
    int64_t shape[4];     /* per-head shape (HWIO for conv kernels, [in,out] for dense)          */
} idqn_leaf_t;

/* Arena layout: every parameter-like array (online, target, mu, nu) is [K][head_stride] floats; head k, leaf l
 * lives at arena + k*head_stride + leaf[l].offset.
 * The GRADIENT arena has K*head_stride + 64 floats arranged as two contiguous regions (two collectives in the
 * data-parallel step): [K][gP] all leaves except the cnn's Dense_0/kernel (same order; gP = head_stride - its padded
 * size), 64 floats reserved for the caller (the Python mirror keeps the K losses there), then [K][Dense_0/kernel].
 * For the fc and impala architectures the second region is empty and gP = head_stride.                           */
int idqn_layout(const idqn_config_t* cfg, int32_t* n_leaves, idqn_leaf_t* leaves /*[IDQN_MAX_LEAVES]*/,
                int64_t* head_stride);

typedef struct idqn_handle_s* idqn_handle_t;

/* The caller (PyTorch-ROCm tensors, storage only) owns the arenas; the handle owns activations
 * and scratch.  count: optax step counter per head (int32, idqn.py:53); losses: per-head loss of
 * the last step (idqn.py:109); cum_losses: f64 running sum == `cumulated_losses += losses`
 * (idqn.py:72) kept on the device so that no per-step host sync is needed.
 * Environment: IDQN_CONV = "bf16x3" (default) | "f32" selects, at creation, the conv arithmetic: f32-accurate
 * products on the bf16 matrix cores (exact three-way operand splits, csrc/convp.h) for every conv forward, data
 * gradient and weight gradient, or v_mfma_f32 everywhere.                                                          */
int idqn_create(const idqn_config_t* cfg, float* online_dev, float* target_dev, float* mu_dev, float* nu_dev,
                float* grad_dev, int32_t* count_dev, float* losses_dev, double* cum_losses_dev,
                idqn_handle_t* out);
int idqn_destroy(idqn_handle_t h);

/* flags for idqn_learn_on_batch */
#define IDQN_F_GRADS_ONLY 1u   /* stop after the gradients are in grad_dev (data-parallel: all-reduce, then idqn_apply_adam) */
#define IDQN_F_PROFILE 2u      /* bracket the dominant kernel with hipEvents (see idqn_profile_read) */
#define IDQN_F_PROFILE_ALL 16u /* one hipEvent after every launch of the step (see idqn_profile_table) */
#define IDQN_F_STOP_AFTER_DENSE0 4u  /* two-call backward, see idqn_backward_rest */
#define IDQN_F_STOP_BEFORE_DENSE0_WGRAD 8u  /* factored data-parallel step, see idqn_finish_step_factored */

/* i-IQN heads -- BASELINE config 3, a LABELLED EXTENSION: the reference snapshot has no quantile code (its README.md:3,10
 * names i-IQN and points at another repository), so nothing here replaces a reference function; oracle/iqn_ref.py states
 * the algorithm (implicit quantile network, Dabney et al. 2018, on the reference's conv trunk; the reference's chain of K
 * heads, idqn.py:13-24,96-109) and parity is pinned to that restatement only.
 * One gradient step of K heads on a minibatch of 1 <= batch <= min(256, max_batch) samples (a handle with n_quantiles > 0
 * takes max_batch <= 256): per head N online fractions, N action-selection
 * fractions and N target fractions per sample, tau_dev = float32 [K][3][N][batch] in (0, 1) (the host draws them);
 * quantile Huber loss (kappa = 1), sum over the online and mean over the target fractions, mean over the batch; Adam on
 * every leaf; count += 1, losses written, cum_losses accumulated -- as idqn_learn_on_batch.  flags: IDQN_F_PROFILE / IDQN_F_PROFILE_ALL only.
 * With idqn_set_per_buffers: weights w float32 [batch] make the loss of head k (1 / batch) sum_b w_b l_kb, where
 * l_kb = (1 / N) sum_ij rho_ij is the per-sample quantile Huber loss, and scale dL/dZ_online of sample b by w_b (the quantile
 * form of loss_k = sum_b w_b td_kb^2 / divisor); td_abs_out [K][batch] receives (1 / N^2) sum_ij |delta_ij|, the mean absolute
 * pairwise TD error (|TD| for N = 1; per_priorities_from_td reads it unchanged).  Either pointer may be NULL; with both NULL the
 * step is the plain one, bit for bit.  A step whose losses are NaN (a gave-up wait of the fused Dense_0 update) writes NaN there. */
int idqn_iqn_learn_on_batch(idqn_handle_t h, const void* state_dev, const void* next_state_dev,
                            const int32_t* action_dev, const float* reward_dev, const uint8_t* terminal_dev,
                            const float* tau_dev, int32_t batch, uint32_t flags, void* stream);
/* Acting rule of IQN for 1 <= n <= max_batch states: q[a] = mean over the N fractions tau_dev [N][n] of Z(s, tau)[a] of head `head`
 * (which = 0 online / 1 target) -> q_out_dev [n][A]; action_out_dev [n] (may be NULL) = argmax, first maximum on ties. */
int idqn_iqn_q_values(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                      const float* tau_dev, float* q_out_dev, int32_t* action_out_dev, void* stream);

/* iDQN.learn_on_batch (idqn.py:96-109) == DQN.learn_on_batch (dqn.py:60-73) for K == 1:
 * 2K forwards, TD target (idqn.py:120-124), squared loss mean over the batch (idqn.py:111-118),
 * K backwards, Adam, count += 1, losses written, cum_losses accumulated.
 * state / next_state: cnn: uint8 [B][H][W][C] (NHWC, the reference's stacked batch, replay_buffer.py:229);
 *                     fc : float32 [B][dim].
 * batch_mean_divisor: the B of the `.mean()` -- pass the GLOBAL batch size when the minibatch is
 * sharded over ranks so that summed shard gradients equal the full-batch gradient.                */
int idqn_learn_on_batch(idqn_handle_t h, const void* state_dev, const void* next_state_dev,
                        const int32_t* action_dev, const float* reward_dev, const uint8_t* terminal_dev,
                        int32_t batch, int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* iDQN.update_online_params (idqn.py:65-72) = ReplayBuffer.sample() (replay_buffer.py:215-230) + learn_on_batch, as ONE call on
 * the HBM frame ring: the stacked gather of replay_gather_stacked (frames of `stack` consecutive transitions, zero frames before
 * an episode start, replay_buffer.py:119-137,223-229) happens inside the step's staging launch, so the sampled minibatch is
 * never materialised and the slots travel as kernel arguments -- no upload, no gather launch.  Same arithmetic and the same
 * results, bit for bit, as replay_gather_stacked followed by idqn_learn_on_batch on its outputs.
 *   frame_ring_dev  uint8 [n_frames][frame_bytes]          (replay_add_frame)
 *   rows_dev        int32 [capacity][8] element rows       (replay_gather_stacked documents the row)
 *   slots_host      int32 [batch] sampled element slots (= key % capacity), HOST memory, read before the call returns
 * Restrictions (IDQN_ERR_INVALID otherwise; callers then gather and call idqn_learn_on_batch): cnn arch on the plane conv
 * path, uint8 frames with frame_bytes == obs_h * obs_w and a multiple of 16, stack == obs_c == 4, batch <= 256.
 * flags as idqn_learn_on_batch, the split steps IDQN_F_STOP_AFTER_DENSE0 / IDQN_F_STOP_BEFORE_DENSE0_WGRAD included (finished by
 * idqn_backward_rest / idqn_finish_step_factored as after idqn_learn_on_batch; bit-identical to gather-then-learn under the same
 * flag).  Only the staging launch reads the ring, the rows and the slots: nothing of them has to outlive this call.          */
int idqn_learn_on_replay(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                         const int32_t* rows_dev, const int32_t* slots_host, int32_t batch, int32_t stack,
                         int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* The same step (idqn.py:65-72, replay_buffer.py:215-230) with the slots in DEVICE memory: slots_dev int32 [batch], read by the
 * staging launch itself (e.g. the leaves per_sample_leaves drew, samplers.py:105-116) -- no host round trip, no gather launch.
 * Every slot must be a valid row of rows_dev (per_importance_weights clamps sampled leaves).  Same results, bit for bit, as
 * idqn_learn_on_replay with the same slots on the host.                                                                       */
int idqn_learn_on_replay_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                             const int32_t* rows_dev, const int32_t* slots_dev, int32_t batch, int32_t stack,
                             int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* The same ONE call (idqn.py:65-72, replay_buffer.py:215-230) for the handles idqn_learn_on_replay refuses; arguments as
 * idqn_learn_on_replay, results bit for bit those of replay_gather_stacked followed by idqn_learn_on_batch on its outputs.
 *   MLP ("fc") handles: float32 frames, frame_bytes * stack == 4 * obs dim, stack in 1..8; feature order as replay_gather_stacked
 *     stacks frame_shape + (stack,): element-major, stack index innermost.  A batch that runs the one-launch step (<= 32 samples,
 *     a net that fits it) reads its minibatch from the ring inside that launch; other batches go through one staging launch.
 *   general-shape cnn handles (the conv path of geometries the plane path does not serve): uint8 frames, frame_bytes ==
 *     obs_h * obs_w (any size), stack == obs_c (any depth); one staging launch, then the step.
 * Restrictions (IDQN_E_INVALID otherwise, nothing enqueued; callers then gather and call idqn_learn_on_batch): not a plane-path
 * cnn handle (idqn_learn_on_replay serves those), not the f32 MFMA conv mode, no quantile heads, batch in [1, max_batch],
 * batch_mean_divisor >= batch, flags as idqn_learn_on_batch accepts them for these handles (no IDQN_F_STOP_*).  Only the first
 * launch reads the ring, the rows and the slots: nothing of them has to outlive this call.                                   */
int idqn_learn_on_replay_fc(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                            const int32_t* rows_dev, const int32_t* slots_host, int32_t batch, int32_t stack,
                            int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* The same step with the slots in DEVICE memory (slots_dev int32 [batch], e.g. the leaves per_sample_leaves drew); bit-identical
 * to idqn_learn_on_replay_fc with the same slots on the host.                                                                */
int idqn_learn_on_replay_fc_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                const int32_t* rows_dev, const int32_t* slots_dev, int32_t batch, int32_t stack,
                                int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* n_steps consecutive replay-sourced steps of an MLP or general-shape cnn handle as ONE call: the handle's state afterwards
 * -- online parameters, Adam moments, count (+= n_steps), losses / gradient / bias-correction scratch / Q debug rows (the last
 * step's), cum_losses (added step by step, in order, in f64) -- equals, byte for byte, n_steps consecutive calls of
 * idqn_learn_on_replay_fc, call i with slots_host + i * batch, the same ring, rows, batch, stack and batch_mean_divisor and
 * flags = 0, on the same stream.  The target arena is read, never written.
 *   slots_host: int32 [n_steps][batch], ordinary HOST memory, read before the call returns (staged through pinned blocks the
 *     handle owns: IDQN_STEPS_STAGING_DEPTH of them, each reused only after the launch that read it has finished, so calls
 *     may follow each other with no synchronisation between them).  Every slot index is used as it arrives.
 *   Handles and batches idqn_learn_on_replay_fc runs through its one-launch step (an MLP whose net fits it, batch <= 32) run
 *     all n_steps in ONE launch that keeps the parameters and moments on chip between the steps; every other handle and
 *     batch idqn_learn_on_replay_fc serves has its n_steps steps enqueued one after the other inside this call.
 * Restrictions (IDQN_E_INVALID otherwise, nothing enqueued or allocated): everything idqn_learn_on_replay_fc refuses; n_steps
 * in [1, IDQN_MAX_STEPS_PER_CALL]; flags == 0; no prioritized-replay buffers set (idqn_set_per_buffers: importance weights
 * and |TD| belong to one step).                                                                                              */
#define IDQN_MAX_STEPS_PER_CALL 32
#define IDQN_STEPS_STAGING_DEPTH 4
int idqn_learn_steps_on_replay_fc(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                  const int32_t* rows_dev, const int32_t* slots_host, int32_t n_steps, int32_t batch,
                                  int32_t stack, int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* The same call with the slots in DEVICE memory (slots_dev int32 [n_steps][batch]; read by the launches, so it must stay
 * unchanged until they have run); bit-identical to the host form.                                                          */
int idqn_learn_steps_on_replay_fc_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                      const int32_t* rows_dev, const int32_t* slots_dev, int32_t n_steps, int32_t batch,
                                      int32_t stack, int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* The i-IQN step on the HBM frame ring: replay_gather_stacked + idqn_iqn_learn_on_batch as ONE call, the way idqn_learn_on_replay
 * fuses the plain step.  Arguments frame_ring_dev .. stack as idqn_learn_on_replay (slots_host: HOST memory, read before the call
 * returns), tau_dev as idqn_iqn_learn_on_batch.  Same results, bit for bit, as the gather followed by idqn_iqn_learn_on_batch on
 * its outputs, importance weights and td_abs of idqn_set_per_buffers included.  Only the staging launch reads the ring, the rows
 * and the slots.  Restrictions (IDQN_E_INVALID otherwise): those of idqn_learn_on_replay plus those of idqn_iqn_learn_on_batch
 * -- a handle with n_quantiles > 0, batch <= min(256, max_batch), flags IDQN_F_PROFILE / IDQN_F_PROFILE_ALL only.          */
int idqn_iqn_learn_on_replay(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                             const int32_t* rows_dev, const int32_t* slots_host, const float* tau_dev, int32_t batch,
                             int32_t stack, uint32_t flags, void* stream);
/* The same step with the slots in DEVICE memory (slots_dev int32 [batch], e.g. the leaves per_sample_leaves drew); bit-identical
 * to idqn_iqn_learn_on_replay with the same slots on the host.                                                              */
int idqn_iqn_learn_on_replay_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                 const int32_t* rows_dev, const int32_t* slots_dev, const float* tau_dev, int32_t batch,
                                 int32_t stack, uint32_t flags, void* stream);
/* Data-parallel overlap: with IDQN_F_STOP_AFTER_DENSE0 (implies gradients only) idqn_learn_on_batch returns
 * once the Dense_0 weight gradient -- 98 % of the gradient bytes, produced first in the backward pass -- is queued;
 * the caller starts all-reducing that slice (RCCL, async) and calls idqn_backward_rest for the conv backward,
 * which then runs concurrently with the collective.                                                               */
int idqn_backward_rest(idqn_handle_t h, void* stream);
/* Factored data-parallel step.  The Dense_0/kernel gradient (98 % of all gradient bytes) is the outer product
 * a3^T . dh over the samples -- rank <= global batch -- so ranks exchange the FACTORS (K x F x 32 + K x J x 32 floats
 * per 32-sample block, ~5.3 MB at K=5) instead of all-reducing the 79 MB product, and every rank runs the fused
 * weight-gradient + Adam kernel over the global batch:
 *   idqn_learn_on_batch(.., IDQN_F_STOP_BEFORE_DENSE0_WGRAD)   forward, head, Dense_0 data gradient
 *   idqn_export_dense0_factors   async copies of this rank's a3 [K][nb][F*32] and dh [K][nb][J*32]
 *   (all-gather both; meanwhile idqn_backward_rest = conv backward; all-reduce the small-leaf gradient region)
 *   idqn_finish_step_factored    phase IDQN_FACTORED_DENSE0: fused Dense_0 update from the gathered factors (needs
 *                                only the gather, so it can run while the small-leaf all-reduce is still in flight);
 *                                phase IDQN_FACTORED_REST: Adam on every other leaf from grad_dev, count += 1,
 *                                cum_losses += losses.  `phases` = either or both (3), Dense_0 first.
 * Block bb of the gathered buffers lives at (bb / nb_inner) * outer + head * head_stride + (bb % nb_inner) * inner
 * (strides in floats); a plain all_gather of the exported buffers gives outer = K*nb*X, head = nb*X, inner = X.   */
int idqn_export_dense0_factors(idqn_handle_t h, float* a3_out_dev, float* dh_out_dev, void* stream);
/* The same two factors WITHOUT a copy: the library keeps dL/dh [K][nb][J*32] directly in front of the online nets' a3
 * [K][nb][F*32], so one contiguous run of n_dh + n_a3 floats at *factors_dev is what a rank contributes to the
 * all-gather (valid from the IDQN_F_STOP_BEFORE_DENSE0_WGRAD call until the next step; ordered behind that call's
 * stream).  In the gathered buffer dh_all = gathered, a3_all = gathered + n_dh, outer stride = n_dh + n_a3.          */
int idqn_dense0_factors(idqn_handle_t h, float** factors_dev, int64_t* n_dh, int64_t* n_a3);
#define IDQN_FACTORED_DENSE0 1u
#define IDQN_FACTORED_REST 2u
int idqn_finish_step_factored(idqn_handle_t h, const float* a3_all_dev, const float* dh_all_dev, int32_t nb_total,
                              int32_t nb_inner, int64_t a3_outer, int64_t a3_head, int64_t a3_inner,
                              int64_t dh_outer, int64_t dh_head, int64_t dh_inner, uint32_t phases, void* stream);
/* Second half of the data-parallel step: Adam from grad_dev, count += 1. */
int idqn_apply_adam(idqn_handle_t h, void* stream);

/* ------------------------------------------------------------------------------------------
 * The data-parallel step with its collectives inside the library (RCCL over xGMI, one process per GPU).  No reference
 * counterpart: iDQN.learn_on_batch (idqn.py:96-109) is single-device; this shards its minibatch mean (idqn.py:111-112).
 * RCCL is resolved at run time (librccl.so.1), the single-GPU entry points do not depend on it.
 * ---------------------------------------------------------------------------------------- */
typedef struct idqn_dp_s* idqn_dp_t;
#define IDQN_DP_UNIQUE_ID_BYTES 128
#define IDQN_DP_SIDE_STREAM 1u /* collectives on a stream of the library's own, ordered by events (the all-gather then runs under
                                  the conv backward); 0: on the caller's stream, in program order, no cross-stream hand-over */
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank (any channel: a file, MPI, torch.distributed). */
int idqn_dp_unique_id(void* id_out /*[IDQN_DP_UNIQUE_ID_BYTES]*/);
/* ncclCommInitRank on the calling thread's current device: collective over the `world` ranks of the job. */
int idqn_dp_create(idqn_handle_t h, const void* unique_id, int32_t rank, int32_t world, uint32_t flags, idqn_dp_t* out);
/* The same around a communicator the caller already owns (an ncclComm_t passed as void*; not destroyed by idqn_dp_destroy). */
int idqn_dp_create_from_comm(idqn_handle_t h, void* nccl_comm, uint32_t flags, idqn_dp_t* out);
/* Destroys the step object (and the communicator idqn_dp_create made).  Call it BEFORE idqn_destroy of the handle it was built on. */
int idqn_dp_destroy(idqn_dp_t dp);
/* rank, world, bytes a rank contributes to the all-gather per 32-sample block of its shard, bytes of the all-reduce (any NULL). */
int idqn_dp_info(idqn_dp_t dp, int32_t* rank, int32_t* world, int64_t* gather_bytes_per_rank, int64_t* allreduce_bytes);
/* One global gradient step: this rank's `batch`-sample shard of a global batch of global_batch = world * batch samples.
 * Enqueues idqn_learn_on_batch(IDQN_F_STOP_BEFORE_DENSE0_WGRAD) -> ncclAllGather of the [dL/dh | a3] run -> conv backward
 * (idqn_backward_rest) -> ncclAllReduce(sum) of the small-leaf gradient region and the K losses -> the fused Dense_0 update
 * over the gathered factors -> Adam on every other leaf, count += 1, cum_losses += losses (idqn_finish_step_factored).
 * Nothing synchronises with the host.  losses_dev then holds the loss of the GLOBAL batch.  flags: IDQN_F_PROFILE(_ALL). */
int idqn_dp_step(idqn_dp_t dp, const void* state_dev, const void* next_state_dev, const int32_t* action_dev,
                 const float* reward_dev, const uint8_t* terminal_dev, int32_t batch, int32_t global_batch, uint32_t flags,
                 void* stream);
/* update_online_params (idqn.py:65-72 = replay_buffer.py:215-230 sample + learn_on_batch) sharded over the ranks: idqn_dp_step's
 * schedule with this rank's shard staged straight from its replica of the frame ring (idqn_learn_on_replay's arguments).
 * The shard's slots are slots_host (host memory, read before the call returns) OR slots_dev (device int32 [batch]): exactly one
 * is non-NULL.  global_batch == world * batch (equal shards); every shard divides its loss by global_batch.
 * With prioritized-replay buffers set on the handle (idqn_set_per_buffers: the shard's weights and its |TD| [K][batch]), the
 * shard's |TD| is also all-gathered into td_all_dev, float [world][K][batch] (per_priorities_from_td_gathered reads that
 * layout), on the collectives' stream; the compute stream is ordered behind it.  td_all_dev must be NULL without them.
 * IDQN_E_INVALID: global_batch != world * batch, both or neither slot pointer, td_all_dev inconsistent with the handle, a non-cnn
 * arch or the general-shape conv path.  flags: IDQN_F_PROFILE(_ALL).                                                          */
int idqn_dp_learn_on_replay(idqn_dp_t dp, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                            const int32_t* rows_dev, int32_t stack, const int32_t* slots_host, const int32_t* slots_dev,
                            int32_t batch, int32_t global_batch, float* td_all_dev, uint32_t flags, void* stream);

/* iDQN.update_target_params, T-step (idqn.py:78-80): target <- online (a REAL copy; the reference
 * aliases immutable arrays), then online[k] <- online[k+1] for k < K-1.  Adam state is not shifted. */
int idqn_target_update(idqn_handle_t h, void* stream);
/* D-step, sync_target_params (idqn.py:20-24,92): target[k] <- online[k-1] for k >= 1.              */
int idqn_target_sync(idqn_handle_t h, void* stream);

/* network.apply(params[head], states) (idqn.py:131, dqn.py:90): Q-values of one head for n <= 32
 * states; which = 0 online / 1 target.  q_out_dev: float32 [n][A].                                 */
int idqn_q_values(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                  float* q_out_dev, void* stream);
/* `network.apply(params[idx], state)` followed by `jnp.argmax` (idqn.py:126-131, dqn.py:88-92): the greedy action of
 * each of the n states (first maximum on ties) as int32 in action_out_dev [n]; the Q-values are left in q_out_dev.   */
int idqn_best_action(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                     float* q_out_dev, int32_t* action_out_dev, void* stream);

/* The greedy branch of select_action for ONE state in PINNED host memory (slimdqn/sample_collection/utils.py:8-21:
 * upload, `best_action`, blocking `.item()`): uint8 pixels for the cnn, float32 features for the fc arch.  The action of
 * head `head` is in action_host_pinned[0] when the call returns; q_out_dev receives the A Q-values (device memory,
 * ordered on `stream` like any other result).  By default the last kernel writes the action into a mapped host mailbox
 * that the call polls, so it returns WITHOUT a stream synchronisation (work queued on `stream` behind it may still be
 * running); IDQN_ACT_POLL=0 restores a device-to-host copy plus hipStreamSynchronize.  After the first call per (net,
 * buffers) the whole sequence is replayed as one hipGraph (IDQN_ACT_GRAPH=0: eager).                                   */
int idqn_act_host(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned, float* q_out_dev,
                  int32_t* action_host_pinned, void* stream);
/* The same in two halves, so that host work that does not depend on the action (the replay-buffer bookkeeping of the
 * PREVIOUS transition, key splits) runs while the GPU computes it: _begin uploads and launches and returns at once, _end
 * waits for the action exactly as idqn_act_host does.  One launch may be pending per handle.                         */
int idqn_act_host_begin(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned, float* q_out_dev,
                        int32_t* action_host_pinned, void* stream);
int idqn_act_host_end(idqn_handle_t h, int32_t* action_host_pinned, void* stream);

/* The same for the i-IQN heads (a handle with cfg.n_quantiles = N > 0): the acting rule of IQN on the reference's
 * best_action protocol (idqn.py:126-131; oracle/iqn_ref.py:157-160, `greedy_action`) for ONE uint8 state and N quantile
 * fractions tau [N] in (0, 1), both in PINNED host memory:  q[a] = (1 / N) sum_l Z(s, tau_l)[a]  of head `head`, summed in
 * the order l = 0 .. N - 1, is left in q_out_dev [A]; its first maximum is in action_host_pinned[0] when the call returns.
 * Mailbox, graph replay (one linear chain per (net, buffers)), IDQN_ACT_POLL and IDQN_ACT_GRAPH as for idqn_act_host; every
 * sum runs in a fixed order, so eager and replayed calls give the same bits.  IDQN_E_INVALID, before anything is enqueued:
 * a handle without quantile heads, a bad head / which, a null pointer, a launch still pending.                          */
int idqn_iqn_act_host(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned,
                      const float* tau_host_pinned, float* q_out_dev, int32_t* action_host_pinned, void* stream);
/* ... in two halves: idqn_act_host_end collects the action of either kind; one launch is pending per handle.         */
int idqn_iqn_act_host_begin(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned,
                            const float* tau_host_pinned, float* q_out_dev, int32_t* action_host_pinned, void* stream);

/* select_action's greedy branch for n <= 32 host states at once, one head each (a vector of environments, each drawing
 * its head as idqn.py:126-131 does): heads_host [n] (ordinary host memory, read before the call returns) and n uint8
 * states in PINNED host memory; row e of q_out_dev [n][A] and actions_host_pinned[e] are, byte for byte, what
 * idqn_act_host gives for (which, heads_host[e], state e) -- the same kernels' arithmetic with a state dimension
 * (csrc/act_many_kernels.h).  States that share a head share one stream of that head's Dense_0 kernel.  Blocking, like
 * idqn_act_host; one linear hipGraph per (n, buffers) serves every head assignment and both parameter sets (the heads
 * travel as data); a mailbox and sequence counter of its own; IDQN_ACT_GRAPH=0 and IDQN_ACT_POLL=0 as for idqn_act_host.
 * IDQN_E_INVALID, before anything is enqueued: n outside [1, 32], a head outside [0, K), which not 0 / 1, a null pointer,
 * an idqn_act_host_begin still pending, a handle with quantile heads, and every handle outside the single-state cnn
 * path (fc, general-shape cnn, IDQN_ACT_GENERIC, J > 512, A > 32).                                                      */
int idqn_act_host_many(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                       float* q_out_dev, int32_t* actions_host_pinned, void* stream);

/* The same call for the handles idqn_act_host_many refuses: arch == IDQN_ARCH_FC with any widths, and general-shape cnn
 * handles (reference ops: idqn.py:126-131 best_action, utils.py:8-21 select_action -- the LunarLander experiment is fc,
 * [100, 100], K = 3).  Signature and contract of idqn_act_host_many; the n states in PINNED host memory are float32 rows
 * [n][obs] for fc and uint8 pixels for the cnn.  Row e of q_out_dev [n][A] and actions_host_pinned[e] are, byte for byte,
 * what idqn_act_host gives for (which, heads_host[e], state e): one workgroup per state runs that path's arithmetic in its
 * order (csrc/fc_act_many_kernels.h), one launch for fc, four for the general-shape cnn.  Blocking; one linear hipGraph
 * per (n, buffers), heads and `which` travel as data; a mailbox and sequence counter that are not the single-state
 * path's; IDQN_ACT_GRAPH=0 and IDQN_ACT_POLL=0 as for idqn_act_host.  IDQN_E_INVALID, before anything is enqueued or
 * allocated on the device: a null pointer, n outside [1, 32], which not 0 / 1, a head outside [0, K), an
 * idqn_act_host_begin still pending, a handle with quantile heads, a handle of the MFMA cnn path (idqn_act_host_many
 * serves those).                                                                                                        */
int idqn_act_host_many_fc(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                          float* q_out_dev, int32_t* actions_host_pinned, void* stream);

/* The same call for impala handles (arch == IDQN_ARCH_IMPALA), which the two entries above refuse.  Signature and contract
 * of idqn_act_host_many_fc; the n states in PINNED host memory are uint8 pixels [n][H][W][C].  Row e of q_out_dev [n][A]
 * and actions_host_pinned[e] are, byte for byte, what idqn_act_host gives for (which, heads_host[e], state e): the n
 * states run as n nets of one image each through the conv and pool kernels of the single-state path, a head's states
 * share ONE stream of its Dense_0/kernel, spread over the chip with every 64-feature pass sum stored and added to the
 * bias in pass order, and one workgroup per state runs the layers behind it (csrc/imp_act_many_kernels.h).  Every shape
 * idqn_create accepts for the architecture is served (heads without a hidden layer, A > 32).  Blocking; one linear
 * hipGraph per (n, buffers), heads and `which` travel as data and the parameter bases are resolved on the device; the
 * handle's many-state slot and mailbox; IDQN_ACT_GRAPH=0 and IDQN_ACT_POLL=0 as for idqn_act_host.  IDQN_E_INVALID,
 * before anything is enqueued or allocated on the device: a handle of another architecture, a null pointer, n outside
 * [1, 32], which not 0 / 1, a head outside [0, K), an idqn_act_host_begin still pending.                                */
int idqn_act_host_many_impala(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                              float* q_out_dev, int32_t* actions_host_pinned, void* stream);

/* The same for the i-IQN heads: the acting rule of idqn_iqn_act_host for n <= 32 host states at once, one head and N
 * fractions each.  heads_host [n] (ordinary host memory, read before the call returns), n uint8 states and the fractions
 * taus [n][N] in (0, 1) in PINNED host memory.  BYTE IDENTITY: row e of q_out_dev [n][A] and actions_host_pinned[e] are,
 * byte for byte, what idqn_iqn_act_host gives for (which, heads_host[e], state e, taus[e]) -- the same kernels'
 * arithmetic, operation for operation and in the same order, with a state dimension (csrc/iqn_act_many_kernels.h).
 * States that share a head share one stream of that head's Dense_0 kernel.  Blocking; one linear hipGraph per (n, buffers)
 * serves every head assignment, both parameter sets and every set of fractions (they travel as data); mailbox, counters
 * and sequence number of its own; IDQN_ACT_GRAPH=0 and IDQN_ACT_POLL=0 as for idqn_act_host.
 * IDQN_E_INVALID, before anything is enqueued: a null pointer, n outside [1, 32], which not 0 / 1, a head outside
 * [0, K), a handle without quantile heads, an acting launch still pending (idqn_act_host_begin / idqn_iqn_act_host_begin),
 * shapes outside the single-state i-IQN kernels (odd F, J not 32 m <= 512, A > 32, N > 64) or outside the acting conv
 * kernels' plan.                                                                                                      */
int idqn_iqn_act_host_many(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned,
                           const float* taus_host_pinned /* [n][N] */, int32_t n,
                           float* q_out_dev /* [n][A] */, int32_t* actions_host_pinned /* [n] */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Seed groups: S independent MLP ("fc") handles learn and act in ONE launch.  No reference counterpart in code: the
 * reference runs its seeds as N processes on one device (launch_job/.../train.sh).  The one-launch MLP step uses one
 * workgroup per head; the heads of a step never talk to each other, so S agents are a grid of (K, S) such workgroups
 * (csrc/fc_group_kernels.h) and every member's bytes after a group call are the bytes of the same call on that member alone.
 * A group is an opaque object over S existing handles.  It owns no parameters: the members keep their arenas, their learning
 * rate, Adam epsilon and gamma^n (a set of seeds or a hyper-parameter sweep), and may be driven alone between group calls
 * on the same stream.  Destroy the group before its members.
 * idqn_group_create refuses (IDQN_E_INVALID, nothing changed): n_members outside [1, 32]; a member that is not an fc handle or
 * whose batches of <= 32 samples do not run the one-launch step; a member whose shape (obs, features, n_actions, n_heads,
 * max_batch) differs from member 0's; a handle (or an online arena) named twice -- one arena would have two writers.  */
typedef struct idqn_group_s* idqn_group_t;
typedef struct idqn_group_ring {   /* a member's replay frame ring, as idqn_learn_on_replay_fc takes it */
    const void* frames_dev; int64_t n_frames, frame_bytes;
    const int32_t* rows_dev; int32_t stack, reserved;
} idqn_group_ring_t;
int idqn_group_create(const idqn_handle_t* members, int32_t n_members, idqn_group_t* out);
int idqn_group_destroy(idqn_group_t group);
/* idqn_learn_on_replay_fc for every member at once: rings [S], slots_host [S][batch] (ordinary host memory, read before the
 * call returns; they and the S member records travel in ONE pinned block with one upload, staged as
 * idqn_learn_steps_on_replay_fc stages its slots), one batch, mean divisor and flags for all members.  ONE launch of grid (K, S).
 * Refuses (IDQN_E_INVALID, nothing enqueued, allocated or staged): batch > 32; flags other than IDQN_F_GRADS_ONLY; a member with
 * prioritized-replay buffers set (idqn_set_per_buffers); everything idqn_learn_on_replay_fc refuses for a member and its ring. */
int idqn_group_learn_on_replay_fc(idqn_group_t group, const idqn_group_ring_t* rings, const int32_t* slots_host, int32_t batch,
                                  int32_t mean_divisor, uint32_t flags, void* stream);
/* idqn_learn_steps_on_replay_fc for every member at once: slots_host [S][n_steps][batch]; ONE persistent launch of grid (K, S)
 * (IDQN_FC_LEARN_STEPS_LOOP=1: n_steps single group launches enqueued inside the call).  Refuses what the single group step
 * refuses, n_steps outside [1, IDQN_MAX_STEPS_PER_CALL] and any flag.                                                          */
int idqn_group_learn_steps_on_replay_fc(idqn_group_t group, const idqn_group_ring_t* rings, const int32_t* slots_host,
                                        int32_t n_steps, int32_t batch, int32_t mean_divisor, uint32_t flags, void* stream);
/* idqn_per_learn_on_replay for every member at once: the prioritized step of S MLP agents.  per[g] is member g's
 * idqn_per_step_t (declared with idqn_per_learn_on_replay below): its own tree (depth, n_items -- members with different
 * replay capacities are served), beta, eps, alpha, reduce_max, stratified and buffers; uniforms_host float64 [batch] in
 * ordinary host memory, read before the call returns; tau_dev NULL.  The S member records with the members' weights / |TD|
 * pointers, the S tree records and the S x batch uniforms travel in ONE pinned block of the group's staging ring (the event
 * guard of the other learner entries): one asynchronous copy, then THREE launches -- k_per_group_draw (grid S: the draws and
 * weights of every member), k_fc_group_step (grid (K, S), slots = member g's leaves_dev) and k_per_group_write_back (grid S)
 * (csrc/per_group_kernels.h: the phases of csrc/per_phases.h on record g).  No host synchronisation, no allocation after the
 * first call, no per-member launch; the members' own prioritized-replay pointers (idqn_set_per_buffers) stay unset throughout.
 * CONTRACT: for every member, online parameters, moments, count, losses, cum_losses, tree nodes, max_priority_dev, leaves,
 * weights, |TD| and priorities after the call equal, byte for byte, what idqn_per_learn_on_replay leaves on that member
 * alone for the same uniforms on the same stream.
 * Refuses (IDQN_E_INVALID with idqn_last_error, nothing enqueued, allocated or staged, nothing changed): a NULL pointer other
 * than max_priority_dev / priorities_dev; batch outside [1, 32]; any flag; a non-NULL tau_dev; depth outside [1, 31];
 * n_items < 1; a member with idqn_set_per_buffers set; everything per_draw, per_write_back and idqn_learn_on_replay_fc_dev
 * refuse for a member; two members naming the same nodes_dev, leaves_dev, weights_dev, td_abs_dev, tree_scratch_dev or non-NULL
 * priorities_dev / max_priority_dev (one buffer would have two writers).                                                      */
struct idqn_per_step;
int idqn_group_per_learn_on_replay_fc(idqn_group_t group, const idqn_group_ring_t* rings /*[S]*/,
                                      const struct idqn_per_step* per /*[S]*/, int32_t batch, int32_t mean_divisor,
                                      uint32_t flags, void* stream);
/* idqn_per_learn_steps_on_replay for every member at once: n_steps consecutive prioritized steps of S MLP agents as ONE call.
 * per[g] is member g's idqn_per_steps_t (declared with idqn_per_learn_steps_on_replay below): leaves_dev / weights_dev
 * [n_steps][batch], td_abs_dev [n_steps][K][batch], priorities_dev [n_steps][batch] (may be NULL), uniforms_host float64
 * [n_steps][batch] in ordinary host memory, read before the call returns.  n_steps in [1, IDQN_MAX_STEPS_PER_CALL], batch in
 * [1, 32], no flags.  Enqueued: ONE pinned block and ONE asynchronous copy -- the member records (step i's record of member g
 * carries that step's slots = row i of the leaves, its weights row and its |TD| row, as idqn_group_per_learn_on_replay_fc sets
 * them), the tree records and all S x n_steps x batch uniforms -- then k_per_group_draw on row 0, for every step the unchanged
 * k_fc_group_step (grid (K, S)) on that step's records, k_per_group_turn (grid S: the write-back of step i and the draw of
 * step i + 1 of member g in one workgroup, csrc/per_group_kernels.h) behind every step but the last, k_per_group_write_back
 * behind the last: 2 n_steps + 1 launches and one upload for all members, where n_steps calls of
 * idqn_group_per_learn_on_replay_fc make 3 n_steps launches and n_steps uploads and S calls of idqn_per_learn_steps_on_replay
 * S (2 n_steps + 1) launches.  At n_steps = 1 the call enqueues exactly what idqn_group_per_learn_on_replay_fc enqueues.  The
 * persistent k_fc_group_steps cannot serve here: every step's draw depends on the previous step's |TD|, so the sampler has to
 * run between two steps.  The block lies in the group's one staging ring, which every group learner entry shares
 * (IDQN_STEPS_STAGING_DEPTH blocks sized for n_steps = 32, each reused only after the launches that read it have finished;
 * all allocated by the group's first learner call, none later); the bytes a call uploads are its own block's alone.
 * CONTRACT: for every member, online parameters, both moments, count, losses, cum_losses, tree nodes, max_priority_dev and
 * every step's row of leaves, weights, |TD| and priorities after the call equal, byte for byte, n_steps calls of
 * idqn_group_per_learn_on_replay_fc on the rows of the uniforms on the same stream -- hence also
 * idqn_per_learn_steps_on_replay on that member alone.
 * Refuses (IDQN_E_INVALID with idqn_last_error naming the entry and the member, nothing enqueued, allocated, staged or
 * changed): a NULL pointer other than priorities_dev / max_priority_dev; n_steps or batch out of range; any flag; depth outside
 * [1, 31]; n_items < 1; a member with idqn_set_per_buffers set; everything idqn_learn_on_replay_fc_dev refuses for a member and
 * its ring; two members naming the same nodes_dev, leaves_dev, weights_dev, td_abs_dev, tree_scratch_dev or non-NULL
 * priorities_dev / max_priority_dev.                                                                                        */
struct idqn_per_steps;
int idqn_group_per_learn_steps_on_replay_fc(idqn_group_t group, const idqn_group_ring_t* rings /*[S]*/,
                                            const struct idqn_per_steps* per /*[S]*/, int32_t n_steps, int32_t batch,
                                            int32_t mean_divisor, uint32_t flags, void* stream);
/* idqn_act_host_many_fc over the members: state e (float32 rows [n][obs] in PINNED host memory) is evaluated on head
 * heads_host[e] of member member_host[e] (both ordinary host memory, read before the call returns).  Row e of q_out_dev [n][A]
 * and actions_host_pinned[e] are, byte for byte, what idqn_act_host gives on that member for (which, heads_host[e], state e).
 * One launch behind the copy node, one workgroup per state; the per-state parameter base travels in the uploaded block, so one
 * hipGraph per (n, buffers) serves every assignment.  The group has an acting slot (block, mailbox, counters) of its own; the
 * members' slots are untouched.  IDQN_E_INVALID before anything is enqueued: a null pointer, n outside [1, 32], which not
 * 0 / 1, a member outside [0, S), a head outside [0, K).                                                                  */
int idqn_group_act_host_fc(idqn_group_t group, int32_t which, const int32_t* member_host, const int32_t* heads_host,
                           const void* states_host_pinned, int32_t n, float* q_out_dev, int32_t* actions_host_pinned, void* stream);

/* Acting groups: the greedy actions of S Atari-shaped (MFMA cnn) agents in one call.  The members are 1..32 handles of the
 * domain idqn_act_host_many accepts.  The group owns ONE acting slot (pinned block and its device copy, conv activations and
 * Dense_0 partials for 32 states, mailbox and counters, graph map); it allocates nothing on a member, writes no member memory,
 * and a member may be driven alone between two group calls.  Destroy the group before its members.
 * idqn_act_group_create refuses (IDQN_E_INVALID, nothing changed): n_members outside [1, 32]; IDQN_ACT_GENERIC; a member that is
 * null, an fc handle, a handle with quantile heads, one with J > 512 or A > 32, any other general-shape cnn handle; a member that differs from member 0 in observation, features, n_actions or n_heads; a handle named twice.       */
typedef struct idqn_act_group_s* idqn_act_group_t;
int idqn_act_group_create(const idqn_handle_t* members, int32_t n_members, idqn_act_group_t* out);
int idqn_act_group_destroy(idqn_act_group_t group);
/* idqn_act_host_many over the members: state e (uint8 [n][H][W][C] in PINNED host memory) is evaluated on head heads_host[e] of
 * member member_host[e] (both ordinary host memory, read before the call returns) with the online (which = 0) or target (1)
 * parameters.  Row e of q_out_dev [n][A] and actions_host_pinned[e] are, byte for byte, what idqn_act_host gives on that member
 * for (which, heads_host[e], state e).  One copy node and five launches -- three conv layers, Dense_0 per run of states with
 * one (member, head) (such states share the W0 stream in register chunks of 8; the same head on two members does not), the
 * head kernel per state; the per-state parameter bases travel in the uploaded block, so one hipGraph per (n, buffers) serves
 * every member and head assignment and both sets.  The actions come back through the slot's mailbox; IDQN_ACT_GRAPH=0 and
 * IDQN_ACT_POLL=0 as for idqn_act_host_many.  IDQN_E_INVALID before anything is enqueued: a null pointer, n outside [1, 32],
 * which not 0 / 1, a member outside [0, S), a head outside [0, K), a member with an idqn_act_host_begin still pending.      */
int idqn_act_group_host(idqn_act_group_t group, int32_t which, const int32_t* member_host, const int32_t* heads_host,
                        const void* states_host_pinned, int32_t n, float* q_out_dev, int32_t* actions_host_pinned, void* stream);

/* Test / debug access to internal activation buffers by name (device pointer + byte size).        */
int idqn_debug_buffer(idqn_handle_t h, const char* name, void** ptr_dev, int64_t* nbytes);

/* Test access to the host code that builds the item table of a one-item plane conv launch (csrc/convp_items.h); no
 * device call.  params = {items_per_slot, range_major, nb, n_var, in_split, S, row_bytes, pix_bytes, in_slot_bytes,
 * wq_stride, then per variant (4 of them): r_begin, r_cnt, OH, OW, in_off_h, in_off_w, w_off} (38 values);
 * out = n_items descriptors of 64 bytes: int64 in_off, int64 w_off, int32 net, out_slot, var, p0, np, oh0,
 * uint16 c0[4], uint16 ncol[4], int32 batch block, int32 0.                                                        */
int idqn_debug_conv_items(const int64_t* params, int32_t n_params, int32_t n_items, void* out_host);
/* Mean duration (ms) and launch count of the dominant kernel over the IDQN_F_PROFILE calls since
 * the last read; synchronises the events it reads.  kernel_name: the dominant kernel.  For MLP
 * handles it is the kernel the LAST step launched, chosen per call and not at idqn_create, with the
 * template variant: k_fc_step_par, k_fc_step_par<ring>, k_fc_steps_par (the persistent launch of
 * idqn_learn_steps_on_replay_fc; when that entry loops, the single step's name), k_fc_step_mfma<global>,
 * k_fc_step_mfma<lds>, k_fc_step_lds<32>, k_fc_step_lds<16>, k_fc_step_lds<8>, k_fc_step.  It is
 * returned whether or not a step carried IDQN_F_PROFILE.                                             */
int idqn_profile_read(idqn_handle_t h, double* mean_ms, int32_t* n_launches, char* kernel_name /*[64]*/);
/* Per-launch table of the IDQN_F_PROFILE_ALL steps since the last read (at most ~100 steps are kept): one line per
 * launch of a step, "name\tmean microseconds\tcount\n", in launch order.  A launch's time is the span between the
 * event behind the previous launch and the event behind it (its duration plus its dispatch gap).                    */
int idqn_profile_table(idqn_handle_t h, char* out, int32_t out_bytes);

/* ------------------------------------------------------------------------------------------
 * Sum tree (slimdqn/sample_collection/sum_tree.py).  nodes_dev: float64 [2**depth - 1] in HBM,
 * depth = ceil(log2(capacity)) + 1, first leaf at 2**(depth-1) - 1 (sum_tree.py:14-17).
 * ---------------------------------------------------------------------------------------- */
/* SumTree.set (sum_tree.py:20-47): deltas against the current leaves BEFORE de-duplication, first
 * occurrence of a duplicate wins, per-level sequential accumulation in ascending node order
 * (bit-exact with np.add.at).  n <= 4096.  scratch_dev: >= 16 * 4096 bytes.                        */
int sumtree_set(double* nodes_dev, int32_t depth, const int32_t* indices_dev, const double* values_dev,
                int32_t n, void* scratch_dev, void* stream);
/* SumTree.get (sum_tree.py:49-51) */
int sumtree_get(const double* nodes_dev, int32_t depth, const int32_t* indices_dev, int32_t n,
                double* out_dev, void* stream);
/* SumTree.query (sum_tree.py:58-102).  status_dev[0] |= 1 if a target is outside [0, root)
 * (-> ValueError, :73-74), |= 2 if the per-level invariant `target < node` fails (-> the reference's
 * assert at :81).  out_dev: int32 leaf indices.                                                     */
int sumtree_query(const double* nodes_dev, int32_t depth, const double* targets_dev, int32_t n,
                  int32_t* out_dev, int32_t* status_dev, void* stream);

/* SumTree.query with ONE host read (sum_tree.py:58-102 returns numpy; samplers.py:105-116 `sample` needs root, leaves and
 * the status of the range check on the host): the n float64 values at values_host are the targets, or -- scale_by_root --
 * the uniforms u_i of the host's PCG64, turned into numpy's `Generator.uniform(0.0, root)` = 0.0 + root * u_i on the device
 * (samplers.py:110).  One launch reads them from a mapped host mailbox, descends, maps leaf -> key through
 * index_to_key_dev (int32 [capacity], NULL: keys = leaves) and writes leaves, keys, root and status back; the host polls
 * the mailbox's sequence number -- no device->host copy, no stream synchronisation, no separate read of the root.
 * status: bit 0 a target outside [0, root) (-> ValueError), bit 1 the per-level assert (:81), bit 2 a leaf >= n_live, the
 * number of valid entries of index_to_key_dev (-> the reference's IndexError from `_index_to_key[index]`, samplers.py:114;
 * its key is returned as -1; n_live < 0: not checked).  root == 0: leaves are 0.  */
int sampler_mailbox_create(int32_t max_n, void** mailbox_out);
int sampler_mailbox_destroy(void* mailbox);
int sumtree_query_host(const double* nodes_dev, int32_t depth, const double* values_host, int32_t n,
                       int32_t scale_by_root, const int32_t* index_to_key_dev, int32_t n_live, void* mailbox,
                       int32_t* leaves_out_host, int32_t* keys_out_host, double* root_out_host,
                       int32_t* status_out_host, void* stream);
/* UniformSamplingDistribution's index -> key map on the device (samplers.py:26-49), for callers that keep sampled keys on
 * the device: add = sampler_map_set(map, len, key); remove = sampler_map_set(map, hole, moved last key) (:31-35: the host
 * map knows both); sample = sampler_map_indices over the int32 indices the host generator drew (:43-49). */
int sampler_map_set(int32_t* index_to_key_dev, int32_t index, int32_t key, void* stream);
int sampler_map_indices(const int32_t* index_to_key_dev, const int32_t* indices_dev, int32_t n, int32_t* keys_out_dev,
                        void* stream);
/* PrioritizedSamplingDistribution.add (samplers.py:62-66): index_to_key[index] = key and tree.set(index, value) for the
 * new last index, ONE launch.  The inverse map key -> index stays a host dict: its only consumers are host-called
 * operations whose arguments are host keys (remove, update). */
int sampler_prioritized_add(double* nodes_dev, int32_t depth, int32_t* index_to_key_dev, int32_t index, int32_t key,
                            double value, void* stream);
/* PrioritizedSamplingDistribution.remove (samplers.py:89-103) for hole = key_to_index[key], last = len - 1: the last
 * entry's priority moves into the hole by the two-leaf set {hole: leaf[last], last: 0.0} (one leaf {hole: 0.0} when
 * hole == last), its key by index_to_key[hole] = index_to_key[last] (:31-35) -- ONE launch, the moved priority is read on
 * the device (the reference reads it with tree.get, :99).  index_to_key_dev may be NULL (tree only). */
int sampler_prioritized_remove(double* nodes_dev, int32_t depth, int32_t* index_to_key_dev, int32_t hole, int32_t last,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Prioritized-replay write-back: an EXTENSION with no reference counterpart (the reference's sample() drops the
 * sampled keys, replay_buffer.py:222-230, and its loss has no importance weights, idqn.py:111-112) -- SURVEY 8f-4,
 * "design freely, parity unpinned".  Checked against the oracle's weighted loss / TD errors only.
 * ---------------------------------------------------------------------------------------- */
/* Per-sample loss weights (float [batch], NULL = the reference's plain mean) and an output for |TD error|
 * (float [K][batch], NULL = none) used by every following idqn_learn_on_batch: loss_k = sum_b w_b td_kb^2 / divisor. */
int idqn_set_per_buffers(idqn_handle_t h, const float* weights_dev, float* td_abs_out_dev);
/* SumTree.set for ONE leaf with the index passed by value (no index upload; sum_tree.py:33-47 for n = 1); the new
 * value is `value`, or value_dev[0] when value_dev is not NULL (e.g. the running maximum priority).                  */
int sumtree_set_one(double* nodes_dev, int32_t depth, int32_t index, double value, const double* value_dev,
                    void* stream);
/* Leaves for targets made on the device from uniforms in [0, 1) (float64 [n]): u_i * root, or the stratified
 * (i + u_i) / n * root; same descent as sumtree_query, no host read of the root.                                      */
int per_sample_leaves(const double* nodes_dev, int32_t depth, const double* uniforms_dev, int32_t n,
                      int32_t stratified, int32_t* leaves_out_dev, void* stream);
/* w_i = (n_items * p_i / root)^(-beta) / max_j w_j for the sampled leaves (p from the sum tree).  The leaves are first
 * clamped, in place, to [0, n_items - 1] (a descent can end on an empty leaf through rounding in the sums).            */
int per_importance_weights(const double* nodes_dev, int32_t depth, int32_t* leaves_dev, int32_t n,
                           int64_t n_items, double beta, float* weights_out_dev, void* stream);
/* priority_i = (mean_k or max_k |td[k][i]| + eps)^alpha as float64, ready for sumtree_set on the same leaves;
 * max_priority_dev[0] (may be NULL) keeps the running maximum (sum_tree.py:18,32 `max_recorded_priority`).           */
int per_priorities_from_td(const float* td_abs_dev, int32_t n_heads, int32_t n, int32_t reduce_max, double eps,
                           double alpha, double* priorities_out_dev, double* max_priority_dev, void* stream);
/* The same from the data-parallel gather td_all_dev [world][K][shard] (idqn_dp_learn_on_replay): priority i = r * shard + j of
 * the global batch is rank r's sample j, so the output is in global-batch order, ready for ONE sumtree_set on the global
 * leaves.  Same mean / max, eps, alpha and running maximum; world == 1 is bit-identical to per_priorities_from_td.           */
int per_priorities_from_td_gathered(const float* td_all_dev, int32_t world, int32_t n_heads, int32_t shard, int32_t reduce_max,
                                    double eps, double alpha, double* priorities_out_dev, double* max_priority_dev, void* stream);
/* per_sample_leaves + per_importance_weights as ONE launch, n in [1, 256]: leaves_out_dev (int32 [n], already clamped to
 * [0, n_items - 1]) and weights_out_dev (float [n]) equal, byte for byte, what the two calls leave there for the same tree and
 * uniforms.  The descents run one wave each over cdiv(n, 4) workgroups; the last workgroup to arrive computes the weights (an
 * arrival counter per stream, owned by the library, made on the stream's first call).                                        */
int per_draw(const double* nodes_dev, int32_t depth, const double* uniforms_dev, int32_t n, int32_t stratified, int64_t n_items,
             double beta, int32_t* leaves_out_dev, float* weights_out_dev, void* stream);
/* per_priorities_from_td + sumtree_set on the same leaves as ONE launch of one workgroup, n in [1, 256]: the node array,
 * max_priority_dev[0] (may be NULL) and priorities_out_dev (float64 [n], may be NULL: the values never leave the chip) equal,
 * byte for byte, the two calls' results -- same sort keys, first occurrence of a duplicate leaf wins, sequential adds per node
 * in ascending-leaf order.  td_abs_dev float [n_heads][n]; scratch_dev as sumtree_set.                                      */
int per_write_back(double* nodes_dev, int32_t depth, const int32_t* leaves_dev, const float* td_abs_dev, int32_t n_heads,
                   int32_t n, int32_t reduce_max, double eps, double alpha, double* priorities_out_dev,
                   double* max_priority_dev, void* scratch_dev, void* stream);
/* One prioritized learner step on the HBM frame ring as ONE call: uniforms -> per_draw -> the replay-sourced step of the
 * handle's family with slots_dev = leaves_dev, the weights and |TD| output in force for this step only -> per_write_back.
 * Handle state (online parameters, moments, count, losses, cum_losses), tree nodes, max_priority_dev, leaves, weights, |TD| and
 * priorities afterwards equal, byte for byte, the chain per_sample_leaves, per_importance_weights, idqn_set_per_buffers, the
 * step, idqn_set_per_buffers(NULL, NULL), per_priorities_from_td, sumtree_set for the same uniforms on the same stream.
 *   uniforms_host: float64 [batch] in [0, 1), ordinary HOST memory, read before the call returns (staged through the pinned
 *     blocks of idqn_learn_steps_on_replay_fc, so calls may follow each other with no synchronisation between them).
 *   The step: idqn_learn_on_replay_dev for plane-path cnn handles, idqn_learn_on_replay_fc_dev for MLP and general-shape cnn
 *     handles (the one-launch MLP step stays one launch), idqn_iqn_learn_on_replay_dev for handles with quantile heads, which
 *     take tau_dev (and batch as their mean divisor).
 * Restrictions (IDQN_E_INVALID otherwise, nothing enqueued, allocated or staged): everything the step's entry refuses; a NULL
 * pointer other than the three marked; batch in [1, min(256, max_batch)]; depth in [1, 31]; n_items >= 1; tau_dev given exactly
 * when the handle has quantile heads; no prioritized-replay buffers set on the handle (idqn_set_per_buffers: the call owns them
 * for its duration and leaves none set); flags IDQN_F_PROFILE / IDQN_F_PROFILE_ALL only.                                     */
typedef struct idqn_per_step {
    double* nodes_dev; int32_t depth; int64_t n_items;
    const double* uniforms_host;   /* [batch] in [0, 1), ordinary HOST memory, read before the call returns */
    int32_t stratified, reduce_max; double beta, eps, alpha;
    double* max_priority_dev;      /* may be NULL */
    int32_t* leaves_dev; float* weights_dev; float* td_abs_dev /* [K][batch] */;
    double* priorities_dev;        /* may be NULL */
    void* tree_scratch_dev;        /* as sumtree_set */
    const float* tau_dev;          /* i-IQN handles: [K][3][N][batch]; NULL otherwise */
} idqn_per_step_t;
int idqn_per_learn_on_replay(idqn_handle_t h, const idqn_per_step_t* per, const uint8_t* frame_ring_dev, int64_t n_frames,
                             int64_t frame_bytes, const int32_t* rows_dev, int32_t batch, int32_t stack,
                             int32_t batch_mean_divisor, uint32_t flags, void* stream);
/* per_write_back on (leaves_dev, td_abs_dev) followed by per_draw on next_uniforms_dev as ONE launch of one workgroup, n in
 * [1, 256] (k_per_turn): between two consecutive prioritized steps the two launches are adjacent, the first is one workgroup
 * and the second must read the tree the first leaves.  The node array, max_priority_dev[0] (may be NULL), priorities_out_dev
 * (may be NULL), next_leaves_out_dev (clamped to [0, n_items - 1]) and next_weights_out_dev afterwards equal, byte for byte,
 * what the two calls leave.  The descents run one wave each, 16 at a time; no arrival counter and no waiting between
 * workgroups: there is one.  Arguments and restrictions: those of per_write_back and per_draw.                              */
int per_turn(double* nodes_dev, int32_t depth, const int32_t* leaves_dev, const float* td_abs_dev, int32_t n_heads, int32_t n,
             int32_t reduce_max, double eps, double alpha, double* priorities_out_dev, double* max_priority_dev, void* scratch_dev,
             const double* next_uniforms_dev, int32_t stratified, int64_t n_items, double beta, int32_t* next_leaves_out_dev,
             float* next_weights_out_dev, void* stream);
/* n_steps consecutive prioritized learner steps on the HBM frame ring as ONE call.  Handle state (online parameters, both
 * moments, count, losses, cum_losses), tree nodes, max_priority_dev and every output row afterwards equal, byte for byte,
 * n_steps calls of idqn_per_learn_on_replay on the rows of uniforms_host on the same stream.  Enqueued: ONE upload of the
 * uniforms, per_draw on row 0, then for every step the replay-sourced step of the handle's family (as idqn_per_learn_on_replay
 * dispatches it; the one-launch MLP step stays one launch per step) on that step's rows, per_turn behind every step but the
 * last, per_write_back behind the last: 2 n_steps + 1 launches around the steps where the single calls make 3 n_steps.
 *   uniforms_host: float64 [n_steps][batch] in [0, 1), ordinary HOST memory, read before the call returns (the handle's pinned
 *     staging blocks, IDQN_STEPS_STAGING_DEPTH of them, each reused only after the launch that read it has finished).
 *   leaves_dev int32 [n_steps][batch], weights_dev float [n_steps][batch], td_abs_dev float [n_steps][K][batch], priorities_dev
 *     float64 [n_steps][batch] (may be NULL): one row per step, each step's row as idqn_per_learn_on_replay leaves it.
 * Restrictions (IDQN_E_INVALID otherwise, nothing enqueued, allocated or staged): handles with quantile heads are not served;
 * n_steps in [1, IDQN_MAX_STEPS_PER_CALL]; everything idqn_per_learn_on_replay refuses; no prioritized-replay buffers set on
 * the handle; flags IDQN_F_PROFILE / IDQN_F_PROFILE_ALL only (with the latter idqn_profile_table lists the launches above
 * as k_per_draw, k_per_turn and k_per_write_back beside the steps' own).                                                    */
typedef struct idqn_per_steps {
    double* nodes_dev; int32_t depth; int64_t n_items;
    const double* uniforms_host;   /* [n_steps][batch] in [0, 1), ordinary HOST memory, read before the call returns */
    int32_t stratified, reduce_max; double beta, eps, alpha;
    double* max_priority_dev;      /* may be NULL */
    int32_t* leaves_dev /* [n_steps][batch] */; float* weights_dev /* [n_steps][batch] */; float* td_abs_dev /* [n_steps][K][batch] */;
    double* priorities_dev;        /* [n_steps][batch]; may be NULL */
    void* tree_scratch_dev;        /* as sumtree_set */
} idqn_per_steps_t;
int idqn_per_learn_steps_on_replay(idqn_handle_t h, const idqn_per_steps_t* per, const uint8_t* frame_ring_dev, int64_t n_frames,
                                   int64_t frame_bytes, const int32_t* rows_dev, int32_t n_steps, int32_t batch, int32_t stack,
                                   int32_t batch_mean_divisor, uint32_t flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * Replay store in HBM (slimdqn/sample_collection/replay_buffer.py:202-230).  The store the product uses is the
 * frame ring described next (frames written once, elements are 8-int32 rows, slot = key % capacity: keys are the
 * monotonically increasing add_count and eviction is FIFO, :206-213); replay_gather further down serves stores that
 * keep whole (state, next_state) pairs per slot.
 * ---------------------------------------------------------------------------------------- */
/* Frame-ring replay store (the layout ReplayBuffer uses): every environment frame is written to HBM once, at ring
 * slot (transition index % n_frames) of frames_dev [n_frames][frame_elems * itemsize]; a replay element is one row
 * of meta_dev, int32 [capacity][8] = {newest state frame slot, valid state frames, newest next_state frame slot,
 * valid next_state frames, action, reward as f32 bits, terminal, 0}.  This call is ReplayBuffer.sample's fetch +
 * unpack + np.stack (replay_buffer.py:223-229) fused with the accumulator's stack building (:119-137,
 * `state[..., ch] = observation`, zero frames before the episode start): for sample i it writes
 * state_out[i][pixel][ch] = frame[newest - (stack-1-ch)][pixel] (0 where fewer than stack frames are valid), the same
 * for next_state, and the three scalars.  Outputs: [n][frame_elems][stack] elements of `itemsize` bytes.            */
int replay_gather_stacked(const uint8_t* frames_dev, int64_t n_frames, int64_t frame_elems, int32_t itemsize,
                          int32_t stack, const int32_t* meta_dev, const int32_t* slots_dev, int32_t n,
                          uint8_t* state_out_dev, uint8_t* next_state_out_dev, int32_t* action_out_dev,
                          float* reward_out_dev, uint8_t* terminal_out_dev, void* stream);
/* Plain row gather of a store that keeps whole (state, next_state) pairs per slot, [capacity][2][obs_bytes]:
 * copies the sampled slots'
 * state / next_state into contiguous [n][obs_bytes] batches.                                       */
int replay_gather(const uint8_t* store_dev, int64_t obs_bytes, const int32_t* slots_dev, int32_t n,
                  uint8_t* state_out_dev, uint8_t* next_state_out_dev, void* stream);
/* Gather of the per-slot scalars kept as arrays [capacity]: action i32, reward f32, terminal u8.   */
int replay_gather_scalars(const int32_t* action_store_dev, const float* reward_store_dev,
                          const uint8_t* terminal_store_dev, const int32_t* slots_dev, int32_t n,
                          int32_t* action_out_dev, float* reward_out_dev, uint8_t* terminal_out_dev,
                          void* stream);
/* ReplayBuffer.add, device half (replay_buffer.py:206-213 keeps transitions on the host): the newest frame, staged in
 * PINNED host memory, is copied asynchronously into slot `slot` of the frame ring in HBM.  The staging slot may be
 * reused once the stream has passed this copy.  The host mirror also sends the new element rows and the sampled slot
 * indices this way (slot 0 of a byte range: frame_ring_dev = destination, frame_bytes = length).                      */
int replay_add_frame(void* frame_ring_dev, int64_t slot, int64_t frame_bytes, const void* frame_host_pinned, void* stream);
/* One vector-environment step of the SEGMENTED frame ring (VectorReplayBuffer; no reference counterpart: the reference collects
 * from one environment): E time lines share one allocation [E * L][frame_bytes], L = S + stack - 1; frame t of environment e goes
 * to slot e * L + (stack - 1) + t % S and, when t % S >= S - (stack - 1), also to the mirror slot e * L + t % S - (S - (stack - 1)),
 * so that every stack is `stack` consecutive slots of one segment and replay_gather_stacked / idqn_learn_on_replay read the ring
 * as they are (n_frames = E * L).  This call replaces E replay_add_frame calls and the row uploads: the caller fills ONE PINNED
 * block, the call copies it asynchronously into block_staging_dev (same size, caller-owned) and ONE launch scatters every frame
 * to its one or two slots and every row to rows_dev.  Block layout, both sides:
 *   int32 [2 * 64]    (source frame index in the block, destination ring slot) pairs, n_writes <= 64 used
 *   int32 [128]       destination element slots, n_rows <= 128 used (the row cap: a step with more rows is split by the caller)
 *   int32 [128][8]    the new rows (replay_gather_stacked documents the row)
 *   uint8 [n_in][frame_bytes] the n_in <= 32 new frames, from byte 5120 on
 * so the block holds 5120 + 32 * frame_bytes bytes and 5120 + n_in * frame_bytes travel.  n_writes + n_rows >= 1.  Frames move
 * 16 B per lane when frame_bytes % 16 == 0 and both buffers are 16-byte aligned, else 4 B, else bytes.  IDQN_E_INVALID before
 * anything is enqueued: a null pointer, a count outside its limit, a source index outside [0, n_in), a ring slot outside
 * [0, n_frames), an element slot outside [0, capacity), a destination named twice.  The pinned block may be refilled once the
 * stream has passed this call.                                                                                               */
int replay_add_step(void* frame_ring_dev, int64_t n_frames, int64_t frame_bytes, int32_t* rows_dev, int64_t capacity,
                    const void* block_host_pinned, void* block_staging_dev, int32_t n_in, int32_t n_writes, int32_t n_rows,
                    void* stream);
/* One lock-step collection of a SEED GROUP (no reference counterpart: the reference starts one process per seed): S SEPARATE
 * ReplayBuffers -- own rings, capacities and row tables, which may differ in frame_bytes, n_frames and capacity -- each take at
 * most one new frame and their pending element rows.  This call replaces the S replay_add_frame calls of the frames and the S to
 * 2 S of the row uploads: the caller fills ONE PINNED block, the call copies `members` to its head, copies block_bytes of it
 * asynchronously into block_staging_dev (caller-owned, at least as large) and ONE launch, grid (work items, S), writes every
 * frame to its ring slot and every row to its table.  Block layout, both sides:
 *   replay_group_member_t [n_members]  from byte 0 (written by the call)
 *   per member, behind the records:    int32 [n_rows] destination element slots + int32 [n_rows][8] the rows, at rows_offset
 *                                      (a multiple of 4; replay_gather_stacked documents the row), n_rows <= 32 (the row cap: a
 *                                      member with more sends them itself first);
 *                                      uint8 [frame_bytes] its new frame at frame_offset (a multiple of 16), if frame_slot >= 0
 * Frames move 16 B per lane when the member's frame_bytes % 16 == 0 and its source and destination are 16-byte aligned, else 4 B,
 * else bytes.  It needs no agent handle and no idqn_group_* object.  IDQN_E_INVALID before anything is enqueued (and before the
 * block is written): a null pointer, n_members outside [1, 32], a block that is not 16-byte aligned, a frame or a row table that
 * is misaligned or leaves [64 * n_members, block_bytes), a frame slot outside [0, n_frames) other than -1, more than 32 rows, an
 * element slot outside [0, capacity) or named twice within a member, two members naming the same ring or the same row table.
 * The pinned block and the staging block may be refilled once the stream has passed this call.                                */
typedef struct replay_group_member_t {
    void* ring_dev;       /* [n_frames][frame_bytes] */
    int32_t* rows_dev;    /* [capacity][8] */
    int64_t n_frames, frame_bytes, capacity;
    int64_t frame_offset; /* byte offset of the new frame in the block */
    int32_t frame_slot;   /* destination ring slot; -1: this member writes no frame */
    int32_t n_rows;
    int64_t rows_offset;  /* byte offset of the row table in the block */
} replay_group_member_t;
int replay_group_add_step(int32_t n_members, const replay_group_member_t* members, void* block_host_pinned,
                          void* block_staging_dev, int64_t block_bytes, void* stream);
/* One vector step of a SEED GROUP whose members are vector buffers: S SEPARATE segmented frame rings (the layout of
 * replay_add_step: E * L slots, mirror slots below a segment's first main slot), which may differ in frame_bytes, n_frames,
 * capacity, E and stack, each take the n_in <= 32 new frames, n_writes <= 64 (source index, destination slot) pairs and
 * n_rows <= 128 element rows of ONE replay_add_step call.  This call replaces those S calls: the caller fills ONE PINNED block, the
 * call copies `members` to its head, copies block_bytes of it asynchronously into block_staging_dev (caller-owned, at least as
 * large) and ONE launch, grid (work items, S), writes every frame to its one or two ring slots and every row to its table.
 * Block layout, both sides:
 *   replay_group_many_member_t [n_members]  from byte 0 (written by the call)
 *   per member, behind the records:         int32 [n_writes][2] (source frame index, destination ring slot) at pairs_offset,
 *                                           int32 [n_rows] destination element slots + int32 [n_rows][8] the rows at rows_offset
 *                                           (both multiples of 4; replay_gather_stacked documents the row);
 *                                           uint8 [n_in][frame_bytes] its new frames at frames_offset (a multiple of 16)
 * Frames move 16 B per lane when the member's frame_bytes % 16 == 0 and source and destination are 16-byte aligned, else 4 B,
 * else bytes.  IDQN_E_INVALID before anything is enqueued (and before the block is written): a null pointer, n_members outside
 * [1, 32], a block that is not 16-byte aligned, a count outside its limit, a member with neither a write nor a row, a table or
 * the frames misaligned or outside [80 * n_members, block_bytes), a source index outside [0, n_in), a ring slot outside
 * [0, n_frames), an element slot outside [0, capacity), a ring slot or an element slot named twice within a member, two members
 * naming the same ring or the same row table.  The pinned block and the staging block may be refilled once the stream has passed
 * this call.                                                                                                                    */
typedef struct replay_group_many_member_t {
    void* ring_dev;        /* [n_frames][frame_bytes] */
    int32_t* rows_dev;     /* [capacity][8] */
    int64_t n_frames, frame_bytes, capacity;
    int32_t n_in, n_writes, n_rows, reserved;
    int64_t pairs_offset;  /* byte offsets in the block: the pair table, */
    int64_t rows_offset;   /* the slot + row table, */
    int64_t frames_offset; /* the new frames */
} replay_group_many_member_t;
int replay_group_add_many(int32_t n_members, const replay_group_many_member_t* members, void* block_host_pinned,
                          void* block_staging_dev, int64_t block_bytes, void* stream);
/* Growth of the frame ring (no reference counterpart: the reference's host dict grows by itself,
 * replay_buffer.py:206-213): the live frames, transition indices [first_t, first_t + count), are copied from slot
 * t % old_n of the old ring to slot t % new_n of the new one (count <= old_n <= new_n, distinct buffers).             */
int replay_ring_regrow(const void* old_ring_dev, int64_t old_n, void* new_ring_dev, int64_t new_n, int64_t first_t,
                       int64_t count, int64_t frame_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDQN_HIP_H */
