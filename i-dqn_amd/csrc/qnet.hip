// Host side of the C ABI for the i-DQN gradient step: layout, workspace, kernel orchestration.
//
// Replaces (reference file:line):
//   iDQN.learn_on_batch          slimdqn/networks/idqn.py:96-109   (jit o vmap of value_and_grad + optax.adam)
//   iDQN.update_target_params    slimdqn/networks/idqn.py:74-94    (copy + shift / sync, as device copies)
//   DQNNet.apply                 slimdqn/networks/architectures/dqn.py:38-70   (cnn, fc; impala: :7-29,54-60, impala_kernels.h)
// One launch sequence per step on the caller's stream; nothing here synchronises with the host.
// Scratch buffers are addressed compactly with the ACTIVE number of 32-sample batch blocks of a call
// (slot = (net * nb + bb) * block); zero borders sit at fixed offsets inside every block-sized slot
// and only interiors are ever written, so they stay zero for any nb.
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>
#include <queue>
#include <functional>

#include <map>
#include <tuple>

#include "act_kernels.h"
#include "act_many_kernels.h"
#include "act_group_args.h"
#include "iqn_act_kernels.h"
#include "iqn_act_many_kernels.h"
#include "cnn_kernels.h"
#include "fc_kernels.h"
#include "fc_par_kernels.h"
#include "fc_steps_kernels.h"
#include "iqn_kernels.h"
#include "gcnn_kernels.h"
#include "impala_kernels.h"
#include "impala_mx_kernels.h"
#include "impala_mx_wgrad_kernels.h"
#include "impala_d0_mx_kernels.h"
#include "fc_act_many_kernels.h"
#include "imp_act_many_kernels.h"
#include "fc_group_kernels.h"
#include "dp_internal.h"
#include "per_step_args.h"
#include "per_group_kernels.h"
#include "convp_fwd_phases.h"
#include "convp_items.h"
#include "staging_ring.h"

namespace {

struct ConvL {
    int K, S, PLh, PLw, CI, CO, IH, IW, OH, OW;
    long w_off, b_off;
};

// CUs the conv launches of the step are planned for (one 512-thread workgroup per CU, all co-resident).  IDQN_CUS < 256
// leaves the rest of the chip to a concurrent stream (the overlapped Dense_0 update, tools/probes/overlap_cumask.py).
// the few run-time switches of the shipped library (INTEGRATION.md lists them)
bool plan_print() { static const bool on = getenv("IDQN_PLAN_PRINT") != nullptr; return on; }  // launch plans to stderr
bool act_generic() { static const bool on = getenv("IDQN_ACT_GENERIC") != nullptr; return on; }  // acting through the batched forward
// the acting entries' two switches, read once per process: IDQN_ACT_POLL=0 collects actions with a device-to-host copy and a
// stream synchronisation instead of the polled mailbox, IDQN_ACT_GRAPH=0 launches eagerly instead of replaying a hipGraph
bool act_no_poll() { static const bool on = getenv("IDQN_ACT_POLL") && atoi(getenv("IDQN_ACT_POLL")) == 0; return on; }
bool act_use_graph() { static const bool on = !(getenv("IDQN_ACT_GRAPH") && atoi(getenv("IDQN_ACT_GRAPH")) == 0); return on; }
// the replay-sourced MLP step's two A/B switches: IDQN_FC_REPLAY_STAGE=1 (read once) sends every batch through the staging launch,
// IDQN_FC_LEARN_STEPS_LOOP=1 (read per call: the bench switches it between its legs) runs an n-step call as n single steps
bool fc_replay_always_stage() { static const bool on = getenv("IDQN_FC_REPLAY_STAGE") && atoi(getenv("IDQN_FC_REPLAY_STAGE")) != 0; return on; }
bool fc_steps_force_loop() { const char* e = getenv("IDQN_FC_LEARN_STEPS_LOOP"); return e && atoi(e) != 0; }

int cu_budget() { return 256; }  // CUs a launch plan may fill

void same_pad(int i, int k, int s, int* out, int* lo, int* hi) {
    *out = (i + s - 1) / s;
    int p = (*out - 1) * s + k - i;
    if (p < 0) p = 0;
    *lo = p / 2;
    *hi = p - *lo;
}

ActGeom make_geom(int H, int W, int C, int lo_h, int hi_h, int lo_w, int hi_w) {
    ActGeom g;
    g.H = H; g.W = W; g.C = C; g.lo_h = lo_h; g.lo_w = lo_w;
    g.Hp = H + lo_h + hi_h; g.Wp = W + lo_w + hi_w;
    g.block = (long)g.Hp * g.Wp * C * 32;
    return g;
}

// zero border a dout buffer needs so that the data-gradient loop never leaves it
void dgrad_pad(int I, int O, int K, int S, int PL, int* lo, int* hi) {
    int mn = 0, mx = O - 1;
    for (int i = 0; i < I; ++i)
        for (int k = 0; k < K; ++k) {
            int t = i + PL - k;
            if (((t % S) + S) % S) continue;
            int o = t >= 0 ? t / S : -((-t) / S);
            if (o < mn) mn = o;
            if (o > mx) mx = o;
        }
    *lo = -mn;
    *hi = mx - (O - 1);
}

struct Layout {
    int n_leaves = 0;
    idqn_leaf_t leaves[IDQN_MAX_LEAVES];
    long head_stride = 0;
};

void add_leaf(Layout& L, const char* name, int ndim, const long* shape, long* off) {
    idqn_leaf_t& lf = L.leaves[L.n_leaves++];
    memset(&lf, 0, sizeof(lf));
    snprintf(lf.name, sizeof(lf.name), "%s", name);
    lf.ndim = ndim;
    long n = 1;
    for (int i = 0; i < ndim; ++i) { lf.shape[i] = shape[i]; n *= shape[i]; }
    lf.offset = *off;
    *off += (n + 63) / 64 * 64;  // every leaf starts on a 256-byte boundary
}

const int KS[3][2] = {{8, 4}, {4, 2}, {3, 1}};  // (kernel, stride) of Conv_0..2, architectures/dqn.py:43-51

// Shapes the MFMA plane kernels (and the f32-MFMA conv kernels) are built for; every other cnn shape the reference's
// DQNNet accepts runs on the general-shape kernels (gcnn_kernels.h).  IDQN_CNN_GENERAL=1 forces those (tests).
bool cnn_fast_shape(const idqn_config_t& c) {
    static const bool force_general = getenv("IDQN_CNN_GENERAL") && atoi(getenv("IDQN_CNN_GENERAL")) != 0;
    if (c.n_quantiles > 0) return true;  // the i-IQN heads exist on the MFMA path only (its checks reject other shapes)
    if (force_general) return false;
    if (c.n_features != 4 || c.obs_c != 4 || c.obs_h < 8 || c.obs_w < 8 || c.n_actions > 32) return false;
    for (int i = 0; i < 3; ++i)
        if (c.features[i] != 32 && c.features[i] != 64) return false;
    return c.features[3] % 128 == 0 && c.features[3] >= 128 && c.features[3] <= 512;
}

int build_layout(const idqn_config_t& c, Layout& L) {
    IDQN_REQUIRE(c.n_heads >= 1 && c.n_actions >= 1 && c.n_actions <= 4096, "n_heads >= 1 and 1 <= n_actions <= 4096 required");
    IDQN_REQUIRE(c.n_features >= 1 && c.n_features <= IDQN_MAX_FEATURES, "n_features out of range");
    IDQN_REQUIRE(c.max_batch >= 1, "max_batch must be positive");
    IDQN_REQUIRE(c.n_quantiles >= 0 && c.n_quantiles <= 64, "n_quantiles must be in [0, 64]");
    IDQN_REQUIRE(c.n_quantiles == 0 || (c.arch == IDQN_ARCH_CNN && c.max_batch <= 256),
                 "i-IQN heads are built for the cnn arch and minibatches of at most 256 samples (max_batch %d)", c.max_batch);
    long off = 0;
    char nm[32];
    if (c.arch == IDQN_ARCH_CNN && !cnn_fast_shape(c)) {
        // general shape: three convs for features[0..2], Dense + ReLU for every features[3:], Dense(n_actions)
        // (architectures/dqn.py:39-53,65-70)
        IDQN_REQUIRE(c.n_quantiles == 0, "i-IQN heads need a shape the MFMA kernels are built for");
        IDQN_REQUIRE(c.n_features >= 3, "cnn: at least 3 features (the three convs), got %d", c.n_features);
        IDQN_REQUIRE(c.obs_h >= 1 && c.obs_w >= 1 && c.obs_c >= 1, "cnn: empty observation");
        int h = c.obs_h, w = c.obs_w, ch = c.obs_c;
        for (int i = 0; i < 3; ++i) {
            IDQN_REQUIRE(c.features[i] >= 1, "cnn: conv width %d", c.features[i]);
            long ks[4] = {KS[i][0], KS[i][0], ch, c.features[i]};
            snprintf(nm, sizeof nm, "Conv_%d/kernel", i);
            add_leaf(L, nm, 4, ks, &off);
            long bs[1] = {c.features[i]};
            snprintf(nm, sizeof nm, "Conv_%d/bias", i);
            add_leaf(L, nm, 1, bs, &off);
            int lo, hi;
            same_pad(h, KS[i][0], KS[i][1], &h, &lo, &hi);
            same_pad(w, KS[i][0], KS[i][1], &w, &lo, &hi);
            ch = c.features[i];
        }
        long fan = (long)h * w * ch;
        for (int i = 3; i <= c.n_features; ++i) {
            long f = i < c.n_features ? c.features[i] : c.n_actions;
            IDQN_REQUIRE(f >= 1, "cnn: dense width %ld", f);
            long ws[2] = {fan, f};
            snprintf(nm, sizeof nm, "Dense_%d/kernel", i - 3);
            add_leaf(L, nm, 2, ws, &off);
            long bs[1] = {f};
            snprintf(nm, sizeof nm, "Dense_%d/bias", i - 3);
            add_leaf(L, nm, 1, bs, &off);
            fan = f;
        }
    } else if (c.arch == IDQN_ARCH_CNN) {
        IDQN_REQUIRE(c.n_actions <= 32, "cnn (MFMA path): n_actions <= 32");
        IDQN_REQUIRE(c.n_features == 4, "cnn: exactly 4 features (three convs + one hidden dense) are built; got %d", c.n_features);
        IDQN_REQUIRE(c.obs_c == 4, "cnn: obs_c must be 4 (Conv_0 packs (kw, c) into 32 rows), got %d", c.obs_c);
        IDQN_REQUIRE(c.obs_h >= 8 && c.obs_w >= 8, "cnn: observation smaller than the first kernel");
        for (int i = 0; i < 3; ++i)
            IDQN_REQUIRE(c.features[i] == 32 || c.features[i] == 64, "cnn: conv features must be 32 or 64, got %d", c.features[i]);
        IDQN_REQUIRE(c.features[3] % 128 == 0 && c.features[3] >= 128 && c.features[3] <= 512,
                     "cnn: dense width must be a multiple of 128 in [128, 512], got %d", c.features[3]);
        int h = c.obs_h, w = c.obs_w, ch = c.obs_c;
        for (int i = 0; i < 3; ++i) {
            long ks[4] = {KS[i][0], KS[i][0], ch, c.features[i]};
            snprintf(nm, sizeof nm, "Conv_%d/kernel", i);
            add_leaf(L, nm, 4, ks, &off);
            long bs[1] = {c.features[i]};
            snprintf(nm, sizeof nm, "Conv_%d/bias", i);
            add_leaf(L, nm, 1, bs, &off);
            int lo, hi;
            same_pad(h, KS[i][0], KS[i][1], &h, &lo, &hi);
            same_pad(w, KS[i][0], KS[i][1], &w, &lo, &hi);
            ch = c.features[i];
        }
        long d0[2] = {(long)h * w * ch, c.features[3]};
        add_leaf(L, "Dense_0/kernel", 2, d0, &off);
        long b0[1] = {c.features[3]};
        add_leaf(L, "Dense_0/bias", 1, b0, &off);
        long d1[2] = {c.features[3], c.n_actions};
        add_leaf(L, "Dense_1/kernel", 2, d1, &off);
        long b1[1] = {c.n_actions};
        add_leaf(L, "Dense_1/bias", 1, b1, &off);
        if (c.n_quantiles > 0) {  // i-IQN heads (extension): the quantile embedding, phi(tau) = relu(Embed_0(cos(pi i tau)))
            long es[2] = {IQN_EMBED, d0[0]};
            add_leaf(L, "Embed_0/kernel", 2, es, &off);
            long eb[1] = {d0[0]};
            add_leaf(L, "Embed_0/bias", 1, eb, &off);
        }
    } else if (c.arch == IDQN_ARCH_FC) {

        long fan = (long)c.obs_h * c.obs_w * c.obs_c;
        for (int i = 0; i <= c.n_features; ++i) {
            long f = i < c.n_features ? c.features[i] : c.n_actions;
            IDQN_REQUIRE(f >= 1 && fan >= 1, "fc: layer widths must be positive");  // (wider than FC_MAX_WIDTH: the generic kernels)
            long ws[2] = {fan, f};
            snprintf(nm, sizeof nm, "Dense_%d/kernel", i);
            add_leaf(L, nm, 2, ws, &off);
            long bs[1] = {f};
            snprintf(nm, sizeof nm, "Dense_%d/bias", i);
            add_leaf(L, nm, 1, bs, &off);
            fan = f;
        }
    } else if (c.arch == IDQN_ARCH_IMPALA) {
        // three Stacks of five 3x3 convs (flax numbers them Conv_0..4), Dense + ReLU for every features[3:], Dense(n_actions)
        // (architectures/dqn.py:7-29,54-60)
        IDQN_REQUIRE(c.n_quantiles == 0, "impala: the i-IQN heads are built for the cnn arch");
        IDQN_REQUIRE(c.n_features >= 3, "impala: at least 3 features (the three Stacks), got %d", c.n_features);
        IDQN_REQUIRE(c.obs_h >= 1 && c.obs_w >= 1 && c.obs_c >= 1, "impala: empty observation");
        int h = c.obs_h, w = c.obs_w, ch = c.obs_c;
        for (int s = 0; s < 3; ++s) {
            IDQN_REQUIRE(c.features[s] >= 1, "impala: Stack width %d", c.features[s]);
            for (int i = 0; i < 5; ++i) {
                long ks[4] = {3, 3, i == 0 ? ch : c.features[s], c.features[s]};
                snprintf(nm, sizeof nm, "Stack_%d/Conv_%d/kernel", s, i);
                add_leaf(L, nm, 4, ks, &off);
                long bs[1] = {c.features[s]};
                snprintf(nm, sizeof nm, "Stack_%d/Conv_%d/bias", s, i);
                add_leaf(L, nm, 1, bs, &off);
            }
            h = (h + 1) / 2; w = (w + 1) / 2; ch = c.features[s];
        }
        long fan = (long)h * w * ch;
        for (int i = 3; i <= c.n_features; ++i) {
            long f = i < c.n_features ? c.features[i] : c.n_actions;
            IDQN_REQUIRE(f >= 1, "impala: dense width %ld", f);
            long ws[2] = {fan, f};
            snprintf(nm, sizeof nm, "Dense_%d/kernel", i - 3);
            add_leaf(L, nm, 2, ws, &off);
            long bs[1] = {f};
            snprintf(nm, sizeof nm, "Dense_%d/bias", i - 3);
            add_leaf(L, nm, 1, bs, &off);
            fan = f;
        }
    } else {
        IDQN_REQUIRE(false, "unknown arch %d (0 = cnn, 1 = fc, 2 = impala)", c.arch);
    }
    L.head_stride = off;
    return IDQN_OK;
}

// One set of nets that run forward together: the 2K training nets, or the single inference net.
struct NetSet {
    int n_nets = 0, nb_cap = 0, n_in_sets = 0;
    int NS = 0;  // split-K of this set's Dense_0 forward
    long part_slabs = 0;  // (block, split) slabs the partial buffer holds per net
    const float** wbase = nullptr;  // dev [n_nets]
    int* in_set = nullptr;          // dev [n_nets] input set read by Conv_0
    int* ident = nullptr;           // dev [n_nets] 0..n_nets-1 (later layers read their own activations)
    float *x = nullptr, *a1 = nullptr, *a2 = nullptr, *a3 = nullptr, *part = nullptr;  // x, a1, a2: f32 conv path only
    unsigned short *x1 = nullptr, *a1p = nullptr, *a2p = nullptr, *wq = nullptr;       // plane conv path (convp.h)
};

// host-side plans of the plane conv launches: the work items of a launch depend only on geometry, net count and batch
// blocks, so they are built once and kept on the device
struct FwdPlan { int n_items = 0, NT = 0, ring = 2, items_per_slot = 0, r_begin[4] = {0, 0, 0, 0}, r_cnt[4] = {1, 1, 1, 1}; size_t stage = 0, lds = 0;
                 int row_parts = 0, n_wg = 0; CItem* items_dev = nullptr;  // row_parts > 0: a plan of the persistent kernel (convp_pp.hip), n_wg workgroups
                 CFwdDesc* desc_dev = nullptr; };  // one-item plans: the item table (convp_items.h), made with the plan, handle-owned
struct WgradPlan { int n_items = 0, n_chunks = 0, chunk_major = 0, MT = 0, PG = 0; size_t lds = 0; };

// workspace of the i-IQN heads (iqn_kernels.h): V = 3K virtual nets x NB = N x nb blocks (fraction q of sample block s
// at block s N + q), sized for nb_max = ceil(max_batch / 32) sample blocks
struct IqnWs {
    int N = 0, V = 0, NS = 2, nb_max = 1;
    const float** wbase_v = nullptr;  // dev [V]: online k | target k | target k
    unsigned short* cosa = nullptr;  // A-fragment planes of the cos blocks [V * N][12][512]
    unsigned short *cosp = nullptr, *wep = nullptr;  // bf16 fragment planes of the cos blocks [V * N][12][512] and of We [2K][F / 32][12][512]
    float *xq = nullptr, *part = nullptr, *hbuf = nullptr, *qpart = nullptr, *dq = nullptr, *dh = nullptr,
          *dx = nullptr, *dpsi = nullptr, *dbg = nullptr, *z = nullptr;
    int QG = 1;              // fraction groups of the embedding backward (partials dpsi / gpart)
    float* gpart = nullptr;  // [QG][K][65][F]
    int HG = 1;              // fraction groups of k_iqn_dh (partials hpart)
    float* hpart = nullptr;  // [HG][K][J * A + J + A]
    float* clk = nullptr;  // IDQN_IQN_CLOCK=1: clock stamps of the forward GEMM's workgroups [<= 1024][4] int64 (debug buffer "iqn_clk")
    // per sample-block count nb (index nb - 1): dispatch order of the merged Dense_0 gradient launch with Adam in its epilogue
    // (plan_iqn_bwd_order), its workgroup count, and whether the planner's makespan prefers it to the two-split launch + Adam pass
    int32_t* bwd_items[8] = {};
    int bwd_blocks[8] = {};
    bool bwd_fuse[8] = {};
    float* lpart = nullptr;  // [K][nb]: per-sample-block loss partials (k_iqn_loss, nb > 1)
    unsigned* gate = nullptr;  // [2 * K * ceil(F / 256) + 64]: IqnD0Gate (arrived, passed, err) of the fused Dense_0 update
    bool d0_adam_done = false;  // this step's merged gradient launch updated Dense_0/kernel itself
    float* g1 = nullptr;  // second partial of the Dense_0 weight gradient [K][F * J] (iqn_gemm.h), N a multiple of 16 only
    long off_we = 0, off_be = 0;
};

// workspace of the general-shape cnn path (gcnn_kernels.h): NHWC f32 activations of the 2K nets, their gradients for the K
// online nets, and the dense head as an FcNet over the flattened conv features
struct GcnnWs {
    bool on = false;
    int Bmax = 0;
    float *act[3] = {nullptr, nullptr, nullptr};   // [2K][Bmax][OH][OW][CO] of Conv_0..2 (act[2] flattened = the head's input)
    float *dact[3] = {nullptr, nullptr, nullptr};  // [K][Bmax][...]: gradient w.r.t. the pre-activation of Conv_0..2
    float *inf_act[3] = {nullptr, nullptr, nullptr};  // one net, 32 states (acting)
    float* inf_ws = nullptr;
};

// workspace of the impala path (impala_kernels.h).  Per Stack s and image: c0 = Conv_0's output [H][W][CO], x[0] = the pool's
// output, y[blk] = relu(Conv_{1+2blk}(relu(x[blk]))), x[blk + 1] = Conv_{2+2blk}(y[blk]) + x[blk], all [PH][PW][CO];
// x[2] is the Stack's output (Stack 2: after the final ReLU, i.e. the dense head's input).
struct ImpActs { float *c0[3], *x[3][3], *y[3][2]; };
struct ImpStackL { int H, W, CI, CO, PH, PW, lo_h, lo_w; long w_off[5], b_off[5]; };
struct ImpalaWs {
    bool on = false;
    bool mx = false;  // IDQN_IMP_CONV=bf16x3: eligible convs (imx_eligible) run on k_imp_conv_mx, forward and data gradient
    int Bmax = 0;
    ImpStackL st[3];
    ImpActs train, infer;  // the 2K training nets x Bmax samples; one net x 32 states (acting)
    float *d[3] = {nullptr, nullptr, nullptr};    // [K][Bmax][PH][PW][CO]: gradient of the Stack's running x
    float *t[3] = {nullptr, nullptr, nullptr};    // same shape: gradient of y (the inner conv's output)
    float *dc0[3] = {nullptr, nullptr, nullptr};  // [K][Bmax][H][W][CO]: gradient of Conv_0's output
    bool wmx = false;  // IDQN_IMP_WGRAD=bf16x3: the same layers' weight gradients run on k_imp_wgrad_mx
    float* wpart = nullptr;  // weight-gradient partials of one conv [K][chunks][9 CI CO + CO] (sized for the largest)
    float* inf_ws = nullptr;
    // a head with a hidden layer: Dense_0 runs on the k_imp_d0_* kernels, k_fc_step on the layers behind it (`tail`)
    bool d0_split = false;
    bool d0mx = false;  // IDQN_IMP_D0=mfma: that forward runs on k_imp_d0_fwd_mx (the same bytes; imp_d0_forward)
    FcNet tail;
    float* hid = nullptr;   // [2K][Bmax][D]  relu(Dense_0)
    float* dhid = nullptr;  // [K][Bmax][D]   dL/d(pre-activation of Dense_0)
    float* inf_hid = nullptr;  // [32][D]     relu(Dense_0) of the acting net
};

}  // namespace

// Buffers, mailbox and counters of the many-state acting entries: idqn_act_host_many (act_many_kernels.h), idqn_act_host_many_fc
// (fc_act_many_kernels.h) and idqn_iqn_act_host_many (iqn_act_many_kernels.h).  A handle is in the domain of exactly one of the
// three, so it carries ONE slot, filled by act_many_alloc on that entry's first call.  Nothing here is shared with the
// single-state path but the capture stream.
struct ActManySlot {
    uint8_t* pin = nullptr;    // pinned block {head, states [32][state bytes]} (hipHostMalloc)
    uint8_t* block = nullptr;  // its device copy, uploaded by the chain's one copy node
    size_t head_bytes = 0;     // sizeof(ActManyTable), or sizeof(IqnActManyBlock): the table and tau [32][64]
    float* ws = nullptr;       // ONE allocation, carved into:
    float* a[3] = {nullptr, nullptr, nullptr};  // conv activations [32][..] (cnn handles)
    // cnn: Dense_0 partials [32][NRG][J]; fc: the dense ping-pong rows [32][2][dmax]; i-IQN: [32][NRG][J / 32][2][NP][16]
    float* part = nullptr;
    float *cos = nullptr, *x = nullptr;  // i-IQN only: [32][64][64], [32][F][NP]
    int32_t* action = nullptr;    // [32]
    int32_t* mail = nullptr;      // host mailbox {action[32], sequence} (mapped + coherent)
    int32_t* mail_dev = nullptr;  // its device address
    unsigned* ctr = nullptr;      // device side: {sequence number, finished workgroups}
    unsigned expected = 0;        // sequence number the next call waits for
    std::map<std::tuple<int, void*, void*>, hipGraphExec_t> graphs;  // (n, q out, host actions)

    // what act_many_alloc's `owned` does not hold: the graphs and the two host blocks (the destroy functions, device idle)
    void release() {
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
        if (mail) (void)hipHostFree(mail);
        if (pin) (void)hipHostFree(pin);
    }
};

struct idqn_handle_s {
    idqn_config_t cfg;
    Layout L;
    float *online, *target, *mu, *nu, *grad, *losses;
    int32_t* count;
    double* cum;
    AdamConsts ad;
    float gamma_n;
    int nb_max;
    // cnn
    ConvL conv[3];
    ActGeom gx, ga1, ga2, ga3, gda3, gda2, gda1;
    int F = 0, J = 0, NS = 0;
    long off_w0 = 0, off_b0 = 0, off_w1 = 0, off_b1 = 0;
    NetSet train, infer;
    IqnWs iqn;
    GcnnWs gc;
    ImpalaWs imp;
    float* dpart = nullptr;  // partial Dense_0 data gradients of the fused weight-gradient kernel [n_jt][K * nb][F][32]
    float *da3 = nullptr, *da2 = nullptr, *da1 = nullptr, *qdbg = nullptr, *slab = nullptr;
    float *hbuf = nullptr, *qpart = nullptr, *bcinv = nullptr;
    float *act_a[3] = {nullptr, nullptr, nullptr}, *act_part = nullptr;  // single-state acting path (act_kernels.h)
    hipStream_t act_stream = nullptr;  // capture stream of the acting graphs
    uint8_t* act_state = nullptr;     // the state of idqn_act_host on the device
    int32_t* act_action = nullptr;
    int32_t* act_mail = nullptr;      // host mailbox {action, sequence} (hipHostMalloc, mapped + coherent) of idqn_act_host
    int32_t* act_mail_dev = nullptr;  // its device address
    unsigned* act_seq = nullptr;      // device-side sequence counter
    unsigned act_expected = 0;        // sequence number the next idqn_act_host call waits for
    bool act_use_mail = false;        // set while idqn_act_host issues / captures its launches
    int act_pending = 0;              // idqn_act_host_begin launched, idqn_act_host_end has not collected yet (1 mailbox, 2 copy)
    // IDQN_STEP_GRAPH=1: the plain cnn step replayed as a hipGraph per (batch buffers, size); value = calls seen, graph
    std::map<std::tuple<const void*, const void*, const void*, const void*, const void*, int, int, const void*, const void*>,
             std::pair<int, hipGraphExec_t>> step_graphs;
    std::map<std::tuple<int, const void*, void*, void*>, hipGraphExec_t> act_graphs;  // (net, host state, q out, host action)
    // idqn_iqn_act_host (iqn_act_kernels.h): fractions, their cosines [N][64], x [F][NP], Dense_0 partials [NRG][J / 32][2][NP][16]
    float *iact_tau = nullptr, *iact_cos = nullptr, *iact_x = nullptr, *iact_part = nullptr;
    std::map<std::tuple<int, const void*, const void*, void*, void*>, hipGraphExec_t> iact_graphs;  // (net, state, fractions, q out, action)
    ActManySlot many;  // the handle's many-state acting entry
    const float* infer_pbase = nullptr;  // parameter base of the net the last idqn_q_values call evaluated
    float *infer_hbuf = nullptr, *infer_qpart = nullptr;  // k_hidden outputs of the single inference net
    float* wt[3] = {nullptr, nullptr, nullptr};  // transformed weights of the Conv_1 / Conv_2 data gradients
    long wt_stride[3] = {0, 0, 0};
    // plane conv path (convp.h; the default): packed weight planes per net, plane dout buffers, per-position dy sums
    bool planes = true;
    unsigned short *da3p = nullptr, *da2p = nullptr, *da1p = nullptr;
    int dh_nb = 0;  // batch blocks of the step that last wrote dL/dh (debug buffer "dh")
    unsigned short* fact_planes = nullptr;  // bf16 planes of the gathered Dense_0 factors (factored data-parallel step)
    long fact_planes_cap = 0;               // in sample blocks
    float* pbuf[3] = {nullptr, nullptr, nullptr};  // [K * nb][OH * OW][CO] of conv layer i
    long wq_stride = 0, wq_fwd[3] = {0, 0, 0}, wq_dg[3] = {0, 0, 0};  // bytes
    std::map<std::tuple<int, int, int, int>, FwdPlan> fwd_plans;  // (role, n_nets, nb, target workgroups)
    std::map<std::tuple<int, int, int>, WgradPlan> wgrad_plans;   // (layer, nb, position chunks)
    int npc_used[3] = {0, 0, 0};  // position chunks (= slabs per head) the weight-gradient launches of THIS step wrote
    int n_cus = 256;  // CUs of the device
    float* td_bpart = nullptr;   // [K * J / 32][nb][TD_BPART] per-block gradient partials of k_td_dh (max_batch > 32)
    unsigned* td_bctr = nullptr;
    float* cprof = nullptr;  // debug (IDQN_CONV_PROF=role): phase stamps of one plane conv launch
    int cprof_role = -1;
    int npc[3], pos_per_chunk[3];
    long slab_stride[3], slab_off[3];
    SlabSeg segs[3];  // slab descriptors of the last backward (consumed by the fused Adam launch)
    // fc
    FcNet fc;
    float* fc_ws = nullptr;
    FcPlan fc_plan_;  // LDS plan of k_fc_step_lds (BS = 0: the net does not fit and the generic kernel runs)
    FcMfmaPlan fcm_plan_;  // LDS plan of k_fc_step_mfma (floats = 0: neither the staged-weights nor the global-weights layout fits)
    bool fcm_global_ = false;  // the plan is fc_mfma_plan_g: weight operands from global memory
    FcParPlan fcp_plan_;  // LDS plan of k_fc_step_par (floats = 0: does not fit); batches of <= 32 samples run it
    FcParPlan fcs_plan_;  // LDS plan of k_fc_steps_par (fc_steps_kernels.h; floats = 0: idqn_learn_steps_on_replay_fc loops over the single step)
    // slot staging of idqn_learn_steps_on_replay_fc (host form) and the uniforms of the prioritized entries (staging_ring.h)
    StagingRing steps;
    // timeline of a whole step (IDQN_F_PROFILE_ALL): one event after every launch; idqn_profile_table averages per name
    std::vector<hipEvent_t> tl_ev;
    std::vector<const char*> tl_name;
    int tl_used = 0;
    bool tl_on = false;
    // profiling of the dominant kernel
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
    const char* dominant = "";
    // Gradient arena layout: [K][gP] small leaves (every leaf but the cnn's Dense_0/kernel, same order, per-head
    // stride gP = P - w0n), 64 floats reserved for the caller (losses), then [K][w0n] Dense_0/kernel gradients.
    // Two contiguous regions = two collectives in the data-parallel step.  fc: w0n = 0, gP = P.
    long gP = 0, g_w0_begin = 0, g_w0_end = 0, g_w0_base = 0;
    // replay-sourced step (idqn_learn_on_replay): the staging launch gathers from the ring (StepIn, below) into these
    int32_t* rp_action = nullptr;   // [max_batch] scalars of the sampled rows, written by the staging launch
    float* rp_reward = nullptr;
    uint8_t* rp_terminal = nullptr;
    // replay-sourced step of the fc / general-shape cnn handles (idqn_learn_on_replay_fc; replay_src_kernels.h): the staging
    // launch's stacked minibatches [max_batch][obs]
    void *rp_state = nullptr, *rp_next = nullptr;
    // prioritized-replay extension: written by idqn_set_per_buffers only, read where a public learner entry fills its StepIn
    const float* is_weight = nullptr;
    float* td_abs = nullptr;
    bool d0_rows = false;  // the last fused Dense_0 launch (pairs of column tiles) finished dL/da3 itself
    bool wt_ready = false;  // the data-gradient kernels of this step are built (k_td_dh_wt)
    bool pend_profile = false;
    int pend_stage = 0;  // 1: stopped before the Dense_0 weight gradient, 2: stopped after it
    int pend_B = 0;  // batch of a backward stopped after Dense_0 (idqn_backward_rest resumes it); 0 = none
    std::vector<void*> owned;
    std::vector<std::pair<std::string, std::pair<void*, long>>> dbg;
};

namespace {

// What ONE gradient step is told beside the handle: every learner entry fills one and hands it to learn_step.
// The minibatch is either five device tensors, or (`frames` set) the replay frame ring with the sampled element slots -- then
// action / reward / terminal (and, on the MLP staging route, state / next_state) name handle-owned buffers (h->rp_*) that the
// step's first launch fills.  Only that FIRST launch reads the ring, the rows and the slots (the staging launch of cnn_forward,
// k_rps_stage, or k_fc_step_par with the ring as its source); everything after it -- on a split step (IDQN_F_STOP_*) the rest
// that idqn_backward_rest / idqn_finish_step_factored enqueue later included -- reads the handle-owned copies.  So a StepIn is a
// stack local of the entry, dropped on return, and the later calls need nothing of it.
struct StepIn {
    const char* fn = "";  // the entry's name, for messages
    int batch = 0, mean_divisor = 0;
    uint32_t flags = 0;
    const void *state = nullptr, *next_state = nullptr;
    const int32_t* action = nullptr;
    const float* reward = nullptr;
    const uint8_t* terminal = nullptr;
    // the frame ring as the source (frames != nullptr); exactly one of slots_dev (int32 [batch] on the device) and slots_host
    // (read before the call returns: the first launch takes them by value, slot_block) is set
    const void* frames = nullptr;
    const int32_t* rows = nullptr;
    long n_frames = 0, frame_bytes = 0;
    int stack = 0;
    const int32_t *slots_dev = nullptr, *slots_host = nullptr;
    const float* tau = nullptr;  // the fractions of a quantile step (selects iqn_learn)
    // importance weights and |TD| output of THIS step: a public entry copies h->is_weight / h->td_abs, the prioritized driver
    // names the step's own rows
    const float* is_weight = nullptr;
    float* td_abs = nullptr;

    bool stop0() const { return flags & IDQN_F_STOP_AFTER_DENSE0; }
    bool stopb() const { return flags & IDQN_F_STOP_BEFORE_DENSE0_WGRAD; }
    bool grads_only() const { return (flags & IDQN_F_GRADS_ONLY) || stop0() || stopb(); }
    bool profile() const { return flags & IDQN_F_PROFILE; }
    template <class Slots>  // StageSlots, RpsSlotsPar
    Slots slot_block() const {
        Slots s = {};
        memcpy(s.slot, slots_host, (size_t)batch * 4);
        return s;
    }
};

int alloc_zero(float** p, long n_floats, idqn_handle_s* h, const char* name) {
    IDQN_HIP_CHECK(hipMalloc((void**)p, (size_t)n_floats * 4));
    IDQN_HIP_CHECK(hipMemset(*p, 0, (size_t)n_floats * 4));
    h->owned.push_back((void*)*p);
    h->dbg.push_back({name, {(void*)*p, n_floats * 4}});
    return IDQN_OK;
}

int alloc_zero16(unsigned short** p, long n, idqn_handle_s* h, const char* name) {
    IDQN_HIP_CHECK(hipMalloc((void**)p, (size_t)n * 2));
    IDQN_HIP_CHECK(hipMemset(*p, 0, (size_t)n * 2));
    h->owned.push_back((void*)*p);
    h->dbg.push_back({name, {(void*)*p, n * 2}});
    return IDQN_OK;
}

// dL/dh [K][nb][J][32] of a batch of nb blocks: ends where the training set's a3 begins (netset_alloc)
float* dh_of(idqn_handle_s* h, int nb) {
    h->dh_nb = nb;
    return h->train.a3 - (long)h->cfg.n_heads * nb * h->J * 32;
}

// step timeline: an event on the stream after the launch just made (name = nullptr: start of a step)
void tl_mark(idqn_handle_s* h, hipStream_t q, const char* name) {
    if (!h->tl_on || h->tl_used >= (int)h->tl_ev.size()) return;
    if (hipEventRecord(h->tl_ev[h->tl_used], q) != hipSuccess) return;
    h->tl_name[h->tl_used++] = name;
}

// the timeline is on for a call made with IDQN_F_PROFILE_ALL (its events are made on the first such call); the start marker
int tl_begin(idqn_handle_s* h, uint32_t flags, hipStream_t q) {
    h->tl_on = (flags & IDQN_F_PROFILE_ALL) != 0;
    if (h->tl_on && h->tl_ev.empty()) {
        h->tl_ev.resize(2048);
        h->tl_name.resize(2048);
        for (auto& e : h->tl_ev) IDQN_HIP_CHECK(hipEventCreate(&e));
    }
    tl_mark(h, q, nullptr);
    return IDQN_OK;
}

// The online nets' Dense_0 kernels are streamed three times per step (forward; fused update: read and written).  While they fit the
// 256 MB memory-side cache beside the step's other traffic -- K * F * J * 4 <= 84 MB: K <= 5 at the Nature width -- the forward reads
// them and the update stores them with the default policy, so that part of them is found on chip again; everything read or written
// once per step (target nets, m, v) stays non-temporal.  More heads: every stream non-temporal, as in rounds 3-4 (the dirty lines
// of a set that cannot stay only get in the way: K = 6 the same, K = 8 +13 us; keeping only the 4-5 heads that would fit: no better
// than none -- profiles/r5_d0_keep_online_ab.txt).
int d0_keep_heads(const idqn_handle_s* h) {
    return (long)h->cfg.n_heads * h->F * h->J * 4 <= 84L << 20 ? h->cfg.n_heads : 0;
}
bool d0_keep_online(const idqn_handle_s* h) { return d0_keep_heads(h) >= h->cfg.n_heads; }  // every head's kernel fits

// k-splits of the Dense_0 forward of `n_nets` nets x `nb` sample blocks: as many 4-wave workgroups as CUs, never more (a 257th
// would stream alone after the others), with balanced splits of the F / 32 row units (cnn_setup has the reasoning)
int d0_splits(const idqn_handle_s* h, int n_nets, int nb) {
    const int ns = 256 * 4 / std::max(1, n_nets * nb * (h->J / 128));
    return std::max(1, std::min(std::min(ns, 64), h->F / 32));
}

int netset_alloc(idqn_handle_s* h, NetSet& s, int n_nets, int nb, int n_in_sets, const char* tag, int units_per_split = 0) {
    s.n_nets = n_nets; s.nb_cap = nb; s.n_in_sets = n_in_sets;
    s.NS = h->NS;
    if (units_per_split > 0) {  // a single acting net: more, shorter splits (each wave's MFMA chain is the latency)
        const int units = h->F / 32;
        s.NS = (units + units_per_split - 1) / units_per_split;
    }
    IDQN_HIP_CHECK(hipMalloc((void**)&s.wbase, sizeof(float*) * n_nets));
    IDQN_HIP_CHECK(hipMalloc((void**)&s.in_set, sizeof(int) * n_nets));
    IDQN_HIP_CHECK(hipMalloc((void**)&s.ident, sizeof(int) * n_nets));
    h->owned.push_back((void*)s.wbase); h->owned.push_back((void*)s.in_set); h->owned.push_back((void*)s.ident);
    std::vector<int> id(n_nets);
    for (int i = 0; i < n_nets; ++i) id[i] = i;
    IDQN_HIP_CHECK(hipMemcpy(s.ident, id.data(), sizeof(int) * n_nets, hipMemcpyHostToDevice));
    std::string t(tag);
    int rc;
    if (h->planes) {  // bf16 planes: one for the pixels, three per activation (block = rows x 32 samples)
        if ((rc = alloc_zero16(&s.x1, (long)n_in_sets * nb * h->gx.block, h, (t + "x1").c_str()))) return rc;
        if ((rc = alloc_zero16(&s.a1p, (long)n_nets * nb * h->ga1.block * 3, h, (t + "a1p").c_str()))) return rc;
        if ((rc = alloc_zero16(&s.a2p, (long)n_nets * nb * h->ga2.block * 3, h, (t + "a2p").c_str()))) return rc;
        if ((rc = alloc_zero16(&s.wq, (long)n_nets * h->wq_stride / 2, h, (t + "wq").c_str()))) return rc;
    } else {
        if ((rc = alloc_zero(&s.x, (long)n_in_sets * nb * h->gx.block, h, (t + "x").c_str()))) return rc;
        if ((rc = alloc_zero(&s.a1, (long)n_nets * nb * h->ga1.block, h, (t + "a1").c_str()))) return rc;
        if ((rc = alloc_zero(&s.a2, (long)n_nets * nb * h->ga2.block, h, (t + "a2").c_str()))) return rc;
    }
    {
        // The training set's a3 (online nets first) sits directly behind the dL/dh area: for a batch of nb blocks dL/dh is
        // placed so that it ENDS where a3 begins, and [dL/dh | a3 of the K online nets] is one contiguous run -- the two
        // factors of the Dense_0 gradient a data-parallel rank sends (idqn_dense0_factors) without copying them anywhere.
        const long front = (&s == &h->train) ? (long)h->cfg.n_heads * nb * h->J * 32 : 0;
        const long n_a3 = (long)n_nets * nb * h->ga3.block;
        float* base = nullptr;
        if ((rc = alloc_zero(&base, front + n_a3, h, (t + "a3_block").c_str()))) return rc;
        s.a3 = base + front;
        h->dbg.push_back({t + "a3", {(void*)s.a3, n_a3 * 4}});
    }
    long slabs = (long)nb * s.NS;  // the training set picks its splits per call (fewer, longer ones for more blocks): room for the largest
    if (&s == &h->train)
        for (int b = 1; b <= nb; ++b) slabs = std::max(slabs, (long)b * d0_splits(h, n_nets, b));
    s.part_slabs = slabs;
    if ((rc = alloc_zero(&s.part, (long)n_nets * slabs * h->J * 32, h, (t + "part").c_str()))) return rc;
    return IDQN_OK;
}

int plan_iqn_bwd_order(idqn_handle_s* h, int nb, int forced_e);
int cnn_setup(idqn_handle_s* h) {
    const idqn_config_t& c = h->cfg;
    int ih = c.obs_h, iw = c.obs_w, ci = c.obs_c;
    int lo_h[3], hi_h[3], lo_w[3], hi_w[3];
    for (int i = 0; i < 3; ++i) {
        ConvL& l = h->conv[i];
        l.K = KS[i][0]; l.S = KS[i][1]; l.CI = ci; l.CO = c.features[i]; l.IH = ih; l.IW = iw;
        same_pad(ih, l.K, l.S, &l.OH, &lo_h[i], &hi_h[i]);
        same_pad(iw, l.K, l.S, &l.OW, &lo_w[i], &hi_w[i]);
        l.PLh = lo_h[i]; l.PLw = lo_w[i];
        l.w_off = h->L.leaves[2 * i].offset;
        l.b_off = h->L.leaves[2 * i + 1].offset;
        ih = l.OH; iw = l.OW; ci = l.CO;
    }
    h->off_w0 = h->L.leaves[6].offset; h->off_b0 = h->L.leaves[7].offset;
    h->off_w1 = h->L.leaves[8].offset; h->off_b1 = h->L.leaves[9].offset;
    const ConvL *c0 = &h->conv[0], *c1 = &h->conv[1], *c2 = &h->conv[2];
    h->gx = make_geom(c0->IH, c0->IW, c0->CI, lo_h[0], hi_h[0], lo_w[0], hi_w[0]);
    h->ga1 = make_geom(c1->IH, c1->IW, c1->CI, lo_h[1], hi_h[1], lo_w[1], hi_w[1]);
    h->ga2 = make_geom(c2->IH, c2->IW, c2->CI, lo_h[2], hi_h[2], lo_w[2], hi_w[2]);
    h->ga3 = make_geom(c2->OH, c2->OW, c2->CO, 0, 0, 0, 0);
    int l, hh, l2, h2;
    dgrad_pad(c2->IH, c2->OH, c2->K, c2->S, c2->PLh, &l, &hh);
    dgrad_pad(c2->IW, c2->OW, c2->K, c2->S, c2->PLw, &l2, &h2);
    h->gda3 = make_geom(c2->OH, c2->OW, c2->CO, l, hh, l2, h2);
    dgrad_pad(c1->IH, c1->OH, c1->K, c1->S, c1->PLh, &l, &hh);
    dgrad_pad(c1->IW, c1->OW, c1->K, c1->S, c1->PLw, &l2, &h2);
    h->gda2 = make_geom(c1->OH, c1->OW, c1->CO, l, hh, l2, h2);
    h->gda1 = make_geom(c0->OH, c0->OW, c0->CO, 0, 0, 0, 0);
    h->F = c2->OH * c2->OW * c2->CO;
    h->J = c.features[3];
    // split-K of the Dense_0 forward: a weight-streaming kernel is bound by ~10 B/clk per CU (MI355X_MICROARCH.md), so
    // what matters is that EVERY CU streams and that they all stream the same amount: as many 4-wave workgroups as CUs,
    // never more (a 257th would stream alone after the others), with balanced splits of the F / 32 row units
    {
        const int units = h->F / 32;
        int ns = 256 * 4 / std::max(1, 2 * c.n_heads * (c.features[3] / 128));
        h->NS = std::max(1, std::min(std::min(ns, 64), units));
    }
    const int K = c.n_heads, nb = h->nb_max;
    int rc;
    if (h->planes) {  // packed weights of one net: forward kernels of the three layers, then the data-gradient kernels
        long off = 0;
        for (int i = 0; i < 3; ++i) {
            h->wq_fwd[i] = off;
            off += (long)h->conv[i].K * h->conv[i].K * h->conv[i].CI * h->conv[i].CO * 6;  // 3 planes x 2 bytes
        }
        for (int i = 1; i < 3; ++i) {
            h->wq_dg[i] = off;
            off += (long)h->conv[i].K * h->conv[i].K * h->conv[i].CI * h->conv[i].CO * 6;
        }
        h->wq_stride = (off + 1023) / 1024 * 1024;
    }
    if ((rc = netset_alloc(h, h->train, 2 * K, nb, 2, ""))) return rc;
    // (i-IQN Q-values take up to max_batch states per call: the acting set holds that many sample blocks)
    if ((rc = netset_alloc(h, h->infer, 1, c.n_quantiles > 0 ? nb : 1, 1, "infer_", 4))) return rc;
    if (h->planes && debug_env("IDQN_CONV_PROF")) {
        h->cprof_role = atoi(debug_env("IDQN_CONV_PROF"));
        // role 10 = the chained forward launch: one [2][4096][8] block of stamps per layer
        if ((rc = alloc_zero(&h->cprof, (h->cprof_role == 10 ? 3 : 1) * 2L * 2 * 8 * 4096, h, "cprof"))) return rc;
    }
    if (h->planes) {
        if (nb > 1) {
            float* c = nullptr;
            if ((rc = alloc_zero(&h->td_bpart, (long)K * (h->J / 32) * nb * TD_BPART, h, "td_bpart"))) return rc;
            if ((rc = alloc_zero(&c, (long)K * (h->J / 32) + 16, h, "td_bctr"))) return rc;
            h->td_bctr = reinterpret_cast<unsigned*>(c);
        }
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->n_cus = cus;
        if ((rc = alloc_zero16(&h->da3p, (long)K * nb * h->gda3.block * 3, h, "da3p"))) return rc;
        if ((rc = alloc_zero16(&h->da2p, (long)K * nb * h->gda2.block * 3, h, "da2p"))) return rc;
        if ((rc = alloc_zero16(&h->da1p, (long)K * nb * h->gda1.block * 3, h, "da1p"))) return rc;
        for (int i = 0; i < 3; ++i) {
            char nm[8];
            snprintf(nm, sizeof nm, "pb%d", i);
            if ((rc = alloc_zero(&h->pbuf[i], (long)K * nb * h->conv[i].OH * h->conv[i].OW * h->conv[i].CO, h, nm))) return rc;
        }
    }
    std::vector<const float*> wb(2 * K);
    std::vector<int> is(2 * K);
    for (int k = 0; k < K; ++k) {
        wb[k] = h->online + (long)k * h->L.head_stride; is[k] = 0;
        wb[K + k] = h->target + (long)k * h->L.head_stride; is[K + k] = 1;
    }
    IDQN_HIP_CHECK(hipMemcpy(h->train.wbase, wb.data(), sizeof(float*) * 2 * K, hipMemcpyHostToDevice));
    IDQN_HIP_CHECK(hipMemcpy(h->train.in_set, is.data(), sizeof(int) * 2 * K, hipMemcpyHostToDevice));
    IDQN_HIP_CHECK(hipMemset(h->infer.in_set, 0, sizeof(int)));
    for (int i = 0; i < 3; ++i) {
        char nm[12];
        snprintf(nm, sizeof nm, "act_a%d", i + 1);
        if ((rc = alloc_zero(&h->act_a[i], (long)h->conv[i].OH * h->conv[i].OW * h->conv[i].CO, h, nm))) return rc;
    }
    if ((rc = alloc_zero(&h->act_part, 256L * h->J, h, "act_part"))) return rc;
    {
        float* p = nullptr;
        if ((rc = alloc_zero(&p, ((long)c.obs_h * c.obs_w * c.obs_c + 3) / 4 + 16, h, "act_state"))) return rc;
        h->act_state = (uint8_t*)p;
        if ((rc = alloc_zero(&p, 16, h, "act_action"))) return rc;
        h->act_action = (int32_t*)p;
    }
    if (h->J % 256 == 0 && (rc = alloc_zero(&h->dpart, (long)(h->J / 256) * K * nb * h->F * 32, h, "dpart"))) return rc;
    if (!h->planes) {
        if ((rc = alloc_zero(&h->da3, (long)K * nb * h->gda3.block, h, "da3"))) return rc;
        if ((rc = alloc_zero(&h->da2, (long)K * nb * h->gda2.block, h, "da2"))) return rc;
        if ((rc = alloc_zero(&h->da1, (long)K * nb * h->gda1.block, h, "da1"))) return rc;
    }
    if ((rc = alloc_zero(&h->qdbg, (long)2 * K * nb * 32 * 32, h, "q"))) return rc;
    if ((rc = alloc_zero(&h->hbuf, (long)2 * K * nb * h->J * 32, h, "h"))) return rc;
    if ((rc = alloc_zero(&h->qpart, (long)2 * K * nb * (h->J / 32) * 32 * 32, h, "qpart"))) return rc;
    if ((rc = alloc_zero(&h->infer_hbuf, (long)h->J * 32, h, "infer_h"))) return rc;
    if ((rc = alloc_zero(&h->infer_qpart, (long)(h->J / 32) * 32 * 32, h, "infer_qpart"))) return rc;
    for (int i = 1; i < 3; ++i) {
        const ConvL& cl = h->conv[i];
        IDQN_REQUIRE(cl.K % cl.S == 0, "conv %d: kernel %d not a multiple of stride %d", i, cl.K, cl.S);
        h->wt_stride[i] = ((long)cl.K * cl.K * cl.CI * cl.CO + 63) / 64 * 64;
        if (!h->planes && (rc = alloc_zero(&h->wt[i], (long)K * h->wt_stride[i], h, i == 1 ? "wt1" : "wt2"))) return rc;
    }
    // weight-gradient slabs: one per workgroup chunk of 16 output positions; one region per conv layer
    long slab_total = 0;
    for (int i = 0; i < 3; ++i) {
        const ConvL& cl = h->conv[i];
        int npos = cl.OH * cl.OW;
        // Chunk size = positions per workgroup.  The launch has K * taps * npc equal workgroups, all resident at once,
        // so its time is (workgroups on the busiest CU) x (positions per workgroup + a fixed cost of ~2 positions for
        // the prologue / slab epilogue); a lone workgroup on a CU has nobody to hide its latencies behind (x 1.1).
        // Measured on the Atari shapes (tools/gpu_ppc.sh): Conv_0 19 -> 38 positions 31.4 -> 28.5 us, Conv_1 16 -> 41
        // positions 30.3 -> 26.0 us, Conv_2 stays at 11 (21.4 us); fewer chunks also mean fewer slabs to sum.
        {
            const int taps = (i == 0) ? cl.K : cl.K * cl.K;
            double best = 1e30;
            for (int npc = 1; npc <= npos; ++npc) {
                const int ppc = (npos + npc - 1) / npc;  // balanced chunks
                if (ppc < 4 && npc > 1) break;
                const long wgs = (long)K * taps * ((npos + ppc - 1) / ppc);
                const double cost = (double)((wgs + 255) / 256) * (ppc + 2.0) * (wgs <= 256 ? 1.1 : 1.0);
                if (cost < best) { best = cost; h->pos_per_chunk[i] = ppc; }
            }
        }
        {
            char nm[16];
            snprintf(nm, sizeof nm, "IDQN_PPC%d", i);  // experiment knob: positions per weight-gradient chunk
            if (const char* e = debug_env(nm)) { const int v = atoi(e); if (v >= 1 && v <= npos) h->pos_per_chunk[i] = v; }
        }
        h->npc[i] = (npos + h->pos_per_chunk[i] - 1) / h->pos_per_chunk[i];
        if (h->planes) {  // plane path: (head, kernel row, chunk) workgroups, about one per CU (Conv_0: (head, chunk))
            const int per_chunk = K * (i == 0 ? 1 : cl.K);
            // never more workgroups than CUs (a 257th would run alone after the others), never more than 64 chunks: k_adam adds a leaf's
            // slabs one after the other (K = 1: 256 chunks of Conv_0 cost it 5 us more than they save the weight gradient)
            int nch = std::min(cu_budget() / per_chunk, 64);
            h->npc[i] = std::max(1, std::min(nch, npos));
        }
        h->slab_stride[i] = ((long)cl.K * cl.K * cl.CI * cl.CO + cl.CO + 63) / 64 * 64;
        h->slab_off[i] = slab_total;
        slab_total += (long)h->npc[i] * K * h->slab_stride[i];
    }
    if ((rc = alloc_zero(&h->slab, slab_total, h, "slab"))) return rc;
    IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_dense0_dgrad<4>, hipFuncAttributeMaxDynamicSharedMemorySize, h->J * 32 * 4));
    IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_dense0_dgrad<3>, hipFuncAttributeMaxDynamicSharedMemorySize, h->J * 32 * 4));
    if (c.n_quantiles > 0) {  // i-IQN heads: V = 3K virtual nets x N fractions x nb sample blocks (iqn_kernels.h)
        IDQN_REQUIRE(h->planes, "i-IQN heads run on the plane conv path (IDQN_CONV=bf16x3)");
        IDQN_REQUIRE(h->J % 256 == 0, "i-IQN heads: dense width %d must be a multiple of 256", h->J);
        IDQN_REQUIRE(nb <= 8, "i-IQN heads: max_batch %d above 256", c.max_batch);
        IqnWs& w = h->iqn;
        w.N = c.n_quantiles; w.V = 3 * K; w.nb_max = nb;
        w.off_we = h->L.leaves[10].offset; w.off_be = h->L.leaves[11].offset;
        const long VN = (long)w.V * w.N * nb, KN = (long)K * w.N * nb;
        IDQN_HIP_CHECK(hipMalloc((void**)&w.wbase_v, sizeof(float*) * w.V));
        h->owned.push_back((void*)w.wbase_v);
        std::vector<const float*> wv(w.V);
        for (int k = 0; k < K; ++k) {
            wv[k] = h->online + (long)k * h->L.head_stride;
            wv[K + k] = wv[2 * K + k] = h->target + (long)k * h->L.head_stride;
        }
        IDQN_HIP_CHECK(hipMemcpy(w.wbase_v, wv.data(), sizeof(float*) * w.V, hipMemcpyHostToDevice));
        {
            float* tmp = nullptr;  // (alloc_zero counts floats: 12 x 512 bf16 = 3072 floats per block)
            if ((rc = alloc_zero(&tmp, VN * 3072, h, "iqn_cosp"))) return rc;
            w.cosp = (unsigned short*)tmp;
            if ((rc = alloc_zero(&tmp, VN * 3072, h, "iqn_cosa"))) return rc;
            w.cosa = (unsigned short*)tmp;
            if ((rc = alloc_zero(&tmp, 2L * K * (h->F / 32) * 3072, h, "iqn_wep"))) return rc;
            w.wep = (unsigned short*)tmp;
        }
        if ((rc = alloc_zero(&w.xq, VN * h->F * 32, h, "iqn_x"))) return rc;
        if ((rc = alloc_zero(&w.part, VN * w.NS * h->J * 32, h, "iqn_part"))) return rc;
        if ((rc = alloc_zero(&w.hbuf, VN * h->J * 32, h, "iqn_h"))) return rc;
        if ((rc = alloc_zero(&w.qpart, VN * (h->J / 32) * 32 * 32, h, "iqn_qpart"))) return rc;
        if ((rc = alloc_zero(&w.z, VN * c.n_actions * 32, h, "iqn_z"))) return rc;
        if ((rc = alloc_zero(&w.dq, KN * c.n_actions * 32, h, "iqn_dq"))) return rc;
        if ((rc = alloc_zero(&w.dh, KN * h->J * 32, h, "iqn_dh"))) return rc;
        if ((rc = alloc_zero(&w.dx, KN * h->F * 32, h, "iqn_dx"))) return rc;
        // the embedding backward deals the fractions of a feature tile to QG workgroups (a divisor of N)
        w.QG = 4;
        while (w.QG > 1 && w.N % w.QG != 0) --w.QG;
        if ((rc = alloc_zero(&w.dpsi, (long)w.QG * K * nb * h->F * 32, h, "iqn_dpsi"))) return rc;
        if ((rc = alloc_zero(&w.gpart, (long)nb * w.QG * K * 65 * h->F, h, "iqn_gpart"))) return rc;
        w.HG = 8;
        while (w.HG > 1 && w.N % w.HG != 0) --w.HG;
        if ((rc = alloc_zero(&w.hpart, (long)nb * w.HG * K * ((long)h->J * c.n_actions + h->J + c.n_actions), h, "iqn_hpart"))) return rc;
        if ((rc = alloc_zero(&w.lpart, (long)K * nb, h, "iqn_lpart"))) return rc;
        if (debug_env("IDQN_IQN_CLOCK") && (rc = alloc_zero(&w.clk, (1024 + 256 * 8 * 2 + 512) * 2, h, "iqn_clk"))) return rc;
        bool any16 = false;  // some batch size gives a block count NB = N nb that is a multiple of 16 (the split GEMM paths)
        for (int b = 1; b <= nb; ++b) any16 = any16 || (w.N * b) % 16 == 0;
        if (any16 && (rc = alloc_zero(&w.g1, (long)K * h->F * h->J, h, "iqn_g1"))) return rc;
        {
            float* gw = nullptr;
            if ((rc = alloc_zero(&gw, 2L * K * cdiv(h->F, 256) + 64, h, "iqn_gate"))) return rc;
            w.gate = reinterpret_cast<unsigned*>(gw);
        }
        for (int b = 1; b <= nb; ++b)
            if ((w.N * b) % 16 == 0 && h->J % 256 == 0 && (rc = plan_iqn_bwd_order(h, b, debug_int("IDQN_IQN_BWD_EARLY", -1)))) return rc;
        if ((rc = alloc_zero(&w.dbg, (long)K * (2 * w.N + 33) * 32, h, "iqn_dbg"))) return rc;
    }
    h->dominant = "k_dense0_wgrad";
    return IDQN_OK;
}

// Dispatch order of k_iqn_d0_bwd_adam (iqn_gemm.h).  A group = (head, 256 rows of Dense_0/kernel) has nbg data-gradient items, which read
// those rows, and n_jh weight-gradient items, which overwrite them in their epilogue and are ~2 x as long (N = 32).  Rules: a group's
// items sit on ONE XCD (workgroup b runs on XCD b % 8; its slot there is b / 8) with the data-gradient items at EARLIER slots than
// the weight-gradient items -- they are dispatched first and wait for nothing, so the gate of the epilogue cannot block progress.
// Within that, the order decides the launch time: the last item of every valid order is a long one, and with each group's items
// back to back the long items start as late as 0.7 of the launch (513 us measured where 408 us of work per CU were queued:
// profiles/r6_iiqn_adam_fuse.txt).  Candidates `e`: the first e groups of the XCD back to back (their long items start in the
// first round), then every other data-gradient item, then the remaining long items together as the last round.  The candidate
// with the smallest list-scheduled makespan on the XCD's 32 CUs, averaged over +- 8 % of the long items' length, is taken.
// One plan per sample-block count nb (NB = N nb blocks per net: NB / 8 data-gradient items per group, weight-gradient items
// over 32 NB rows).  For nb > 1 the same model also decides between this launch and the two-split pair k_iqn_d0_bwd +
// k_iqn_d0_adam (half-length weight-gradient items without epilogue, list-scheduled on all CUs, plus the Adam pass as a stream
// of 32 bytes per Dense_0 element at 4 TB/s); nb = 1 keeps its rule (fused when the items exceed one round of the chip).
static double iqn_bwd_makespan(const std::vector<char>& seq, double dw, int ncu) {
    std::priority_queue<double, std::vector<double>, std::greater<double>> cus;
    for (int i = 0; i < ncu; ++i) cus.push(0.0);
    double end = 0;
    for (char it : seq) {
        const double e = cus.top() + (it ? dw : 1.0);
        cus.pop();
        cus.push(e);
        end = std::max(end, e);
    }
    return end;
}
static std::vector<char> iqn_bwd_seq(int n, int e, int nbg, int n_jh) {  // 0 = data-gradient item, 1 = weight-gradient item
    std::vector<char> s;
    for (int g = 0; g < e; ++g) { s.insert(s.end(), nbg, 0); s.insert(s.end(), n_jh, 1); }
    s.insert(s.end(), (size_t)nbg * (n - e), 0);
    s.insert(s.end(), (size_t)n_jh * (n - e), 1);
    return s;
}
int plan_iqn_bwd_order(idqn_handle_s* h, int nb, int forced_e) {
    IqnWs& w = h->iqn;
    const int NB = w.N * nb;
    const int K = h->cfg.n_heads, nbg = NB / 8, n_jh = h->J / 256, G = K * cdiv(h->F, 256), per = nbg + n_jh;
    // lengths in units of a data-gradient item: 8 blocks x 256 rows x J against 256 x 256 x (32 NB) products (measured 141 : 84 us at NB = 32, J = 512) + epilogue
    const double dw = 1.68 * (NB / 32.0) * (512.0 / h->J) + 0.33;
    const int S = cdiv(G, 8) * per;
    std::vector<int32_t> items((size_t)S * 8, -1);
    double fused = 0;  // the slowest XCD's makespan (units)
    for (int x = 0; x < 8; ++x) {
        const int n = (G - x + 7) / 8;  // groups x, x + 8, ...
        int best_e = n;
        double best = 0;
        for (int e = 0; e <= n; ++e) {
            const std::vector<char> seq = iqn_bwd_seq(n, e, nbg, n_jh);
            double sum = 0;
            for (double sc : {0.92, 0.96, 1.0, 1.04, 1.08}) sum += iqn_bwd_makespan(seq, dw * sc, std::max(1, h->n_cus / 8));
            if (e == 0 || sum < best) { best = sum; best_e = e; }
        }
        if (forced_e >= 0) best_e = std::min(forced_e, n);
        fused = std::max(fused, iqn_bwd_makespan(iqn_bwd_seq(n, best_e, nbg, n_jh), dw, std::max(1, h->n_cus / 8)));
        if (debug_on("IDQN_PLAN_PRINT") && x == 0) fprintf(stderr, "[plan] iqn dense0 gradients (nb %d): %d groups on XCD 0, %d of them back to back\n", nb, n, best_e);
        int s = 0;
        auto put = [&](int g, int within) { items[(size_t)(s++) * 8 + x] = ((x + 8 * g) << 8) | within; };
        for (int g = 0; g < best_e; ++g)
            for (int i = 0; i < per; ++i) put(g, i);
        for (int g = best_e; g < n; ++g)
            for (int i = 0; i < nbg; ++i) put(g, i);
        for (int g = best_e; g < n; ++g)
            for (int i = nbg; i < per; ++i) put(g, i);
    }
    int32_t*& dst = w.bwd_items[nb - 1];
    if (dst) (void)hipFree(dst);
    IDQN_HIP_CHECK(hipMalloc((void**)&dst, items.size() * 4));
    IDQN_HIP_CHECK(hipMemcpy(dst, items.data(), items.size() * 4, hipMemcpyHostToDevice));
    w.bwd_blocks[nb - 1] = (int)items.size();
    const int n_d = G * nbg, n_w1 = G * n_jh;
    if (nb == 1) {
        w.bwd_fuse[0] = n_d + n_w1 > cu_budget();
    } else {
        std::vector<char> seq((size_t)n_d, 0);
        seq.insert(seq.end(), (size_t)2 * n_w1, 1);
        const double unit_us = 84.0 * h->J / 512.0;
        const double adam = (double)K * h->F * h->J * 32.0 / 4.0e6 / unit_us;
        const double split = iqn_bwd_makespan(seq, (dw - 0.33) / 2, std::max(1, h->n_cus)) + adam;
        w.bwd_fuse[nb - 1] = fused < split;
        if (debug_on("IDQN_PLAN_PRINT"))
            fprintf(stderr, "[plan] iqn dense0 update (nb %d): fused %.2f vs two splits + adam %.2f units -> %s\n", nb, fused, split,
                    w.bwd_fuse[nb - 1] ? "fused" : "two splits");
    }
    // IDQN_IQN_ADAM_FUSE=0 (read here, once per plan: INTEGRATION.md): the two-split launch + Adam pass wherever the plan says fused
    // (tests/test_gpu_iqn_shapes.py holds that pair to the oracle at the shapes the planner would never give it)
    if (const char* e = getenv("IDQN_IQN_ADAM_FUSE"))
        if (atoi(e) == 0) w.bwd_fuse[nb - 1] = false;
    return IDQN_OK;
}

// ---- general-shape cnn path (gcnn_kernels.h) -------------------------------------------------------------------------
int gcnn_setup(idqn_handle_s* h) {
    const idqn_config_t& c = h->cfg;
    GcnnWs& g = h->gc;
    g.on = true;
    g.Bmax = c.max_batch;
    int ih = c.obs_h, iw = c.obs_w, ci = c.obs_c, lo, hi;
    for (int i = 0; i < 3; ++i) {
        ConvL& l = h->conv[i];
        l.K = KS[i][0]; l.S = KS[i][1]; l.CI = ci; l.CO = c.features[i]; l.IH = ih; l.IW = iw;
        same_pad(ih, l.K, l.S, &l.OH, &l.PLh, &hi);
        same_pad(iw, l.K, l.S, &l.OW, &l.PLw, &hi);
        (void)lo;
        l.w_off = h->L.leaves[2 * i].offset; l.b_off = h->L.leaves[2 * i + 1].offset;
        ih = l.OH; iw = l.OW; ci = l.CO;
    }
    const int K = c.n_heads;
    h->F = ih * iw * ci;
    FcNet& n = h->fc;  // the dense head over the flattened features
    n.L = c.n_features - 3 + 1;
    IDQN_REQUIRE(n.L <= FC_MAX_LAYERS, "cnn: too many dense layers (%d)", n.L);
    n.d[0] = h->F;
    n.dmax = n.d[0];
    for (int l = 0; l < n.L; ++l) {
        n.d[l + 1] = 3 + l < c.n_features ? c.features[3 + l] : c.n_actions;
        n.dmax = std::max(n.dmax, n.d[l + 1]);
        n.w_off[l] = h->L.leaves[6 + 2 * l].offset;
        n.b_off[l] = h->L.leaves[7 + 2 * l].offset;
    }
    int rc;
    const long B = g.Bmax;
    for (int i = 0; i < 3; ++i) {
        const ConvL& l = h->conv[i];
        const long per = (long)l.OH * l.OW * l.CO;
        char nm[16];
        snprintf(nm, sizeof nm, "g_act%d", i);
        if ((rc = alloc_zero(&g.act[i], 2L * K * B * per, h, nm))) return rc;
        snprintf(nm, sizeof nm, "g_dact%d", i);
        if ((rc = alloc_zero(&g.dact[i], (long)K * B * per, h, nm))) return rc;
        snprintf(nm, sizeof nm, "g_iact%d", i);
        if ((rc = alloc_zero(&g.inf_act[i], 32L * per, h, nm))) return rc;
    }
    if ((rc = alloc_zero(&h->fc_ws, K * ((long)(n.L + 3) * B * n.dmax + 2 * B), h, "fc_ws"))) return rc;
    if ((rc = alloc_zero(&g.inf_ws, 2L * 32 * n.dmax, h, "g_infws"))) return rc;
    if ((rc = alloc_zero(&h->qdbg, 2L * K * B * c.n_actions, h, "q"))) return rc;
    // parameter pointers of the 2K training nets (online first), as the conv kernels index them
    IDQN_HIP_CHECK(hipMalloc((void**)&h->train.wbase, sizeof(float*) * 2 * K));
    h->owned.push_back((void*)h->train.wbase);
    std::vector<const float*> wb(2 * K);
    for (int k = 0; k < K; ++k) {
        wb[k] = h->online + (long)k * h->L.head_stride;
        wb[K + k] = h->target + (long)k * h->L.head_stride;
    }
    IDQN_HIP_CHECK(hipMemcpy(h->train.wbase, wb.data(), sizeof(float*) * 2 * K, hipMemcpyHostToDevice));
    h->dominant = "k_fc_step";
    return IDQN_OK;
}

GConvArgs gconv_args(idqn_handle_s* h, int layer, const float* const* wbase, int n_nets, int n_split, int B, const uint8_t* s0,
                     const uint8_t* s1, const float* in, float* out) {
    const ConvL& l = h->conv[layer];
    GConvArgs a;
    a.in_u8[0] = s0; a.in_u8[1] = s1; a.in = in; a.out = out; a.wbase = wbase; a.w_off = l.w_off; a.b_off = l.b_off;
    a.n_nets = n_nets; a.n_split = n_split; a.B = B; a.IH = l.IH; a.IW = l.IW; a.CI = l.CI; a.OH = l.OH; a.OW = l.OW; a.CO = l.CO;
    a.KS = l.K; a.S = l.S; a.PLh = l.PLh; a.PLw = l.PLw;
    return a;
}

unsigned ggrid(long n) { return (unsigned)std::max(1L, std::min((n + 255) / 256, 65536L)); }

// conv trunk of `n_nets` nets (the first n_split read s0, the rest s1) into act[0..2]
int gcnn_trunk(idqn_handle_s* h, const float* const* wbase, int n_nets, int n_split, int B, const uint8_t* s0, const uint8_t* s1,
               float* const act[3], hipStream_t q) {
    for (int i = 0; i < 3; ++i) {
        const GConvArgs a = gconv_args(h, i, wbase, n_nets, n_split, B, s0, s1, i == 0 ? nullptr : act[i - 1], act[i]);
        hipLaunchKernelGGL(k_gconv_fwd, dim3(ggrid((long)n_nets * B * a.OH * a.OW * a.CO)), dim3(256), 0, q, a);
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// What every MLP-step launch of handle h is told: the arenas, the counters and outputs, the constants.  The batch pointers,
// s_stride / din and is_weight / td_abs stay NULL / 0 for the caller to set.
static FcArgs fc_args(idqn_handle_s* h, int batch, int mean_divisor, bool grads_only) {
    FcArgs a;
    memset(&a, 0, sizeof(a));
    a.net = h->fc; a.online = h->online; a.target = h->target; a.grad = h->grad; a.P = h->L.head_stride;
    a.gamma_n = h->gamma_n; a.B = batch; a.Bdiv = mean_divisor; a.K = h->cfg.n_heads;
    a.ws = h->fc_ws; a.losses = h->losses; a.q_dbg = h->qdbg;
    a.count = h->count; a.bcinv = h->bcinv; a.adam_b1 = h->ad.b1; a.adam_b2 = h->ad.b2;
    a.cum = h->cum; a.finish_step = grads_only ? 0 : 1;
    a.gm = GradMap{h->gP, h->g_w0_begin, h->g_w0_end, h->g_w0_base};
    return a;
}

// The replay frame ring as the one-launch step's minibatch source
template <class Slots>
static FcRingSrc<Slots> fc_ring_src(const void* ring, const int32_t* rows, long n_frames, long frame_bytes, int stack, const Slots& slots) {
    return FcRingSrc<Slots>{(const float*)ring, rows, n_frames, frame_bytes / 4, stack, slots};
}

// k_fc_step_par<PROF, Src>: the stamped instantiation (IDQN_FC_PROF) exists in the debug build only
template <class Src>
static hipError_t fc_step_par_set_lds(int bytes) {
#ifdef IDQN_DEBUG_KNOBS
    if (const hipError_t e = hipFuncSetAttribute((const void*)k_fc_step_par<true, Src>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) return e;
#endif
    return hipFuncSetAttribute((const void*)k_fc_step_par<false, Src>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}
template <class Src>
static void fc_step_par_launch(idqn_handle_s* h, hipStream_t q, const FcArgs& a, bool grads_only, const Src& src) {
    const dim3 grid(h->cfg.n_heads);
    const size_t lds = (size_t)h->fcp_plan_.floats * 4;
    const int adam = grads_only ? 0 : 1;
#ifdef IDQN_DEBUG_KNOBS
    if (debug_on("IDQN_FC_PROF")) {
        hipLaunchKernelGGL((k_fc_step_par<true, Src>), grid, dim3(FCM_T), lds, q, a, h->fcp_plan_, h->ad, h->online, h->mu, h->nu, adam, src);
        return;
    }
#endif
    hipLaunchKernelGGL((k_fc_step_par<false, Src>), grid, dim3(FCM_T), lds, q, a, h->fcp_plan_, h->ad, h->online, h->mu, h->nu, adam, src);
}

int gcnn_learn(idqn_handle_s* h, const StepIn& in, hipStream_t q) {
    GcnnWs& g = h->gc;
    const int K = h->cfg.n_heads, B = in.batch;
    const uint8_t *st = (const uint8_t*)in.state, *st2 = (const uint8_t*)in.next_state;
    const bool profile = in.profile();
    IDQN_REQUIRE(B <= g.Bmax, "batch %d exceeds the workspace (%d)", B, g.Bmax);
    int rc = gcnn_trunk(h, h->train.wbase, 2 * K, K, B, st, st2, g.act, q);
    if (rc) return rc;
    FcArgs a = fc_args(h, B, in.mean_divisor, in.grads_only());
    a.s = g.act[2]; a.s2 = g.act[2] + (long)K * B * h->F; a.s_stride = (long)B * h->F; a.din = g.dact[2];
    a.action = in.action; a.reward = in.reward; a.terminal = in.terminal;
    a.is_weight = in.is_weight; a.td_abs = in.td_abs;
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used], q));
    hipLaunchKernelGGL(k_fc_step, dim3(K), dim3(256), 0, q, a);
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) {
        IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used + 1], q));
        h->ev_used += 2;
    }
    // conv backward, top down: weight gradient of layer i from dact[i], then dact[i - 1] = (W^T dact[i]) * [act[i - 1] > 0]
    for (int i = 2; i >= 0; --i) {
        GConvBwdArgs b;
        b.f = gconv_args(h, i, h->train.wbase, K, K, B, st, st, i == 0 ? nullptr : g.act[i - 1], nullptr);
        b.dy = g.dact[i]; b.din = i > 0 ? g.dact[i - 1] : nullptr; b.grad = h->grad;
        b.gm = GradMap{h->gP, h->g_w0_begin, h->g_w0_end, h->g_w0_base};
        const long nw = (long)b.f.KS * b.f.KS * b.f.CI * b.f.CO + b.f.CO;
        hipLaunchKernelGGL(k_gconv_wgrad, dim3(ggrid(nw), K), dim3(256), 0, q, b);
        if (i > 0) hipLaunchKernelGGL(k_gconv_dgrad, dim3(ggrid((long)K * B * b.f.IH * b.f.IW * b.f.CI)), dim3(256), 0, q, b);
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ---- impala path (impala_kernels.h) ----------------------------------------------------------------------------------
int imp_wgrad_chunks(const ImpStackL& s, int conv, long B) {
    const int H = conv == 0 ? s.H : s.PH, W = conv == 0 ? s.W : s.PW;
    return (int)cdiv(B * cdiv(H, IMP_TH) * cdiv(W, IMP_TW), IMP_WG_TILES);
}

int imp_alloc_acts(idqn_handle_s* h, ImpActs& A, long n_img, const char* tag, bool named) {
    const ImpalaWs& w = h->imp;
    int rc;
    char nm[24];
    for (int s = 0; s < 3; ++s) {
        const ImpStackL& l = w.st[s];
        const long full = (long)l.H * l.W * l.CO, pooled = (long)l.PH * l.PW * l.CO;
        snprintf(nm, sizeof nm, "%s_c0_%d", tag, s);
        if ((rc = alloc_zero(&A.c0[s], n_img * full, h, nm))) return rc;
        for (int i = 0; i < 3; ++i) {
            // the names the tests read: imp_pool<s> = the pool's output, imp_stack<s> = the Stack's output
            if (named && i == 0) snprintf(nm, sizeof nm, "imp_pool%d", s);
            else if (named && i == 2) snprintf(nm, sizeof nm, "imp_stack%d", s);
            else snprintf(nm, sizeof nm, "%s_x%d_%d", tag, i, s);
            if ((rc = alloc_zero(&A.x[s][i], n_img * pooled, h, nm))) return rc;
        }
        for (int i = 0; i < 2; ++i) {
            snprintf(nm, sizeof nm, "%s_y%d_%d", tag, i, s);
            if ((rc = alloc_zero(&A.y[s][i], n_img * pooled, h, nm))) return rc;
        }
    }
    return IDQN_OK;
}

int impala_setup(idqn_handle_s* h) {
    const idqn_config_t& c = h->cfg;
    ImpalaWs& w = h->imp;
    w.on = true;
    w.Bmax = c.max_batch;
    const int K = c.n_heads;
    const long B = w.Bmax;
    int ih = c.obs_h, iw = c.obs_w, ci = c.obs_c, hi;
    long part_max = 0;
    for (int s = 0; s < 3; ++s) {
        ImpStackL& l = w.st[s];
        l.H = ih; l.W = iw; l.CI = ci; l.CO = c.features[s];
        same_pad(ih, 3, 2, &l.PH, &l.lo_h, &hi);
        same_pad(iw, 3, 2, &l.PW, &l.lo_w, &hi);
        for (int i = 0; i < 5; ++i) {
            l.w_off[i] = h->L.leaves[10 * s + 2 * i].offset;
            l.b_off[i] = h->L.leaves[10 * s + 2 * i + 1].offset;
            part_max = std::max(part_max, (long)imp_wgrad_chunks(l, i, B) * (9L * (i == 0 ? l.CI : l.CO) * l.CO + l.CO));
            if (w.wmx && !(s == 0 && i == 0) && imx_eligible(i == 0 ? l.CI : l.CO, l.CO)) {  // the larger of the two plans
                const imxw_plan_t p = imxw_plan((int)B, i == 0 ? l.H : l.PH, i == 0 ? l.W : l.PW, i == 0 ? l.CI : l.CO, l.CO);
                part_max = std::max(part_max, (long)p.n_chunks * p.part_len);
            }
        }
        ih = l.PH; iw = l.PW; ci = l.CO;
    }
    h->F = ih * iw * ci;
    FcNet& n = h->fc;  // the dense head over the flattened features
    n.L = c.n_features - 3 + 1;
    IDQN_REQUIRE(n.L <= FC_MAX_LAYERS, "impala: too many dense layers (%d)", n.L);
    n.d[0] = h->F;
    n.dmax = n.d[0];
    for (int l = 0; l < n.L; ++l) {
        n.d[l + 1] = 3 + l < c.n_features ? c.features[3 + l] : c.n_actions;
        n.dmax = std::max(n.dmax, n.d[l + 1]);
        n.w_off[l] = h->L.leaves[30 + 2 * l].offset;
        n.b_off[l] = h->L.leaves[31 + 2 * l].offset;
    }
    int rc;
    if ((rc = imp_alloc_acts(h, w.train, 2L * K * B, "imp", true))) return rc;
    if ((rc = imp_alloc_acts(h, w.infer, 32, "imp_i", false))) return rc;
    for (int s = 0; s < 3; ++s) {
        const ImpStackL& l = w.st[s];
        char nm[16];
        snprintf(nm, sizeof nm, "imp_d%d", s);
        if ((rc = alloc_zero(&w.d[s], (long)K * B * l.PH * l.PW * l.CO, h, nm))) return rc;
        snprintf(nm, sizeof nm, "imp_t%d", s);
        if ((rc = alloc_zero(&w.t[s], (long)K * B * l.PH * l.PW * l.CO, h, nm))) return rc;
        snprintf(nm, sizeof nm, "imp_dc0_%d", s);
        if ((rc = alloc_zero(&w.dc0[s], (long)K * B * l.H * l.W * l.CO, h, nm))) return rc;
    }
    if ((rc = alloc_zero(&w.wpart, (long)K * part_max, h, "imp_wpart"))) return rc;
    if ((rc = alloc_zero(&h->fc_ws, K * ((long)(n.L + 3) * B * n.dmax + 2 * B), h, "fc_ws"))) return rc;
    if ((rc = alloc_zero(&w.inf_ws, 2L * 32 * n.dmax, h, "imp_infws"))) return rc;
    w.d0_split = n.L >= 2;
    w.d0mx = w.d0mx && impd0x_applies(1, n.L);  // a head without a hidden layer has no such launch: the mode is a no-op
    if (w.d0_split) {
        FcNet& t = w.tail;
        t.L = n.L - 1;
        t.dmax = 0;
        for (int l = 0; l <= t.L; ++l) {
            t.d[l] = n.d[l + 1];
            t.dmax = std::max(t.dmax, t.d[l]);
        }
        for (int l = 0; l < t.L; ++l) {
            t.w_off[l] = n.w_off[l + 1];
            t.b_off[l] = n.b_off[l + 1];
        }
        if ((rc = alloc_zero(&w.hid, 2L * K * B * n.d[1], h, "imp_hid"))) return rc;
        if ((rc = alloc_zero(&w.dhid, (long)K * B * n.d[1], h, "imp_dhid"))) return rc;
        if ((rc = alloc_zero(&w.inf_hid, 32L * n.d[1], h, "imp_ihid"))) return rc;
    }
    if ((rc = alloc_zero(&h->qdbg, 2L * K * B * c.n_actions, h, "q"))) return rc;
    IDQN_HIP_CHECK(hipMalloc((void**)&h->train.wbase, sizeof(float*) * 2 * K));
    h->owned.push_back((void*)h->train.wbase);
    std::vector<const float*> wb(2 * K);
    for (int k = 0; k < K; ++k) {
        wb[k] = h->online + (long)k * h->L.head_stride;
        wb[K + k] = h->target + (long)k * h->L.head_stride;
    }
    IDQN_HIP_CHECK(hipMemcpy(h->train.wbase, wb.data(), sizeof(float*) * 2 * K, hipMemcpyHostToDevice));
    h->dominant = "k_fc_step";
    return IDQN_OK;
}

// one conv launch of Stack s: `conv` 0..4 forward, or its data gradient (dgrad: in = the output gradient)
enum ImpKind { IMP_FWD_U8, IMP_FWD_U8_PER_NET, IMP_FWD_PLAIN, IMP_FWD_INNER, IMP_FWD_RES, IMP_FWD_RES_RELU, IMP_DG_PLAIN, IMP_DG_MASK, IMP_DG_MASK_SKIP };
void imp_conv(idqn_handle_s* h, ImpKind kind, int s, int conv, const float* const* wbase, int n_nets, int n_split, int B,
              const uint8_t* s0, const uint8_t* s1, const float* in, float* out, const float* aux, const float* mask, hipStream_t q,
              const char* name) {
    const ImpStackL& l = h->imp.st[s];
    const bool dg = kind >= IMP_DG_PLAIN;
    ImpConvArgs a;
    a.in_u8[0] = s0; a.in_u8[1] = s1; a.in = in; a.out = out; a.aux = aux; a.mask = mask; a.wbase = wbase;
    a.w_off = l.w_off[conv]; a.b_off = l.b_off[conv]; a.n_nets = n_nets; a.n_split = n_split; a.B = B;
    a.H = conv == 0 ? l.H : l.PH; a.W = conv == 0 ? l.W : l.PW;
    const int leaf_ci = conv == 0 ? l.CI : l.CO;
    a.CI = dg ? l.CO : leaf_ci; a.CO = dg ? leaf_ci : l.CO;
    const dim3 blk(256);
    if (h->imp.mx && kind >= IMP_FWD_PLAIN && imx_eligible(leaf_ci, l.CO)) {  // the uint8 conv and every other layer: below
        const imx_plan_t p = imx_plan(a.H, a.W, a.CO, (long)n_nets * B);
        const dim3 mgrid(p.tiles, p.n_tiles, p.images);
        switch (kind) {
        case IMP_FWD_PLAIN: hipLaunchKernelGGL((k_imp_conv_mx<false, false, false, false, false>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<conv0>"; break;
        case IMP_FWD_INNER: hipLaunchKernelGGL((k_imp_conv_mx<true, true, false, false, false>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<inner>"; break;
        case IMP_FWD_RES: hipLaunchKernelGGL((k_imp_conv_mx<false, false, true, false, false>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<res>"; break;
        case IMP_FWD_RES_RELU: hipLaunchKernelGGL((k_imp_conv_mx<false, true, true, false, false>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<res>"; break;
        case IMP_DG_PLAIN: hipLaunchKernelGGL((k_imp_conv_mx<false, false, false, true, false>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<dgrad>"; break;
        case IMP_DG_MASK: hipLaunchKernelGGL((k_imp_conv_mx<false, false, false, true, true>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<dgrad mask>"; break;
        case IMP_DG_MASK_SKIP: hipLaunchKernelGGL((k_imp_conv_mx<false, false, true, true, true>), mgrid, blk, 0, q, a); name = "k_imp_conv_mx<dgrad mask skip>"; break;
        default: break;
        }
        tl_mark(h, q, name);
        return;
    }
    const dim3 grid((unsigned)(cdiv(a.H, IMP_TH) * cdiv(a.W, IMP_TW)), (unsigned)cdiv(a.CO, IMP_COB), (unsigned)(n_nets * B));
    switch (kind) {
    case IMP_FWD_U8: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_U8, false, false, false, false, false, 4>), grid, blk, 0, q, a); break;
    case IMP_FWD_U8_PER_NET: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_U8, false, false, false, false, false, 4, true>), grid, blk, 0, q, a); break;
    case IMP_FWD_PLAIN: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, false, false, false, false, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_FWD_INNER: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, true, true, false, false, false, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_FWD_RES: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, false, true, false, false, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_FWD_RES_RELU: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, true, true, false, false, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_DG_PLAIN: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, false, false, true, false, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_DG_MASK: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, false, false, true, true, IMP_CIC>), grid, blk, 0, q, a); break;
    case IMP_DG_MASK_SKIP: hipLaunchKernelGGL((k_imp_conv<IMP_SRC_F32, false, false, true, true, true, IMP_CIC>), grid, blk, 0, q, a); break;
    }
    tl_mark(h, q, name);
}

ImpPoolArgs imp_pool_args(const ImpStackL& l, long n_img) {
    ImpPoolArgs p;
    p.c0 = nullptr; p.out = nullptr; p.dy = nullptr; p.dx = nullptr; p.N = n_img;
    p.H = l.H; p.W = l.W; p.C = l.CO; p.PH = l.PH; p.PW = l.PW; p.lo_h = l.lo_h; p.lo_w = l.lo_w;
    return p;
}

// the three Stacks of `n_nets` nets (the first n_split read s0, the rest s1) on B samples each, into A
// per_net_u8 (B = 1, idqn_act_host_many_impala): net e reads state e of s0
int impala_trunk(idqn_handle_s* h, const float* const* wbase, int n_nets, int n_split, int B, const uint8_t* s0, const uint8_t* s1,
                 const ImpActs& A, hipStream_t q, bool per_net_u8 = false) {
    for (int s = 0; s < 3; ++s) {
        const ImpStackL& l = h->imp.st[s];
        if (s == 0) imp_conv(h, per_net_u8 ? IMP_FWD_U8_PER_NET : IMP_FWD_U8, s, 0, wbase, n_nets, n_split, B, s0, s1, nullptr, A.c0[s], nullptr, nullptr, q, "k_imp_conv<u8>");
        else imp_conv(h, IMP_FWD_PLAIN, s, 0, wbase, n_nets, n_split, B, nullptr, nullptr, A.x[s - 1][2], A.c0[s], nullptr, nullptr, q, "k_imp_conv<conv0>");
        ImpPoolArgs p = imp_pool_args(l, (long)n_nets * B);
        p.c0 = A.c0[s]; p.out = A.x[s][0];
        hipLaunchKernelGGL(k_imp_pool_fwd, dim3(ggrid(p.N * l.PH * l.PW * l.CO)), dim3(256), 0, q, p);
        tl_mark(h, q, "k_imp_pool_fwd");
        for (int blk = 0; blk < 2; ++blk) {
            imp_conv(h, IMP_FWD_INNER, s, 1 + 2 * blk, wbase, n_nets, n_split, B, nullptr, nullptr, A.x[s][blk], A.y[s][blk], nullptr, nullptr, q,
                     "k_imp_conv<inner>");
            imp_conv(h, s == 2 && blk == 1 ? IMP_FWD_RES_RELU : IMP_FWD_RES, s, 2 + 2 * blk, wbase, n_nets, n_split, B, nullptr, nullptr,
                     A.y[s][blk], A.x[s][blk + 1], A.x[s][blk], nullptr, q, "k_imp_conv<res>");
        }
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// weight + bias gradient of conv `conv` of Stack s for the K online nets: per-chunk partials, then their ordered sum
void imp_wgrad(idqn_handle_s* h, int s, int conv, int B, const uint8_t* st, const float* in, bool relu_in, const float* dy, hipStream_t q) {
    const ImpStackL& l = h->imp.st[s];
    const int K = h->cfg.n_heads;
    ImpWgradArgs a;
    a.in_u8 = st; a.in = in; a.dy = dy; a.part = h->imp.wpart; a.B = B;
    a.H = conv == 0 ? l.H : l.PH; a.W = conv == 0 ? l.W : l.PW; a.CI = conv == 0 ? l.CI : l.CO; a.CO = l.CO;
    if (h->imp.wmx && !st && imx_eligible(a.CI, a.CO)) {  // the uint8 conv and every other layer: below
        const imxw_plan_t p = imxw_plan(B, a.H, a.W, a.CI, a.CO);
        a.n_tiles = (int)p.n_tiles;
        a.n_chunks = (int)p.n_chunks;
        const dim3 mgrid(p.n_chunks, p.m_blocks * p.n_blocks, (unsigned)K);
        if (relu_in) hipLaunchKernelGGL((k_imp_wgrad_mx<true>), mgrid, dim3(256), 0, q, a);
        else hipLaunchKernelGGL((k_imp_wgrad_mx<false>), mgrid, dim3(256), 0, q, a);
        tl_mark(h, q, "k_imp_wgrad_mx");
    } else {
        a.n_tiles = B * cdiv(a.H, IMP_TH) * cdiv(a.W, IMP_TW);
        a.n_chunks = cdiv(a.n_tiles, IMP_WG_TILES);
        const dim3 grid((unsigned)a.n_chunks, (unsigned)(cdiv(a.CI, IMP_CIC) * cdiv(a.CO, IMP_COB)), (unsigned)K);
        if (st) hipLaunchKernelGGL((k_imp_wgrad<IMP_SRC_U8, false>), grid, dim3(256), 0, q, a);
        else if (relu_in) hipLaunchKernelGGL((k_imp_wgrad<IMP_SRC_F32, true>), grid, dim3(256), 0, q, a);
        else hipLaunchKernelGGL((k_imp_wgrad<IMP_SRC_F32, false>), grid, dim3(256), 0, q, a);
        tl_mark(h, q, "k_imp_wgrad");
    }
    ImpWreduceArgs r;
    r.part = h->imp.wpart; r.grad = h->grad; r.gm = GradMap{h->gP, h->g_w0_begin, h->g_w0_end, h->g_w0_base};
    r.w_off = l.w_off[conv]; r.b_off = l.b_off[conv]; r.nw = 9L * a.CI * a.CO; r.CO = a.CO; r.n_chunks = a.n_chunks;
    hipLaunchKernelGGL(k_imp_wreduce, dim3(ggrid(r.nw + r.CO), K), dim3(256), 0, q, r);
    tl_mark(h, q, "k_imp_wreduce");
}

// Dense_0 forward of `nets` nets on d0.B samples each, hid = relu(x W + b): the ONE statement of that launch, for the learner
// step's 2K nets and for the one net of idqn_q_values / idqn_act_host.  Both kernels give the same bytes.
int imp_d0_forward(idqn_handle_s* h, const ImpD0Args& d0, int nets, hipStream_t q) {
    if (h->imp.d0mx) {
        IDQN_REQUIRE(impd0x_shape_ok(d0.B, d0.F, d0.D, nets), "Dense_0 forward: B = %d, F = %d, D = %d, %d nets", d0.B, d0.F, d0.D, nets);
        const impd0x_plan_t p = impd0x_plan(d0.B, d0.F, d0.D, nets);
        hipLaunchKernelGGL(k_imp_d0_fwd_mx, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(256), 0, q, d0);
        tl_mark(h, q, "k_imp_d0_fwd_mx");
    } else {
        hipLaunchKernelGGL(k_imp_d0_fwd, dim3((unsigned)cdiv(d0.D, IMP_D0_OC), (unsigned)cdiv(d0.B, IMP_D0_SB), (unsigned)nets), dim3(256), 0, q, d0);
        tl_mark(h, q, "k_imp_d0_fwd");
    }
    return IDQN_OK;
}

int impala_learn(idqn_handle_s* h, const StepIn& in, hipStream_t q) {
    ImpalaWs& w = h->imp;
    const ImpActs& A = w.train;
    const int K = h->cfg.n_heads, B = in.batch;
    const uint8_t *st = (const uint8_t*)in.state, *st2 = (const uint8_t*)in.next_state;
    const bool profile = in.profile();
    IDQN_REQUIRE(B <= w.Bmax, "batch %d exceeds the workspace (%d)", B, w.Bmax);
    int rc = impala_trunk(h, h->train.wbase, 2 * K, K, B, st, st2, A, q);
    if (rc) return rc;
    FcArgs a = fc_args(h, B, in.mean_divisor, in.grads_only());
    a.s = A.x[2][2]; a.s2 = A.x[2][2] + (long)K * B * h->F; a.s_stride = (long)B * h->F; a.din = w.d[2];
    ImpD0Args d0;
    const int D = h->fc.d[1], sblocks = cdiv(B, IMP_D0_SB);
    if (w.d0_split) {
        d0.x = A.x[2][2]; d0.hid = w.hid; d0.dh = w.dhid; d0.din = w.d[2]; d0.wbase = h->train.wbase; d0.grad = h->grad;
        d0.gm = GradMap{h->gP, h->g_w0_begin, h->g_w0_end, h->g_w0_base};
        d0.w_off = h->fc.w_off[0]; d0.b_off = h->fc.b_off[0]; d0.B = B; d0.F = h->F; d0.D = D;
        if ((rc = imp_d0_forward(h, d0, 2 * K, q))) return rc;
        a.net = w.tail; a.s = w.hid; a.s2 = w.hid + (long)K * B * D; a.s_stride = (long)B * D; a.din = w.dhid;
    }
    a.action = in.action; a.reward = in.reward; a.terminal = in.terminal;
    a.is_weight = in.is_weight; a.td_abs = in.td_abs;
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used], q));
    hipLaunchKernelGGL(k_fc_step, dim3(K), dim3(256), 0, q, a);
    tl_mark(h, q, "k_fc_step");
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) {
        IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used + 1], q));
        h->ev_used += 2;
    }
    if (w.d0_split) {
        hipLaunchKernelGGL(k_imp_d0_wgrad, dim3((unsigned)cdiv(h->F, IMP_D0_R), (unsigned)cdiv(D, IMP_D0_OC), (unsigned)K), dim3(256), 0, q, d0);
        tl_mark(h, q, "k_imp_d0_wgrad");
        hipLaunchKernelGGL(k_imp_d0_dgrad, dim3((unsigned)cdiv(h->F, IMP_D0_R), (unsigned)sblocks, (unsigned)K), dim3(256), 0, q, d0);
        tl_mark(h, q, "k_imp_d0_dgrad");
    }
    // Stacks top down.  w.d[s] holds dL/dx of the Stack's running x (entering Stack 2: the head's input gradient, already
    // masked by the final ReLU); each block adds its branch to it in place.
    const float* const* wb = h->train.wbase;
    for (int s = 2; s >= 0; --s) {
        const ImpStackL& l = w.st[s];
        for (int blk = 1; blk >= 0; --blk) {
            imp_wgrad(h, s, 2 + 2 * blk, B, nullptr, A.y[s][blk], false, w.d[s], q);
            imp_conv(h, IMP_DG_MASK, s, 2 + 2 * blk, wb, K, K, B, nullptr, nullptr, w.d[s], w.t[s], nullptr, A.y[s][blk], q, "k_imp_conv<dgrad mask>");
            imp_wgrad(h, s, 1 + 2 * blk, B, nullptr, A.x[s][blk], true, w.t[s], q);
            imp_conv(h, IMP_DG_MASK_SKIP, s, 1 + 2 * blk, wb, K, K, B, nullptr, nullptr, w.t[s], w.d[s], w.d[s], A.x[s][blk], q,
                     "k_imp_conv<dgrad mask skip>");
        }
        ImpPoolArgs p = imp_pool_args(l, (long)K * B);
        p.c0 = A.c0[s]; p.dy = w.d[s]; p.dx = w.dc0[s];
        hipLaunchKernelGGL(k_imp_pool_bwd, dim3(ggrid(p.N * l.H * l.W * l.CO)), dim3(256), 0, q, p);
        tl_mark(h, q, "k_imp_pool_bwd");
        imp_wgrad(h, s, 0, B, s == 0 ? st : nullptr, s == 0 ? nullptr : A.x[s - 1][2], false, w.dc0[s], q);
        if (s > 0) imp_conv(h, IMP_DG_PLAIN, s, 0, wb, K, K, B, nullptr, nullptr, w.dc0[s], w.d[s - 1], nullptr, nullptr, q, "k_imp_conv<dgrad>");
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

int fc_setup(idqn_handle_s* h) {
    const idqn_config_t& c = h->cfg;
    FcNet& n = h->fc;
    n.L = c.n_features + 1;
    n.d[0] = c.obs_h * c.obs_w * c.obs_c;
    n.dmax = n.d[0];
    for (int l = 0; l < n.L; ++l) {
        n.d[l + 1] = l < c.n_features ? c.features[l] : c.n_actions;
        if (n.d[l + 1] > n.dmax) n.dmax = n.d[l + 1];
        n.w_off[l] = h->L.leaves[2 * l].offset;
        n.b_off[l] = h->L.leaves[2 * l + 1].offset;
    }
    const long B = c.max_batch, K = c.n_heads;
    int rc;
    if ((rc = alloc_zero(&h->fc_ws, K * ((long)(n.L + 3) * B * n.dmax + 2 * B) + 2 * 32 * n.dmax, h, "fc_ws"))) return rc;
    if ((rc = alloc_zero(&h->qdbg, 2 * K * B * c.n_actions, h, "q"))) return rc;
    h->fc_plan_ = fc_plan(n);
    if (n.dmax > FC_MAX_WIDTH) h->fc_plan_.BS = 0;  // wider layers: the generic kernel (any width)
    if (h->fc_plan_.BS) {
        const int bytes = (int)(h->fc_plan_.floats * 4);
        IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_step_lds<32>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_step_lds<16>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_step_lds<8>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    }
    h->fcp_plan_ = fc_par_plan(n, h->L.head_stride);
    // IDQN_FC_PAR=0: the two-launch path (k_fc_step_mfma / k_fc_step_lds + k_adam) for every batch size
    if ((getenv("IDQN_FC_PAR") && atoi(getenv("IDQN_FC_PAR")) == 0) || n.dmax > FC_MAX_WIDTH) h->fcp_plan_.floats = 0;
    if (h->fcp_plan_.floats) {
        const int bytes = (int)(h->fcp_plan_.floats * 4);
        IDQN_HIP_CHECK(fc_step_par_set_lds<FcBatchSrc>(bytes));
        IDQN_HIP_CHECK(fc_step_par_set_lds<FcRingSrc<RpsSlotsPar>>(bytes));
        IDQN_HIP_CHECK(fc_step_par_set_lds<FcRingSrc<RpsSlotsDev>>(bytes));
        h->fcs_plan_ = fc_steps_plan(n, h->L.head_stride);
        if (h->fcs_plan_.floats)
            IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_steps_par<FcRingSrc<RpsSlotsDev>>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(h->fcs_plan_.floats * 4)));
    }
    h->fcm_plan_ = fc_mfma_plan(n);
    if (n.dmax > FC_MAX_WIDTH) h->fcm_plan_.floats = 0;
    h->fcm_global_ = false;
    if (!h->fcm_plan_.floats && n.dmax <= FC_MAX_WIDTH) {
        // the matrix does not fit LDS beside the activations: the same kernel with the weight operand read from global memory
        h->fcm_plan_ = fc_mfma_plan_g(n);
        h->fcm_global_ = h->fcm_plan_.floats != 0;
    }
    if (h->fcm_plan_.floats) {
        if (h->fcm_global_)
            IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_step_mfma<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(h->fcm_plan_.floats * 4)));
        else
            IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_step_mfma<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(h->fcm_plan_.floats * 4)));
    }
    h->dominant = "k_fc_step";
    return IDQN_OK;
}

// Conv_1 / Conv_2 kernels re-indexed for the data gradient-as-convolution (k_wt_build), f32
int wt_build_args(idqn_handle_s* h, WtBuildArgs& wb) {  // returns the x extent of the launch
    wb.wbase = h->train.wbase; wb.K = h->cfg.n_heads;
    long maxe = 0;
    for (int i = 1; i <= 2; ++i) {
        const ConvL& l = h->conv[i];
        WtLayer& w = wb.layer[i - 1];
        w.wt = h->wt[i]; w.w_off = l.w_off; w.wt_stride = h->wt_stride[i];
        w.KH = l.K; w.KW = l.K; w.CI = l.CI; w.CO = l.CO; w.S = l.S; w.PLh = l.PLh; w.PLw = l.PLw;
        w.n_var = l.S * l.S; w.KHs = l.K / l.S; w.KWs = l.K / l.S;
        maxe = std::max(maxe, (long)l.K * l.K * l.CI * l.CO);
    }
    return cdiv(maxe, 256);
}

int build_dgrad_weights(idqn_handle_s* h, hipStream_t q) {
    if (h->wt_ready) return IDQN_OK;  // already built this step, inside the TD / loss launch
    WtBuildArgs wb;
    const int nx = wt_build_args(h, wb);
    hipLaunchKernelGGL(k_wt_build, dim3(nx, wb.K, 2), dim3(256), 0, q, wb);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// ---- plane conv path: launch plans -----------------------------------------------------------------------------
// role 0..2: forward of Conv_0..2; 3: data gradient of Conv_2; 4: data gradient of Conv_1
struct RoleGeom {
    int NPA, CT, NQ, NCC, S, SX, KH, n_var;
    CVar var[4];
};

int role_geom(idqn_handle_s* h, int role, RoleGeom& g) {
    memset(&g, 0, sizeof(g));
    if (role <= 2) {
        const ConvL& l = h->conv[role];
        g.NPA = role == 0 ? 1 : 3; g.CT = l.CO / 32; g.S = l.S; g.KH = l.K; g.n_var = 1;
        if (role == 0) {  // (kw, c) rows of a kernel row in 16-row chunks of 4 pixels x 4 channels
            IDQN_REQUIRE(l.CI == 4 && l.K == 8 && l.S == 4, "plane conv: Conv_0 is built for 8x8 stride 4 over 4 channels");
            g.NQ = l.K * l.CI / 16; g.NCC = 1; g.SX = 1;
        } else {
            g.NQ = l.K; g.NCC = l.CI / 16; g.SX = l.S;
        }
        CVar& v = g.var[0];
        v.w_off = h->wq_fwd[role]; v.in_off_h = 0; v.in_off_w = 0; v.OH = l.OH; v.OW = l.OW;
        v.out_mul = 1; v.out_add_h = 0; v.out_add_w = 0;
    } else {
        const int i = role == 3 ? 2 : 1;
        const ConvL& l = h->conv[i];
        const ActGeom& gd = i == 2 ? h->gda3 : h->gda2;
        const int KHs = l.K / l.S;
        g.NPA = 3; g.CT = l.CI / 32; g.NQ = KHs; g.NCC = l.CO / 16; g.S = 1; g.SX = 1; g.KH = KHs; g.n_var = l.S * l.S;
        IDQN_REQUIRE(g.n_var <= 4, "plane conv: stride %d data gradient has more than 4 parities", l.S);
        for (int vi = 0; vi < g.n_var; ++vi) {
            const int rh = vi / l.S, rw = vi % l.S;
            const int ph = (rh + l.PLh) % l.S, pw = (rw + l.PLw) % l.S;
            CVar& v = g.var[vi];
            v.w_off = h->wq_dg[i] + (long)vi * KHs * KHs * l.CO * l.CI * 6;
            v.in_off_h = (rh + l.PLh - ph) / l.S + gd.lo_h - KHs + 1;
            v.in_off_w = (rw + l.PLw - pw) / l.S + gd.lo_w - KHs + 1;
            v.OH = (l.IH - rh + l.S - 1) / l.S; v.OW = (l.IW - rw + l.S - 1) / l.S;
            v.out_mul = l.S; v.out_add_h = rh; v.out_add_w = rw;
            IDQN_REQUIRE(v.in_off_h >= 0 && v.in_off_w >= 0 && v.OH > 0 && v.OW > 0, "conv %d dgrad: bad variant geometry", i);
        }
    }
    return IDQN_OK;
}

// LDS bytes of one stage for positions [p0, p0 + np) of a variant with OW columns
long fwd_stage_bytes(const RoleGeom& g, int OW, int p0, int np, int* n_rows) {
    long bytes = (long)g.NQ * g.CT * 3 * 1024;
    const int oh0 = p0 / OW, oh1 = (p0 + np - 1) / OW;
    for (int row = oh0; row <= oh1; ++row) {
        const int lo = std::max(p0, row * OW), hi = std::min(p0 + np, (row + 1) * OW);
        bytes += (long)((hi - lo - 1) * g.SX + g.NQ) * g.NPA * 1024;
    }
    *n_rows = oh1 - oh0 + 1;
    return bytes;
}

// one candidate plan: about `target` workgroups per launch, `budget` bytes of LDS each (160 KB: one per CU, 80 KB: two)
int plan_fwd_target(int role, int n_nets, int nb, const RoleGeom& g, int target, size_t budget, FwdPlan& pl) {
    const int nt_max = convp_fwd_max_nt(g.CT);
    long npos_total = 0;
    for (int v = 0; v < g.n_var; ++v) npos_total += (long)g.var[v].OH * g.var[v].OW;
    const int per_slot = std::max(1, target / (n_nets * nb));
    int n_items = 0, np_all = 0;
    long stage_max = 0;
    // ranges per variant: proportional to its positions, rounded DOWN (one workgroup more than CUs would run alone after
    // all the others), leftovers to the variants with the most positions per range
    int Rv[4] = {1, 1, 1, 1}, used = 0;
    for (int v = 0; v < g.n_var; ++v) {
        const long npos = (long)g.var[v].OH * g.var[v].OW;
        Rv[v] = (int)std::max(1L, std::min(npos, per_slot * npos / npos_total));
        used += Rv[v];
    }
    for (; used < per_slot; ++used) {
        int best = -1;
        double worst = 0;
        for (int v = 0; v < g.n_var; ++v) {
            const double load = (double)g.var[v].OH * g.var[v].OW / Rv[v];
            if (Rv[v] < g.var[v].OH * g.var[v].OW && load > worst) { worst = load; best = v; }
        }
        if (best < 0) break;
        ++Rv[best];
    }
    for (int v = 0; v < g.n_var; ++v) {
        const int OW = g.var[v].OW, npos = g.var[v].OH * OW;
        int R = Rv[v];
        // limits: tiles per wave, rows spanned, LDS (two stages in 160 KB)
        for (;; ++R) {
            const int np = (npos + R - 1) / R;
            bool ok = (np * g.CT + 3) / 4 <= nt_max;
            const long masks = role >= 3 ? 4L * ((np * g.CT + 3) / 4) * CF_MASK_TILE_BYTES : 0;  // the data gradient's mask tiles
            for (int r = 0, p0 = 0; ok && r < R; ++r) {
                const int n = npos / R + (r < npos % R ? 1 : 0);
                int rows;
                if (n > 0 && (2 * fwd_stage_bytes(g, OW, p0, n, &rows) + masks > (long)budget - 8 * 1024 || rows > CP_MAX_STRIPS)) ok = false;
                p0 += n;
            }
            if (ok || R >= npos) break;
        }
        Rv[v] = R;
        for (int n = 0; n < n_nets; ++n)
            for (int bb = 0; bb < nb; ++bb)
                for (int r = 0, p0 = 0; r < R; ++r) {
                    const int cnt = npos / R + (r < npos % R ? 1 : 0);
                    if (cnt == 0) continue;
                    ++n_items;
                    int rows;
                    stage_max = std::max(stage_max, fwd_stage_bytes(g, OW, p0, cnt, &rows));
                    IDQN_REQUIRE(rows <= CP_MAX_STRIPS, "plane conv: %d positions span %d rows", cnt, rows);
                    np_all = std::max(np_all, cnt);
                    p0 += cnt;
                }
    }
    // The kernel derives item b arithmetically: slot = b / items_per_slot (net-major: consecutive workgroups, which the
    // XCD-contiguous remap keeps on one XCD, share a net's weights), then variant and balanced range inside the slot.
    pl = FwdPlan();
    pl.n_items = n_items;
    for (int v = 0; v < g.n_var; ++v) {
        pl.r_begin[v] = pl.items_per_slot;
        pl.r_cnt[v] = Rv[v];
        pl.items_per_slot += Rv[v];
    }
    IDQN_REQUIRE(pl.n_items == pl.items_per_slot * n_nets * nb, "plane conv: role %d item count %d does not match its ranges", role, pl.n_items);
    pl.NT = (np_all * g.CT + 3) / 4;
    IDQN_REQUIRE(pl.NT >= 1 && pl.NT <= nt_max, "plane conv: role %d needs %d tiles per wave", role, pl.NT);
    pl.stage = (size_t)stage_max;
    pl.ring = convp_fwd_ring(pl.stage, pl.NT, role <= 2 ? 0 : 1, budget);
    pl.lds = convp_fwd_lds(pl.stage, pl.NT, role <= 2 ? 0 : 1, pl.ring, role != 2, role == 2);
    IDQN_REQUIRE(pl.lds <= budget, "plane conv: role %d needs %zu bytes of LDS", role, pl.lds);
    return IDQN_OK;
}

// The launch plan of a role: one workgroup per CU, all co-resident, equal work.  IDQN_CONV_WGS=512 plans two smaller
// workgroups per CU instead (80 KB of LDS each), so that one's prologue / first fill / epilogue overlaps the other's main
// loop -- measured: Conv_0 forward 18.8 -> 18.5 us, Conv_1 data gradient 16.9 -> 21.7 us (more weight re-staging per
// MFMA, a two-deep ring); not the default.
int plan_fwd(idqn_handle_s* h, int role, int n_nets, int nb, const RoleGeom& g, FwdPlan** out, int target) {
    auto key = std::make_tuple(role, n_nets, nb, target);
    auto itp = h->fwd_plans.find(key);
    if (itp != h->fwd_plans.end()) { *out = &itp->second; return IDQN_OK; }
    FwdPlan pl;
    int rc = plan_fwd_target(role & 7, n_nets, nb, g, target, 160 * 1024, pl);
    if (rc) return rc;
    // A whole-chip forward launch whose workgroups would carry the same number of tiles per wave with ~18 % fewer of them
    // takes the smaller grid: the matrix loop is as long, the staging traffic and the fill burst are smaller (Conv_1 / Conv_2
    // forward at K = 5: 250 -> 210 workgroups, 24.5 -> 23.7 and 24.1 -> 23.2 us, profiles/r3_conv_cu_budget_sweep.txt;
    // Conv_0 would need 6 tiles instead of 5 and keeps 250).
    if (target == cu_budget() && (role & 7) <= 2) {
        FwdPlan p2;
        if (plan_fwd_target(role & 7, n_nets, nb, g, target * 13 / 16, 160 * 1024, p2) == IDQN_OK && p2.NT == pl.NT && p2.n_items < pl.n_items)
            pl = p2;
    }
    if (plan_print())
        fprintf(stderr, "[plan] fwd role %d nets %d nb %d target %d: %d workgroups, NT %d, ring %d, stage %zu B, lds %zu B, supersteps %d, "
                "ranges/slot %d (NPA %d CT %d NQ %d)\n", role, n_nets, nb, target, pl.n_items, pl.NT, pl.ring, pl.stage, pl.lds,
                g.KH * g.NCC, pl.items_per_slot, g.NPA, g.CT, g.NQ);
    *out = &(h->fwd_plans[key] = pl);
    return IDQN_OK;
}


// The persistent form of a forward / data-gradient role (convp_pp.hip) for launches with several items per CU: every
// output row of every variant is cut into `parts` column ranges (items never cross rows: one strip per stage), as few as
// the tile count per wave (<= convp_pp_max_nt) and the LDS (ring x stage + the epilogue slots <= 160 KB) allow.  Candidates
// are ranked by a per-item cost model -- supersteps x max(matrix cycles + ramp, staged bytes / fill rate), the rates read
// off profiles/r6_cprof_b256.txt -- summed over the items and divided over the CUs; IDQN_PP_PARTS<role> (debug build)
// overrides the choice for sweeps.  Returns IDQN_E_INVALID when no candidate fits (the caller keeps the one-item launch).
int plan_fwd_pp(idqn_handle_s* h, int role, int n_nets, int nb, const RoleGeom& g, FwdPlan** out) {
    auto key = std::make_tuple(role + 16, n_nets, nb, 0);
    (void)0;
    auto itp = h->fwd_plans.find(key);
    if (itp != h->fwd_plans.end()) { *out = &itp->second; return itp->second.n_items > 0 ? IDQN_OK : IDQN_E_INVALID; }
    char nm[32];
    role &= 7;  // (bit 3 marks the acting set's plans)
    snprintf(nm, sizeof nm, "IDQN_PP_PARTS%d", role);
    const int forced = debug_int(nm, 0), forced_ring = debug_int("IDQN_PP_RING", 0);
    const int NSS = g.KH * g.NCC, nm_prod = g.NPA == 3 ? 6 : 3, cus = cu_budget();
    const bool epi1 = role >= 3, planes_out = role != 2, f32_out = role == 2;
    int ow_max = 0;
    for (int v = 0; v < g.n_var; ++v) ow_max = std::max(ow_max, g.var[v].OW);
    FwdPlan best;
    double best_cost = 0;
    for (int parts = 1; parts <= ow_max; ++parts) {
        if (forced && parts != forced) continue;
        FwdPlan pl;
        int np_max = 0;
        double work = 0;  // cycles of all items of one slot
        bool ok = true;
        pl.row_parts = parts;
        for (int v = 0; v < g.n_var && ok; ++v) {
            const int OW = g.var[v].OW, OH = g.var[v].OH;
            if (parts > OW) { ok = false; break; }
            np_max = std::max(np_max, (OW + parts - 1) / parts);
            pl.r_begin[v] = pl.items_per_slot;
            pl.r_cnt[v] = OH * parts;
            pl.items_per_slot += OH * parts;
        }
        if (!ok) continue;
        pl.NT = (np_max * g.CT + 3) / 4;
        if (pl.NT < 2) pl.NT = 2;  // (the smallest kernel built)
        if (!convp_pp_built(g.NPA, g.CT, g.NQ, pl.NT) || NSS - 1 < pl.NT) continue;
        pl.stage = (size_t)(g.NQ * g.CT * 3 + ((np_max - 1) * g.SX + g.NQ) * g.NPA) * 1024;
        const size_t epi = convp_pp_epi_bytes(pl.NT, epi1 ? 1 : 0, planes_out, f32_out);
        pl.ring = (forced_ring != 2 && 3 * pl.stage + epi <= 160 * 1024) ? 3 : 2;
        pl.lds = pl.ring * pl.stage + epi;
        if (pl.lds > 160 * 1024) continue;
        for (int v = 0; v < g.n_var; ++v) {
            const int OW = g.var[v].OW, OH = g.var[v].OH;
            for (int part = 0; part < parts; ++part) {
                const int np = OW / parts + (part < OW % parts ? 1 : 0);
                const double mfma = (double)((np * g.CT + 3) / 4) * g.NQ * nm_prod * 32 + 450;
                const double fill = (double)(g.NQ * g.CT * 3 + ((np - 1) * g.SX + g.NQ) * g.NPA) * 1024 / (pl.ring == 3 ? 30.0 : 26.0);
                work += OH * (NSS * std::max(mfma, fill) + 600);
            }
        }
        pl.n_items = pl.items_per_slot * n_nets * nb;
        pl.n_wg = std::min(pl.n_items, cus);
        const int rounds = (pl.n_items + pl.n_wg - 1) / pl.n_wg;
        // whole launch: the slots' work over the CUs, stretched by the last round's idle CUs
        const double cost = work * n_nets * nb / pl.n_wg * ((double)rounds * pl.n_wg / pl.n_items);
        if (plan_print())
            fprintf(stderr, "[plan] pp role %d parts %d: %d items, NT %d, ring %d, stage %zu B, lds %zu B, model %.0f k cycles\n", role, parts,
                    pl.n_items, pl.NT, pl.ring, pl.stage, pl.lds, cost / 1e3);
        if (best.n_items == 0 || cost < best_cost) { best = pl; best_cost = cost; }
    }
    if (best.n_items > 0) {
        // the item table, in the launch order of the one-item kernels (convp_items.h)
        CFwdArgs ta;
        memset(&ta, 0, sizeof(ta));
        ta.items_per_slot = best.items_per_slot; ta.row_parts = best.row_parts; ta.range_major = role == 0; ta.nb = nb; ta.n_var = g.n_var;
        for (int v = 0; v < g.n_var; ++v) { ta.r_begin[v] = best.r_begin[v]; ta.r_cnt[v] = best.r_cnt[v]; ta.var[v] = g.var[v]; }
        std::vector<CItem> tab((size_t)best.n_items);
        IDQN_REQUIRE(convp_fill_pp_items(ta, best.n_items, tab.data()), "persistent plane conv: role %d ranges are no row cut", role);
        IDQN_HIP_CHECK(hipMalloc((void**)&best.items_dev, tab.size() * sizeof(CItem)));
        h->owned.push_back((void*)best.items_dev);
        IDQN_HIP_CHECK(hipMemcpy(best.items_dev, tab.data(), tab.size() * sizeof(CItem), hipMemcpyHostToDevice));
    }
    *out = &(h->fwd_plans[key] = best);
    if (best.n_items == 0) return IDQN_E_INVALID;
    if (plan_print())
        fprintf(stderr, "[plan] pp role %d nets %d nb %d: parts %d -> %d items on %d workgroups, NT %d, ring %d, stage %zu B, lds %zu B\n", role, n_nets,
                nb, best.row_parts, best.n_items, best.n_wg, best.NT, best.ring, best.stage, best.lds);
    return IDQN_OK;
}

int plan_wgrad(idqn_handle_s* h, int layer, int nb, WgradPlan** out, int n_chunks = 0) {
    if (n_chunks <= 0) n_chunks = h->npc[layer];
    auto key = std::make_tuple(layer, nb, n_chunks);
    auto itp = h->wgrad_plans.find(key);
    if (itp != h->wgrad_plans.end()) { *out = &itp->second; return IDQN_OK; }
    const ConvL& l = h->conv[layer];
    const int K = h->cfg.n_heads, npos = l.OH * l.OW, nch = std::min(n_chunks, std::min(h->npc[layer], npos));  // (the slab region holds npc chunks)
    WgradPlan pl;
    pl.n_chunks = nch;
    pl.MT = layer == 0 ? l.K : l.K * l.CI / 32;
    const long dy_pix = 3L * l.CO * 64, x_pix = (layer == 0 ? 1L : 3L) * l.CI * 64;
    for (pl.PG = layer == 0 ? 4 : 2;; --pl.PG) {  // positions per LDS stage: as many as two stages leave room for
        const long XB = layer == 0 ? (long)l.K * (pl.PG + 1) * 1024 : ((pl.PG - 1) * l.S + l.K) * x_pix;
        pl.lds = (size_t)(2 * (XB + pl.PG * dy_pix));
        if (pl.lds + 2048 <= 160 * 1024 || pl.PG == 1) break;
        if (layer == 0 && pl.PG > 2) --pl.PG;  // Conv_0: 4, 2 or 1 positions (never 0)
    }
    IDQN_REQUIRE(pl.lds + 2048 <= 160 * 1024, "plane wgrad: layer %d needs %zu bytes of LDS", layer, pl.lds);
    // item order = workgroup order (the XCD-contiguous remap gives an XCD consecutive items): head-major, so that the kernel
    // rows of one chunk share its x / dy strips through L2; Conv_0 chunk-major, because its K heads read the SAME staged
    // minibatch and a pixel strip then crosses the fabric once per XCD instead of once per head.  The kernel derives its
    // item (head, chunk, kernel row, balanced position range) from the workgroup index.
    pl.chunk_major = layer == 0 ? 1 : 0;
    pl.n_chunks = nch;
    pl.n_items = K * nch * (layer == 0 ? 1 : l.K);
    (void)nb;
    if (plan_print())
        fprintf(stderr, "[plan] wgrad layer %d: %d workgroups, %d chunks of ~%d positions, PG %d, MT %d, lds %zu B\n", layer,
                pl.n_items, nch, npos / nch, pl.PG, pl.MT, pl.lds);
    *out = &(h->wgrad_plans[key] = pl);
    return IDQN_OK;
}

// staging launch: pixels -> bf16 plane, conv kernels -> packed planes (forward kernels of every net of the set, and
// for the training set the data-gradient kernels of the K online nets).  `ring`: the step input of a replay-sourced training
// step -- the pixels are gathered from its frame ring and the sampled rows' scalars written to h->rp_action / _reward / _terminal
int planes_stage(idqn_handle_s* h, NetSet& s, const uint8_t* st, const uint8_t* st2, int B, int nb, hipStream_t q, const StepIn* ring) {
    StageArgs a;
    memset(&a, 0, sizeof(a));
    a.src[0] = st; a.src[1] = st2 ? st2 : st;
    a.x1 = s.x1; a.E = (long)h->gx.H * h->gx.W * h->gx.C; a.B = B; a.nb = nb; a.n_sets = s.n_in_sets;
    a.H = h->gx.H; a.W = h->gx.W; a.C = h->gx.C; a.lo_h = h->gx.lo_h; a.lo_w = h->gx.lo_w; a.Hp = h->gx.Hp; a.Wp = h->gx.Wp;
    a.n_prep_blocks = cdiv(a.E, 64) * nb * s.n_in_sets;
    a.wbase = s.wbase; a.wq = s.wq; a.wq_stride = h->wq_stride;
    const bool train = &s == &h->train;
    long blocks = 0;
    int nj = 0;
    for (int i = 0; i < 3; ++i) {
        const ConvL& l = h->conv[i];
        PackJob& j = a.job[nj++];
        j.src_off = l.w_off; j.dst_off = h->wq_fwd[i]; j.n_nets = s.n_nets;
        j.KHv = l.K; j.CT = l.CO / 32; j.mode = 0;
        if (i == 0) { j.NQ = l.K * l.CI / 16; j.NCC = 1; j.div255 = 1; } else { j.NQ = l.K; j.NCC = l.CI / 16; }
        j.KW = l.K; j.CI = l.CI; j.CO = l.CO; j.S = l.S;
        j.blocks_per_net = cdiv((long)j.KHv * j.NCC * j.NQ * j.CT * 64, 256);
        j.first_block = blocks;
        blocks += (long)j.blocks_per_net * j.n_nets;
    }
    for (int i = 2; i >= 1 && train; --i) {
        const ConvL& l = h->conv[i];
        const int KHs = l.K / l.S;
        for (int vi = 0; vi < l.S * l.S; ++vi) {
            IDQN_REQUIRE(nj < 8, "plane conv: more than 8 kernel blocks to pack");
            PackJob& j = a.job[nj++];
            j.src_off = l.w_off; j.dst_off = h->wq_dg[i] + (long)vi * KHs * KHs * l.CO * l.CI * 6; j.n_nets = h->cfg.n_heads;
            j.KHv = KHs; j.NQ = KHs; j.NCC = l.CO / 16; j.CT = l.CI / 32; j.mode = 1;
            j.KW = l.K; j.CI = l.CI; j.CO = l.CO; j.S = l.S; j.PLh = l.PLh; j.PLw = l.PLw; j.rh = vi / l.S; j.rw = vi % l.S; j.KHs = KHs;
            j.blocks_per_net = cdiv((long)j.KHv * j.NCC * j.NQ * j.CT * 64, 256);
            j.first_block = blocks;
            blocks += (long)j.blocks_per_net * j.n_nets;
        }
    }
    a.n_jobs = nj;
    if (train) { a.K = h->cfg.n_heads; a.count = h->count; a.bcinv = h->bcinv; a.b1 = h->ad.b1; a.b2 = h->ad.b2; }
    if (train && ring) {
        a.frames = (const uint8_t*)ring->frames; a.rows = ring->rows; a.n_frames = ring->n_frames; a.frame_bytes = ring->frame_bytes;
        a.act_out = h->rp_action; a.rew_out = h->rp_reward; a.term_out = h->rp_terminal;
        if (ring->slots_dev) return convp_launch_stage(a, a.n_prep_blocks + (int)blocks, q, nullptr, ring->slots_dev);
        const StageSlots slots = ring->slot_block<StageSlots>();
        return convp_launch_stage(a, a.n_prep_blocks + (int)blocks, q, &slots, nullptr);
    }
    if (debug_on("IDQN_STAGE_SKIP_PIXELS")) a.n_prep_blocks = 0;  // timing probe: the launch without its pixel half (wrong results)
    return convp_launch_stage(a, a.n_prep_blocks + (int)blocks, q);
}

// one plane conv launch: role 0..2 forward of Conv_0..2 for net set s, 3 / 4 data gradient of Conv_2 / Conv_1
// launch arguments + plan of a forward / data-gradient role, planned for about `target` workgroups
int conv_args(idqn_handle_s* h, NetSet& s, int role, int nb, int target, CFwdArgs& a, RoleGeom& g, FwdPlan*& pl) {
    int rc = role_geom(h, role, g);
    if (rc) return rc;
    const bool fwd = role <= 2;
    const int n_nets = fwd ? s.n_nets : h->cfg.n_heads;
    if ((rc = plan_fwd(h, role + (fwd && &s == &h->infer ? 8 : 0), n_nets, nb, g, &pl, target))) return rc;
    memset(&a, 0, sizeof(a));
    a.wq = s.wq;
    a.items_per_slot = pl->items_per_slot;
    for (int v = 0; v < 4; ++v) { a.r_begin[v] = pl->r_begin[v]; a.r_cnt[v] = pl->r_cnt[v]; }
    if (&s == &h->infer) { a.pbase[0] = a.pbase[1] = h->infer_pbase; a.n_first = 1; }
    else { a.pbase[0] = h->online; a.pbase[1] = h->target; a.n_first = h->cfg.n_heads; }
    a.pstride = h->L.head_stride; a.wq_stride = h->wq_stride; a.nb = nb; a.n_var = g.n_var;
    a.KH = g.KH; a.NCC = g.NCC; a.S = g.S; a.SX = g.SX;
    for (int v = 0; v < g.n_var; ++v) a.var[v] = g.var[v];
    const ActGeom* gin;   // input planes
    const ActGeom* gout;  // output planes
    if (fwd) {
        const ConvL& l = h->conv[role];
        const unsigned short* ins[3] = {s.x1, s.a1p, s.a2p};
        unsigned short* outs[3] = {s.a1p, s.a2p, nullptr};
        const ActGeom* gi[3] = {&h->gx, &h->ga1, &h->ga2};
        const ActGeom* go[3] = {&h->ga1, &h->ga2, &h->ga3};
        gin = gi[role]; gout = go[role];
        a.in = ins[role]; a.out3 = outs[role]; a.epilogue = 0; a.b_off = l.b_off; a.CO = l.CO;
        a.in_split = role == 0 ? (s.n_in_sets > 1 ? s.n_nets / 2 : s.n_nets + 1) : 0;
        a.range_major = role == 0;
        if (role == 2) { a.out_f32 = s.a3; a.f32_slot = h->ga3.block; a.f32_W = l.OW; }
        a.pix_bytes = g.NPA * l.CI * 64; a.plane_bytes = l.CI * 64;
        a.xstep = role == 0 ? 1024 : a.pix_bytes;
    } else {
        const int i = role == 3 ? 2 : 1;
        const ConvL& l = h->conv[i];
        gin = i == 2 ? &h->gda3 : &h->gda2;
        gout = i == 2 ? &h->gda2 : &h->gda1;
        const ActGeom* gm = i == 2 ? &h->ga2 : &h->ga1;
        a.in = i == 2 ? h->da3p : h->da2p;
        a.out3 = i == 2 ? h->da2p : h->da1p;
        a.mask3 = i == 2 ? s.a2p : s.a1p;
        a.pb = h->pbuf[i - 1];
        a.epilogue = 1; a.CO = l.CI; a.in_split = 0;
        a.mask_slot = gm->block * 6; a.mask_Wp = gm->Wp; a.mask_lo_h = gm->lo_h; a.mask_lo_w = gm->lo_w; a.mask_C = l.CI;
        a.pix_bytes = 3 * l.CO * 64; a.plane_bytes = l.CO * 64; a.xstep = a.pix_bytes;
    }
    a.in_slot = gin->block * (role == 0 ? 2 : 6);
    a.row_bytes = gin->Wp * a.pix_bytes;
    a.out_slot = gout->block * 6; a.out_Wp = gout->Wp; a.out_lo_h = gout->lo_h; a.out_lo_w = gout->lo_w;
    a.out_W = gout->W; a.out_H = gout->H;
    // The plan's item table: what it holds depends on the plan key (role and net set, nets, blocks, target) and the handle's
    // geometry only -- offsets, no pointers -- so it is made once, with the plan (a debug-build plan override is another key:
    // another plan, another table), and every later step only passes its address.
    if (!pl->desc_dev) {
        std::vector<CFwdDesc> tab((size_t)pl->n_items);
        IDQN_REQUIRE(convp_fill_fwd_items(a, pl->n_items, tab.data()), "plane conv: role %d has an item its descriptor cannot hold", role);
        CFwdDesc* dev = nullptr;
        IDQN_HIP_CHECK(hipMalloc((void**)&dev, tab.size() * sizeof(CFwdDesc)));
        h->owned.push_back((void*)dev);
        IDQN_HIP_CHECK(hipMemcpy(dev, tab.data(), tab.size() * sizeof(CFwdDesc), hipMemcpyHostToDevice));
        pl->desc_dev = dev;
    }
    a.items = pl->desc_dev;
    return IDQN_OK;
}

long long* conv_prof(idqn_handle_s* h, NetSet& s, int role, const FwdPlan* pl) {
    return (h->cprof && h->cprof_role == role && &s == &h->train && pl->n_items <= 4096) ? (long long*)h->cprof : nullptr;
}

int planes_conv(idqn_handle_s* h, NetSet& s, int role, int nb, hipStream_t q) {
    CFwdArgs a;
    RoleGeom g;
    FwdPlan* pl;
    int rc = conv_args(h, s, role, nb, cu_budget(), a, g, pl);
    if (rc) return rc;
    // several items per CU (many sample blocks or heads): the persistent form, where the first fill, the table arithmetic
    // and the epilogue of an item run beside another item's matrix loop (convp_pp.hip).  IDQN_CONV_PP=0: one item per workgroup.
    static const int pp_roles = getenv("IDQN_CONV_PP") ? atoi(getenv("IDQN_CONV_PP")) : 15;  // bit r: role r (role 4, the Conv_1 data gradient, measured flat: profiles/r6_pp_ab.txt)
    if (((pp_roles >> role) & 1) && pl->n_items > cu_budget()) {
        FwdPlan* pp;
        const bool fwd = role <= 2;
        if (plan_fwd_pp(h, role + (fwd && &s == &h->infer ? 8 : 0), fwd ? s.n_nets : h->cfg.n_heads, nb, g, &pp) == IDQN_OK) {
            a.items_per_slot = pp->items_per_slot;
            for (int v = 0; v < 4; ++v) { a.r_begin[v] = pp->r_begin[v]; a.r_cnt[v] = pp->r_cnt[v]; }
            a.row_parts = pp->row_parts;
            return convp_launch_fwd_pp(a, g.NPA, g.CT, g.NQ, pp->NT, pp->n_items, pp->n_wg, pp->stage, pp->ring, pp->lds, q, pp->items_dev,
                                       conv_prof(h, s, role, pl));
        }
    }
    return convp_launch_fwd(a, g.NPA, g.CT, g.NQ, pl->NT, pl->n_items, pl->stage, pl->ring, pl->lds, q, conv_prof(h, s, role, pl));
}

// launch arguments + plan of a weight-gradient layer cut into n_chunks position chunks (0: the layer's default)
int wgrad_args(idqn_handle_s* h, int layer, int nb, int n_chunks, CWgradArgs& a, WgradPlan*& pl) {
    NetSet& s = h->train;
    const ConvL& l = h->conv[layer];
    int rc = plan_wgrad(h, layer, nb, &pl, n_chunks);
    if (rc) return rc;
    const unsigned short* xs[3] = {s.x1, s.a1p, s.a2p};
    const unsigned short* dys[3] = {h->da1p, h->da2p, h->da3p};
    const ActGeom* gx[3] = {&h->gx, &h->ga1, &h->ga2};
    const ActGeom* gd[3] = {&h->gda1, &h->gda2, &h->gda3};
    memset(&a, 0, sizeof(a));
    a.x = xs[layer]; a.dy = dys[layer]; a.pb = h->pbuf[layer]; a.slab = h->slab + h->slab_off[layer];
    a.n_chunks = pl->n_chunks; a.chunk_major = pl->chunk_major; a.kh_per_item = layer == 0 ? 1 : l.K;
    const int npx = layer == 0 ? 1 : 3;
    a.x_slot = gx[layer]->block * 2 * npx; a.dy_slot = gd[layer]->block * 6; a.slab_stride = h->slab_stride[layer];
    a.x_shared = layer == 0 ? 1 : 0;
    a.K = h->cfg.n_heads; a.nb = nb; a.KH = l.K; a.KW = l.K; a.S = l.S; a.CI = l.CI; a.CO = l.CO; a.OH = l.OH; a.OW = l.OW;
    a.x_pix = npx * l.CI * 64; a.x_plane = l.CI * 64; a.x_row = gx[layer]->Wp * a.x_pix;
    a.dy_pix = 3 * l.CO * 64; a.dy_Wp = gd[layer]->Wp; a.dy_lo_h = gd[layer]->lo_h; a.dy_lo_w = gd[layer]->lo_w;
    a.PG = pl->PG; a.out_div = layer == 0 ? 255.0f : 1.0f;
    return IDQN_OK;
}

int planes_wgrad(idqn_handle_s* h, int layer, int nb, hipStream_t q) {
    CWgradArgs a;
    WgradPlan* pl;
    int rc = wgrad_args(h, layer, nb, 0, a, pl);
    if (rc) return rc;
    const int NPX = layer == 0 ? 1 : 3, CT = h->conv[layer].CO / 32;
    h->npc_used[layer] = pl->n_chunks;
    return convp_launch_wgrad(a, NPX, pl->MT, CT, pl->n_items, pl->lds, q);
}

// Data gradient of conv `layer` and weight gradient of the same layer in ONE launch (convp_pair.hip) when that pair of
// kernels is built for the plans; *done = false: nothing was launched, the caller runs them one after the other.
int planes_pair(idqn_handle_s* h, int layer, int nb, hipStream_t q, bool* done) {
    *done = false;
    const int cus = cu_budget();
    if (layer < 1 || layer > 2) return IDQN_OK;
    // experiment knobs: IDQN_PAIR_D<layer> = workgroups planned for the data gradient, IDQN_PAIR_C<layer> = position chunks
    // of the weight gradient (default: what the data gradient leaves of the 256 CUs)
    auto knob = [&](const char* stem, int dflt) {
        char nm[32];
        snprintf(nm, sizeof nm, "%s%d", stem, layer);
        const char* e = debug_env(nm);
        return e ? atoi(e) : dflt;
    };
    const int d_target = knob("IDQN_PAIR_D", cus / 2);
    NetSet& s = h->train;
    const int role = layer == 2 ? 3 : 4, K = h->cfg.n_heads;
    const ConvL& l = h->conv[layer];
    CFwdArgs f;
    RoleGeom g;
    FwdPlan* pf;
    int rc = conv_args(h, s, role, nb, d_target, f, g, pf);
    if (rc) return rc;
    const int n_chunks = std::min(knob("IDQN_PAIR_C", 1 << 20), (cus - pf->n_items) / (K * l.K));  // what is left of the chip, in whole position chunks
    if (n_chunks < 1) return IDQN_OK;
    CWgradArgs w;
    WgradPlan* pw;
    if ((rc = wgrad_args(h, layer, nb, n_chunks, w, pw))) return rc;
    const int WCT = l.CO / 32, ntw = (pw->MT * WCT + 3) / 4;
    if (pf->n_items + pw->n_items > cus || !convp_pair_built(g.NPA, g.CT, g.NQ, pf->NT, 3, WCT, ntw, pw->PG)) return IDQN_OK;
    h->npc_used[layer] = pw->n_chunks;
    *done = true;
    return convp_launch_pair(f, g.NPA, g.CT, g.NQ, pf->NT, pf->n_items, pf->stage, pf->ring, pf->lds, w, 3, pw->MT, WCT, pw->n_items,
                             pw->lds, q, conv_prof(h, s, role, pf));
}

// ---- forward of a net set: staging, 3 convs, Dense_0 partials -----------------------------------
// (`ring`: planes_stage)
int cnn_forward(idqn_handle_s* h, NetSet& s, const uint8_t* st, const uint8_t* st2, int B, hipStream_t q, bool with_dense0 = true,
                const StepIn* ring = nullptr) {
    const int nb = cdiv(B, 32);
    IDQN_REQUIRE(nb <= s.nb_cap, "batch %d exceeds the workspace (%d blocks of 32)", B, s.nb_cap);
    if (h->planes) {
        static const char* nm[3] = {"conv0 fwd", "conv1 fwd", "conv2 fwd"};
        int rc = planes_stage(h, s, st, st2, B, nb, q, ring);
        tl_mark(h, q, "stage (pixels + kernel packing)");
        for (int i = 0; i < 3 && !rc; ++i) { rc = planes_conv(h, s, i, nb, q); tl_mark(h, q, nm[i]); }
        if (rc) return rc;
    } else {
        PrepArgs pa;
        pa.src[0] = st; pa.src[1] = st2 ? st2 : st;
        pa.x = s.x;
        pa.E = (long)h->gx.H * h->gx.W * h->gx.C; pa.B = B; pa.nb = nb; pa.n_sets = s.n_in_sets; pa.g = h->gx;
        hipLaunchKernelGGL(k_prep_u8, dim3(cdiv(pa.E, 64), nb, s.n_in_sets), dim3(256), 0, q, pa);
        const float* ins[3] = {s.x, s.a1, s.a2};
        float* outs[3] = {s.a1, s.a2, s.a3};
        const ActGeom* gin[3] = {&h->gx, &h->ga1, &h->ga2};
        const ActGeom* gout[3] = {&h->ga1, &h->ga2, &h->ga3};
        for (int i = 0; i < 3; ++i) {
            const ConvL& l = h->conv[i];
            ConvFwdArgs a;
            memset(&a, 0, sizeof(a));
            a.in = ins[i]; a.out = outs[i]; a.wbase = s.wbase; a.wt_base = nullptr; a.in_set = (i == 0) ? s.in_set : s.ident;
            a.b_off = l.b_off; a.in_block = gin[i]->block; a.out_block = gout[i]->block;
            a.n_nets = s.n_nets; a.nb = nb; a.n_var = 1; a.epilogue = 0;
            a.KH = l.K; a.KWCI = l.K * l.CI; a.S = l.S; a.CI = l.CI; a.CO = l.CO; a.IWp = gin[i]->Wp;
            a.out_Wp = gout[i]->Wp; a.out_lo_h = gout[i]->lo_h; a.out_lo_w = gout[i]->lo_w;
            IDQN_REQUIRE(a.KWCI % 32 == 0, "conv %d: a kernel row of %d (kw, ci) rows is not a multiple of the 32-row chunk", i, a.KWCI);
            const int npw = (l.CO == 32) ? 4 : 2;  // positions per workgroup
            ConvVariant& v = a.var[0];
            v.w_off = l.w_off; v.in_off_h = 0; v.in_off_w = 0; v.OH = l.OH; v.OW = l.OW;
            v.out_mul = 1; v.out_add_h = 0; v.out_add_w = 0; v.pg_begin = 0;
            a.npg = cdiv(l.OH * l.OW, npw);
            a.n_items = (long)s.n_nets * nb * a.npg;
            if (l.CO == 32)
                hipLaunchKernelGGL((k_conv_fwd<1, 1>), dim3((unsigned)a.n_items), dim3(256), 0, q, a);
            else
                hipLaunchKernelGGL((k_conv_fwd<2, 1>), dim3((unsigned)a.n_items), dim3(256), 0, q, a);
        }
    }
    if (!with_dense0) {  // (the i-IQN heads take the trunk features from here)
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    if (&s == &h->train && nb > 1) s.NS = d0_splits(h, s.n_nets, nb);  // (nb == 1: the value cnn_setup chose)
    else if (&s == &h->train) s.NS = h->NS;
    DenseFwdArgs d;
    d.in = s.a3; d.part = s.part; d.wbase = s.wbase; d.w_off = h->off_w0;
    d.n_nets = s.n_nets; d.nb = nb; d.NS = s.NS; d.n_jt = h->J / 128; d.F = h->F; d.J = h->J;
    d.bb_inner = (h->planes && nb > 1) ? 1 : 0;
    d.n_items = (long)s.n_nets * nb * d.NS * d.n_jt;
    d.net_rot = s.n_in_sets > 1 ? s.n_nets / 2 : 0;
    // the online nets' Dense_0 kernels (re-read by the fused update of the same step) with default-policy loads: k_dense0_fwd3
    // (K <= 3: the frozen target nets' kernels fit beside the online ones -- 2 K F J 4 <= 100 MB -- and are found on chip step after step:
    // K = 2 -3 us, K = 3 -2 us, K = 4 the same)
    const bool keep_target = d0_keep_online(h) && 2L * h->cfg.n_heads * h->F * h->J * 4 <= 100L << 20;
    // (the online nets' loads are default-policy for ANY number of heads: where nothing can stay on chip the fused update still runs 3-6 % faster behind
    // them -- K = 6 / 7 / 16 / 32: step -3.5 / -5 / -5 / -6 us, K = 8 / 64 the same; what depends on the size is only the store policy of theta_new)
    d.nt_from = s.n_in_sets > 1 ? (keep_target ? s.n_nets : s.n_nets / 2) : 0;
    // >= 8 sample blocks per net (B = 256): the tiled bf16x3 GEMM of the i-IQN heads (iqn_gemm.h: 256 x 256 tiles, operands split in
    // registers and parked in LDS as MFMA fragments) -- the same interleaved split-K and product order, so the same partials
    // layout for k_hidden; splits chosen to fill the chip (debug build, IDQN_D0_FWD_GEMM=0: the block-inner streaming kernel k_dense0_fwd3b).
    static const bool fwd_gemm = debug_int("IDQN_D0_FWD_GEMM", 1) != 0;
    if (fwd_gemm && h->planes && &s == &h->train && nb % 8 == 0 && h->J % 256 == 0 && h->F % 16 == 0) {
        const int per_split = s.n_nets * (nb / 8) * (h->J / 256);
        const int nsg = std::max(1, std::min(std::min(256 / std::max(1, per_split), 64), h->F / 16));
        if ((long)nb * nsg <= s.part_slabs) {
            s.NS = nsg;
            IqnD0FwdArgs g;
            g.x = s.a3; g.wbase = s.wbase; g.part = s.part; g.w_off = h->off_w0;
            g.V = s.n_nets; g.nb = nb; g.NS = nsg; g.F = h->F; g.J = h->J; g.clk = nullptr;
            const size_t lds = 2 * (size_t)IG_STAGE;
            static LdsAttrMark attr;
            if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_fwd<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_iqn_d0_fwd<2>, dim3((unsigned)(per_split * nsg)), dim3(512), lds, q, g);
            tl_mark(h, q, "dense0 fwd (tiled GEMM)");
            IDQN_HIP_CHECK(hipGetLastError());
            return IDQN_OK;
        }
    }
    if (h->planes) {
        if (d.bb_inner) hipLaunchKernelGGL(k_dense0_fwd3b, dim3(cdiv(d.n_items, 4)), dim3(256), 0, q, d);
        else {
            // fewer than 256 four-wave workgroups (plain DQN: 2 nets x 64 splits x 4 column tiles): two waves each, so that every
            // CU streams (a CU is the unit of streaming bandwidth)
            const int wpw = d.n_items <= 512 ? 2 : 4;
            hipLaunchKernelGGL(k_dense0_fwd3, dim3(cdiv(d.n_items, wpw)), dim3(64 * wpw), 0, q, d);
        }
    } else hipLaunchKernelGGL(k_dense0_fwd, dim3(cdiv(d.n_items, 4)), dim3(256), 0, q, d);
    tl_mark(h, q, "dense0 fwd");
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

void fill_adam_args(idqn_handle_s* h, long begin, long end, long skip_b, long skip_e, bool from_slabs, bool epilogue, AdamArgs& a);
int launch_adam(idqn_handle_s* h, long begin, long end, long skip_b, long skip_e, bool from_slabs, hipStream_t q, bool epilogue = false) {
    AdamArgs a;
    IDQN_REQUIRE(skip_b == skip_e || (skip_b >= begin && skip_e <= end && skip_b % 4 == 0 && skip_e % 4 == 0),
                 "launch_adam: bad skip range");
    fill_adam_args(h, begin, end, skip_b, skip_e, from_slabs, epilogue, a);
    hipLaunchKernelGGL(k_adam, dim3(cdiv(end - begin - (skip_e - skip_b), 256), h->cfg.n_heads), dim3(256), 0, q, a);  // 4 lanes per float4
    tl_mark(h, q, "adam (small leaves + slab sums)");
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// arguments of the weight-gradient launch of conv layer i (shared by the plain and the mixed launch)
ConvWgradArgs make_wgrad_args(idqn_handle_s* h, int i, int nb) {
    NetSet& s = h->train;
    const ConvL& l = h->conv[i];
    const float* acts_in[3] = {s.x, s.a1, s.a2};
    const float* douts[3] = {h->da1, h->da2, h->da3};
    const ActGeom* gact[3] = {&h->gx, &h->ga1, &h->ga2};
    const ActGeom* gdo[3] = {&h->gda1, &h->gda2, &h->gda3};
    ConvWgradArgs a;
    a.in = acts_in[i]; a.dout = douts[i]; a.slab = h->slab + h->slab_off[i];
    a.in_net_stride = (i == 0) ? 0 : (long)nb * gact[i]->block;
    a.slab_stride = h->slab_stride[i];
    a.K = h->cfg.n_heads; a.nb = nb; a.npc = h->npc[i]; a.KH = l.K; a.S = l.S; a.CO = l.CO;
    a.OH = l.OH; a.OW = l.OW; a.pos_per_chunk = h->pos_per_chunk[i];
    a.gin = *gact[i]; a.gd = *gdo[i]; a.in_C = l.CI;
    if (i == 0) { a.KWe = 1; a.CIe = l.K * l.CI; } else { a.KWe = l.K; a.CIe = l.CI; }
    a.n_items = (long)a.K * a.KH * a.KWe * a.npc;  // workgroups
    return a;
}

// arguments of the data-gradient launch of conv layer i (1 or 2): a stride-1 forward convolution over dout with the
// transformed kernels of k_wt_build, one variant per output parity
int make_dgrad_args(idqn_handle_s* h, int i, int nb, ConvFwdArgs& a) {
    NetSet& s = h->train;
    const int K = h->cfg.n_heads;
    const ConvL& l = h->conv[i];
    const float* douts[3] = {h->da1, h->da2, h->da3};
    const ActGeom* gdo[3] = {&h->gda1, &h->gda2, &h->gda3};
    const float* acts_in[3] = {s.x, s.a1, s.a2};
    const ActGeom* gact[3] = {&h->gx, &h->ga1, &h->ga2};
    float* dins[3] = {nullptr, h->da1, h->da2};
    const ActGeom* gdi[3] = {nullptr, &h->gda1, &h->gda2};
    const int KHs = l.K / l.S, nvar = l.S * l.S;
    memset(&a, 0, sizeof(a));
    a.in = douts[i]; a.out = dins[i]; a.wbase = s.wbase; a.wt_base = h->wt[i]; a.wt_stride = h->wt_stride[i];
    a.in_set = s.ident; a.mask = acts_in[i];
    a.in_block = gdo[i]->block; a.out_block = gdi[i]->block; a.mask_block = gact[i]->block;
    a.n_nets = K; a.nb = nb; a.n_var = nvar; a.epilogue = 1;
    a.KH = KHs; a.KWCI = KHs * l.CO; a.S = 1; a.CI = l.CO; a.CO = l.CI; a.IWp = gdo[i]->Wp;
    a.out_Wp = gdi[i]->Wp; a.out_lo_h = gdi[i]->lo_h; a.out_lo_w = gdi[i]->lo_w;
    a.mask_Wp = gact[i]->Wp; a.mask_lo_h = gact[i]->lo_h; a.mask_lo_w = gact[i]->lo_w;
    IDQN_REQUIRE(a.KWCI % 32 == 0, "conv %d dgrad: %d rows per kernel row is not a multiple of 32", i, a.KWCI);
    const int npw = (l.CI == 32) ? 4 : 2;
    int pg = 0;
    for (int vi = 0; vi < nvar; ++vi) {
        const int rh = vi / l.S, rw = vi % l.S;
        const int ph = (rh + l.PLh) % l.S, pw = (rw + l.PLw) % l.S;
        ConvVariant& v = a.var[vi];
        v.w_off = (long)vi * KHs * KHs * l.CO * l.CI;
        v.in_off_h = (rh + l.PLh - ph) / l.S + gdo[i]->lo_h - KHs + 1;
        v.in_off_w = (rw + l.PLw - pw) / l.S + gdo[i]->lo_w - KHs + 1;
        v.OH = (l.IH - rh + l.S - 1) / l.S; v.OW = (l.IW - rw + l.S - 1) / l.S;
        v.out_mul = l.S; v.out_add_h = rh; v.out_add_w = rw; v.pg_begin = pg;
        IDQN_REQUIRE(v.in_off_h >= 0 && v.in_off_w >= 0 && v.OH > 0 && v.OW > 0, "conv %d dgrad: bad variant geometry", i);
        pg += cdiv(v.OH * v.OW, npw);
    }
    a.npg = pg;
    a.n_items = (long)K * nb * a.npg;
    return IDQN_OK;
}

int cnn_backward_rest(idqn_handle_s* h, int B, bool fuse_adam, hipStream_t q);

// Dense_0 weight gradient (+ fused Adam) over nb_total sample blocks addressed through (outer, head, inner) strides
int launch_dense0_wgrad(idqn_handle_s* h, const float* a3, const float* dh, int nb_total, int nb_inner, long a3_outer,
                        long a3_head, long a3_inner, long dh_outer, long dh_head, long dh_inner, bool fuse_adam,
                        bool profile, hipStream_t q, bool fuse_dg = false) {
    const int K = h->cfg.n_heads;
    DenseWgradArgs dw;
    dw.dpart = h->dpart;
    dw.a3p = dw.dhp = nullptr;
    // The fused update over a GLOBAL batch (factored data-parallel step, >= 2 sample blocks per head): the factors are
    // split into bf16 planes once and the contraction runs at the bf16 MFMA rate.
    const bool bf3 = h->planes && fuse_adam && !fuse_dg && nb_total >= 2 && h->J % 256 == 0;
    if (bf3) {
        if (h->fact_planes_cap < nb_total) {  // (first step of a job, or a larger world: outside any timed region)
            if (h->fact_planes) { IDQN_HIP_CHECK(hipStreamSynchronize(q)); IDQN_HIP_CHECK(hipFree(h->fact_planes)); }
            IDQN_HIP_CHECK(hipMalloc((void**)&h->fact_planes, (size_t)3 * nb_total * K * (h->F + h->J) * 32 * 2));
            h->fact_planes_cap = nb_total;
        }
        SplitFactorsArgs sa;
        sa.a3 = a3; sa.dh = dh; sa.a3_outer = a3_outer; sa.a3_head = a3_head; sa.a3_inner = a3_inner;
        sa.dh_outer = dh_outer; sa.dh_head = dh_head; sa.dh_inner = dh_inner;
        sa.K = K; sa.nb = nb_total; sa.nb_inner = nb_inner; sa.F = h->F; sa.J = h->J;
        sa.a3p = h->fact_planes; sa.dhp = h->fact_planes + (long)3 * nb_total * K * h->F * 32;
        // The default update kernel (k_dense0_wgrad_alds<1>) splits its a3 tiles itself, straight from the gathered f32 factors:
        // only dL/dh (6 % of the factor bytes) goes through the plane copy.
        sa.a3p = nullptr;
        hipLaunchKernelGGL(k_split_factors, dim3((unsigned)cdiv((long)h->J * 4, 256), (unsigned)(nb_total * K)), dim3(256), 0, q, sa);
        tl_mark(h, q, "factor planes");
        dw.a3p = sa.a3p; dw.dhp = sa.dhp;
    }
    dw.a3 = a3; dw.dh = dh; dw.grad = h->grad; dw.theta = h->online; dw.mu = h->mu; dw.nu = h->nu;
    dw.bcinv = h->bcinv; dw.ad = h->ad; dw.g_w0_base = h->g_w0_base; dw.g_w0_stride = h->g_w0_end - h->g_w0_begin;
    dw.w_off = h->off_w0; dw.P = h->L.head_stride;
    dw.a3_outer = a3_outer; dw.a3_head = a3_head; dw.a3_inner = a3_inner;
    dw.dh_outer = dh_outer; dw.dh_head = dh_head; dw.dh_inner = dh_inner;
    h->d0_rows = false;
    const int nq = (h->J % 256 == 0) ? 2 : 1;  // 256- or 128-wide column tiles
    dw.K = K; dw.nb = nb_total; dw.nb_inner = nb_inner; dw.n_ft = h->F / 32; dw.n_jt = h->J / (128 * nq);
    dw.F = h->F; dw.J = h->J; dw.item0 = 0; dw.keep_heads = d0_keep_heads(h);
    dw.da3p = nullptr; dw.da3f = nullptr; dw.pb = nullptr; dw.C = 0; memset(&dw.g, 0, sizeof(dw.g));

    dw.n_items = (long)K * dw.n_ft * dw.n_jt;  // workgroups
    const dim3 wgrid((unsigned)dw.n_items);
    // profiling: the start / stop events ride on the kernel's own dispatch packet (hipExtLaunchKernelGGL), so the
    // elapsed time is the kernel's, without the gaps that separate marker packets from their neighbours
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) {
        e0 = h->ev[h->ev_used]; e1 = h->ev[h->ev_used + 1];
        h->ev_used += 2;
    }
    // (the extended launch only when there is something to time: it is not a capturable node of a step graph)
#define D0W_LAUNCH(...)                                                                                   \
    do {                                                                                                  \
        if (e0) hipExtLaunchKernelGGL((k_dense0_wgrad<__VA_ARGS__>), wgrid, dim3(256), 0, q, e0, e1, 0, dw); \
        else hipLaunchKernelGGL((k_dense0_wgrad<__VA_ARGS__>), wgrid, dim3(256), 0, q, dw);               \
    } while (0)
    // Default where it applies (one sample block, J = 512, nothing deferred): one workgroup per PAIR of column tiles
    // (dense0_pair_body) -- the second tile's requests go out under the first tile's last phase, and the workgroup finishes
    // dL/da3 itself (it holds both partials): no partials in HBM, no k_da3_finalize launch, no hand-off.  Bit-identical.
    // Measured on three boxes against two workgroups + finalize (profiles/r4_d0_pair_ab.txt): step -0.7 / -3 / -5 us; the kernel
    // itself takes 2 - 5 us more than the tile kernel (a row's two 1 KB halves are streamed 12 us apart instead of side by side by
    // sibling workgroups), the finalize launch it replaces took 5.3 us + a boundary.
    const bool pair = fuse_adam && nq == 2 && fuse_dg && nb_total == 1 && h->J == 512;
    if (pair) {
        // one workgroup per PAIR of column tiles; the launch finishes dL/da3 itself
        dw.da3p = h->da3p; dw.da3f = h->da3; dw.pb = h->pbuf[2]; dw.g = h->gda3; dw.C = h->conv[2].CO;
        h->d0_rows = true;
        const dim3 pgrid((unsigned)(K * dw.n_ft));
        // one or two heads at the Nature width: theta, m, v and the target nets (4 x 16 MB per head) fit the memory-side cache beside the step's
        // other traffic -- every stream of the update default-policy (K = 1 -1.9 us, K = 2 -4 us; K = 3 +5, K = 5 +16: profiles/r5_d0_keep_online_ab.txt)
        const bool keep_all = d0_keep_online(h) && 4L * K * h->F * h->J * 4 <= 128L << 20;
        // heads [0, keep) keep theta_new on chip, the others store it non-temporally: one launch per policy (a kernel with both bodies spills)
        const int keep = keep_all ? K : std::min(dw.keep_heads, K);
        for (int part = 0; part < 2; ++part) {
            const int k0 = part == 0 ? 0 : keep, k1 = part == 0 ? keep : K;
            if (k1 <= k0) continue;
            DenseWgradArgs dp = dw;
            dp.item0 = k0 * dw.n_ft;
            const dim3 grid((unsigned)((k1 - k0) * dw.n_ft));
            hipEvent_t s0 = (e0 && k0 == 0) ? e0 : nullptr, s1 = (e0 && k1 == K) ? e1 : nullptr;
            const void* fn = keep_all ? (const void*)k_dense0_wgrad_pair<false, false, true>
                             : part == 0 ? (const void*)k_dense0_wgrad_pair<false, false, false> : (const void*)k_dense0_wgrad_pair<false, true, false>;
            void* args[] = {&dp};
            if (s0 || s1) IDQN_HIP_CHECK(hipExtLaunchKernel(fn, grid, dim3(256), args, 0, q, s0, s1, 0));
            else IDQN_HIP_CHECK(hipLaunchKernel(fn, grid, dim3(256), args, 0, q));
        }
    } else if (fuse_adam && nq == 2 && fuse_dg) D0W_LAUNCH(true, 2, true);
    else if (bf3) {  // the factored data-parallel update over >= 2 sample blocks: a3 fragments through LDS
        const int keep = std::min(dw.keep_heads, K);
        for (int part = 0; part < 2; ++part) {  // (one launch per cache policy of theta_new, as for the pair kernel)
            const int k0 = part == 0 ? 0 : keep, k1 = part == 0 ? keep : K;
            if (k1 <= k0) continue;
            DenseWgradArgs dp = dw;
            dp.item0 = k0 * dw.n_ft * dw.n_jt;
            const dim3 grid((unsigned)((k1 - k0) * dw.n_ft * dw.n_jt));
            hipEvent_t s0 = (e0 && k0 == 0) ? e0 : nullptr, s1 = (e0 && k1 == K) ? e1 : nullptr;
            const void* fn = part == 0 ? (const void*)k_dense0_wgrad_alds<1, false> : (const void*)k_dense0_wgrad_alds<1, true>;
            void* args[] = {&dp};
            if (s0 || s1) IDQN_HIP_CHECK(hipExtLaunchKernel(fn, grid, dim3(256), args, 0, q, s0, s1, 0));
            else IDQN_HIP_CHECK(hipLaunchKernel(fn, grid, dim3(256), args, 0, q));
        }
    }
    else if (fuse_adam && nq == 2) D0W_LAUNCH(true, 2);
    else if (fuse_adam) D0W_LAUNCH(true, 1);
    else if (nq == 2) D0W_LAUNCH(false, 2);
    else D0W_LAUNCH(false, 1);
#undef D0W_LAUNCH
    tl_mark(h, q, fuse_dg ? "dense0 wgrad + dgrad + adam" : fuse_adam ? "dense0 wgrad + adam" : "dense0 wgrad");
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

int cnn_backward(idqn_handle_s* h, const StepIn& in, hipStream_t q) {
    const int B = in.batch, Bdiv = in.mean_divisor;
    const bool fuse_adam = !in.grads_only(), profile = in.profile(), stop_after_dense0 = in.stop0(), stop_before_dense0_wgrad = in.stopb();
    const int K = h->cfg.n_heads, nb = cdiv(B, 32);
    NetSet& s = h->train;
    const ConvL *c0 = &h->conv[0], *c1 = &h->conv[1], *c2 = &h->conv[2];
    // head: h + Dense_1 partials for all 2K nets, then TD / loss / dL/dq / dL/dh / Dense_1 + Dense_0-bias gradients
    HiddenArgs hi;
    hi.part = s.part; hi.wbase = s.wbase; hi.b0_off = h->off_b0; hi.w1_off = h->off_w1; hi.nb = nb; hi.NS = s.NS;
    hi.J = h->J; hi.A = h->cfg.n_actions; hi.hbuf = h->hbuf; hi.qpart = h->qpart;
    hipLaunchKernelGGL(k_hidden, dim3(h->J / 32, 2 * K * nb), dim3(256), 0, q, hi);
    tl_mark(h, q, "hidden");
    TdArgs ta;
    ta.hbuf = h->hbuf; ta.qpart = h->qpart; ta.wbase = s.wbase; ta.b0_off = h->off_b0; ta.w1_off = h->off_w1;
    ta.b1_off = h->off_b1; ta.P = h->L.head_stride; ta.K = K;
    {
        const long w0n = h->g_w0_end - h->g_w0_begin;
        ta.gP = h->gP; ta.g_b0_off = h->off_b0 - w0n; ta.g_w1_off = h->off_w1 - w0n; ta.g_b1_off = h->off_b1 - w0n;
    } ta.nb = nb; ta.J = h->J; ta.A = h->cfg.n_actions;
    ta.B = B; ta.Bdiv = Bdiv; ta.action = in.action; ta.reward = in.reward; ta.terminal = in.terminal; ta.gamma_n = h->gamma_n;
    ta.prof = (h->cprof && h->cprof_role == 9) ? (long long*)h->cprof : nullptr;
    ta.dh = dh_of(h, nb); ta.q_dbg = h->qdbg; ta.grad = h->grad; ta.losses = h->losses;
    ta.count = h->count; ta.bcinv = h->bcinv; ta.b1 = h->ad.b1; ta.b2 = h->ad.b2;
    ta.cum = h->cum; ta.finish_step = fuse_adam ? 1 : 0;
    ta.is_weight = in.is_weight; ta.td_abs = in.td_abs; ta.bpart = nullptr; ta.bctr = nullptr;
    ta.bcinv_done = h->planes ? 1 : 0;  // (the plane path's staging launch writes the bias corrections)
    h->wt_ready = false;
    if (!h->planes) {  // (the plane path packs the data-gradient kernels in its staging launch)
        WtBuildArgs wb;
        const int nx = wt_build_args(h, wb);
        hipLaunchKernelGGL(k_td_dh_wt, dim3((h->J / 32) * K + nx * K * 2), dim3(256), 0, q, ta, wb, nx);
        h->wt_ready = true;
    } else {
        // several sample blocks: one workgroup per block, the last to arrive adds the blocks' gradient partials in block order
        const bool per_block = nb > 1 && h->td_bpart && debug_int("IDQN_TD_PER_BLOCK", 1);
        if (per_block) { ta.bpart = h->td_bpart; ta.bctr = h->td_bctr; }
        hipLaunchKernelGGL(k_td_dh, dim3(h->J / 32, K, per_block ? nb : 1), dim3(256), 0, q, ta);
    }
    tl_mark(h, q, "td + loss + dh");
    // Dense_0 data gradient -> da3 (zero-bordered for the Conv_2 data gradient).  On the fused single-device path it is
    // computed INSIDE the weight-gradient + Adam kernel (theta streams once) and finished by k_da3_finalize; the two-call
    // paths of the data-parallel step need it before the weight gradient and keep the separate kernel.
    // Several sample blocks on ONE device (B > 32): the schedule of the factored data-parallel step without its collectives -- the
    // data gradient as its own launch, the factors split once into bf16 planes, the update contracting them at the bf16 MFMA rate
    // (k_dense0_wgrad_alds) -- instead of the fused kernel's f32 MFMAs over every block (B = 256: profiles/r5_b256_ab.txt)
    const bool many = nb >= 3 && h->planes && h->J % 256 == 0;  // (two blocks: the same either way, 0.5065 against 0.5085 ms)
    const bool fuse_dg = fuse_adam && !stop_after_dense0 && !stop_before_dense0_wgrad && h->dpart && !many;
    // eight (or a multiple of eight) local sample blocks: the data gradient as the tiled bf16x3 GEMM the i-IQN heads use for their
    // fraction blocks (csrc/iqn_gemm.h: W read once per group of 8 blocks, products at the bf16 rate) + the finalize launch for the
    // ReLU mask / planes / per-position sums, instead of one f32-MFMA pass over W per block
    if (!fuse_dg && many && nb % 8 == 0 && h->dpart && h->J % 16 == 0) {
        IqnD0DgradArgs g;
        g.dh = dh_of(h, nb); g.wbase = s.wbase; g.dx = h->dpart; g.w_off = h->off_w0; g.K = K; g.nb = nb; g.F = h->F; g.J = h->J;
        const size_t lds = 2 * (size_t)IG_STAGE;
        // rows of W per workgroup (64 x row tiles per wave): what fills the chip -- rounds of items x length of an item (K = 5, 8 blocks:
        // 205 items of 192 rows in one round instead of 155 of 256)
        int rt = 4;
        {
            long best = 0;
            for (int c = 4; c >= 2; --c) {
                const long cost = (long)cdiv((long)K * (nb / 8) * cdiv(h->F, 64 * c), cu_budget()) * c;
                if (c == 4 || cost < best) { best = cost; rt = c; }
            }
            if (debug_int("IDQN_DGRAD_RT", 0) >= 2 && debug_int("IDQN_DGRAD_RT", 0) <= 4) rt = debug_int("IDQN_DGRAD_RT", 0);
        }
        const unsigned grid = (unsigned)(K * (nb / 8) * cdiv(h->F, 64 * rt));
        // (mask, planes and per-position sums in the GEMM's epilogue instead of the finalize launch: bit-identical, 110.3 us against
        // 84.3 + 25.6 -- the epilogue's plane stores are 8-byte pieces a row apart)
        {
            static LdsAttrMark attr;
            if (attr.needs(lds)) {
                IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_dgrad<2, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_dgrad<2, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_dgrad<2, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
            if (rt == 4) hipLaunchKernelGGL((k_iqn_d0_dgrad<2, 4>), dim3(grid), dim3(512), lds, q, g);
            else if (rt == 3) hipLaunchKernelGGL((k_iqn_d0_dgrad<2, 3>), dim3(grid), dim3(512), lds, q, g);
            else hipLaunchKernelGGL((k_iqn_d0_dgrad<2, 2>), dim3(grid), dim3(512), lds, q, g);
            tl_mark(h, q, "dense0 dgrad (tiled GEMM)");
            Da3FinalizeArgs fa;
            fa.dpart = h->dpart; fa.a3 = s.a3; fa.da3 = h->da3; fa.da3p = h->da3p; fa.pb = h->pbuf[2];
            fa.n_rows = (long)K * nb * h->F; fa.n_jt = 1; fa.F = h->F; fa.C = c2->CO; fa.K = K; fa.nb = nb; fa.g = h->gda3;
            hipLaunchKernelGGL(k_da3_finalize, dim3(cdiv(fa.n_rows * 8, 256)), dim3(256), 0, q, fa);
            tl_mark(h, q, "da3 finalize (sum, mask, planes)");
        }
    } else
    if (!fuse_dg) {
        DenseDgradArgs dd;
        dd.dh = dh_of(h, nb); dd.a3 = s.a3; dd.da3 = h->da3; dd.da3p = h->da3p; dd.pb = h->pbuf[2]; dd.wbase = s.wbase; dd.w_off = h->off_w0;
        dd.K = K; dd.nb = nb; dd.n_ft = h->F / 32; dd.F = h->F; dd.J = h->J; dd.C = c2->CO; dd.g = h->gda3; dd.raw = nullptr;
        // 4 or 3 f tiles per workgroup, whichever leaves the busiest CU fewer tiles (two workgroups fit a CU's LDS)
        const long wg4 = (long)K * nb * cdiv(dd.n_ft, 4), wg3 = (long)K * nb * cdiv(dd.n_ft, 3);
        const long busy4 = cdiv(wg4, 256) * 4, busy3 = wg3 <= 512 ? cdiv(wg3, 256) * 3 : 1 << 30;
        if (busy3 < busy4) {
            dd.n_items = wg3;
            hipLaunchKernelGGL((k_dense0_dgrad<3>), dim3((unsigned)dd.n_items), dim3(192), h->J * 32 * 4, q, dd);
        } else {
            dd.n_items = wg4;
            hipLaunchKernelGGL((k_dense0_dgrad<4>), dim3((unsigned)dd.n_items), dim3(256), h->J * 32 * 4, q, dd);
        }
        tl_mark(h, q, "dense0 dgrad");
    }
    if (stop_before_dense0_wgrad) {
        h->pend_B = B; h->pend_stage = 1; h->pend_profile = profile;
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    // Dense_0 weight gradient (+ Adam): the dominant, HBM-bound kernel
    int rcw = launch_dense0_wgrad(h, s.a3, dh_of(h, nb), nb, nb, 0, (long)nb * h->F * 32, (long)h->F * 32, 0,
                                  (long)nb * h->J * 32, (long)h->J * 32, fuse_adam, profile, q, fuse_dg);
    if (rcw) return rcw;
    if (fuse_dg && !h->d0_rows) {
        Da3FinalizeArgs fa;
        fa.dpart = h->dpart; fa.a3 = s.a3; fa.da3 = h->da3; fa.da3p = h->da3p; fa.pb = h->pbuf[2];
        fa.n_rows = (long)K * nb * h->F; fa.n_jt = h->J / 256; fa.F = h->F; fa.C = c2->CO; fa.K = K; fa.nb = nb; fa.g = h->gda3;
        hipLaunchKernelGGL(k_da3_finalize, dim3(cdiv(fa.n_rows * 8, 256)), dim3(256), 0, q, fa);
        tl_mark(h, q, "da3 finalize (sum, mask, planes)");
    }
    if (stop_after_dense0) {
        h->pend_B = B; h->pend_stage = 2;
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    return cnn_backward_rest(h, B, fuse_adam, q);
}

// the slab descriptor of conv layer i (position chunks = what its weight-gradient launch of THIS step wrote)
void fill_seg(idqn_handle_s* h, int i, SlabSeg& g, long first_block) {
    const ConvL& l = h->conv[i];
    g.slab = h->slab + h->slab_off[i]; g.slab_stride = h->slab_stride[i]; g.w_off = l.w_off; g.b_off = l.b_off;
    g.wsize = (long)l.K * l.K * l.CI * l.CO; g.npc = h->planes ? h->npc_used[i] : h->npc[i]; g.bsize = l.CO;
    g.first_block = first_block;
}

void fill_adam_args(idqn_handle_s* h, long begin, long end, long skip_b, long skip_e, bool from_slabs, bool epilogue, AdamArgs& a) {
    a.ep_count = epilogue ? h->count : nullptr; a.ep_losses = h->losses; a.ep_cum = h->cum;
    a.theta = h->online; a.mu = h->mu; a.nu = h->nu; a.grad = h->grad; a.bcinv = h->bcinv; a.ad = h->ad;
    a.P = h->L.head_stride; a.begin = begin; a.end = end; a.skip_begin = skip_b; a.skip_end = skip_e;
    a.K = h->cfg.n_heads; a.n_seg = from_slabs ? 3 : 0;
    a.gP = h->gP; a.w0_begin = h->g_w0_begin; a.w0_end = h->g_w0_end; a.g_w0_base = h->g_w0_base;
    for (int i = 0; i < 3; ++i) a.seg[i] = h->segs[i];
    if (skip_b == skip_e) a.skip_begin = a.skip_end = end;  // nothing skipped
}

int cnn_backward_rest(idqn_handle_s* h, int B, bool fuse_adam, hipStream_t q) {
    const int K = h->cfg.n_heads, nb = cdiv(B, 32);
    NetSet& s = h->train;
    const ConvL* cl[3] = {&h->conv[0], &h->conv[1], &h->conv[2]};
    SlabReduceArgs r;
    r.grad = h->grad; r.gP = h->gP; r.K = K; r.n_seg = 3;
    long nblk = 0;
    if (h->planes) {
        // data gradients (stride-1 convolutions over the zero-bordered dout planes), then the weight gradients
        // per layer, top down: its data gradient and its weight gradient read the same dy and are independent of each other --
        // one launch for both where that pair of kernels is built (planes_pair), else one after the other
        static const char* nd[3] = {"", "conv1 dgrad", "conv2 dgrad"};
        static const char* nw[3] = {"conv0 wgrad", "conv1 wgrad", "conv2 wgrad"};
        static const char* np[3] = {"", "conv1 dgrad + wgrad", "conv2 dgrad + wgrad"};
        int rc = IDQN_OK;
        for (int i = 2; i >= 0 && !rc; --i) {
            bool paired = false;
            if (i >= 1) rc = planes_pair(h, i, nb, q, &paired);
            if (paired) { tl_mark(h, q, np[i]); continue; }
            if (i >= 1 && !rc) { rc = planes_conv(h, s, i == 2 ? 3 : 4, nb, q); tl_mark(h, q, nd[i]); }
            if (!rc) {
                rc = planes_wgrad(h, i, nb, q);
                tl_mark(h, q, nw[i]);
            }
        }
        if (rc) return rc;
    } else {
        // data gradients as forward convolutions over the zero-bordered dout buffers with transformed weights
        int rcb = build_dgrad_weights(h, q);
        if (rcb) return rcb;
        for (int i = 2; i >= 1; --i) {
            const ConvL& l = *cl[i];
            ConvFwdArgs a;
            int rcd = make_dgrad_args(h, i, nb, a);
            if (rcd) return rcd;
            if (l.CI == 32)
                hipLaunchKernelGGL((k_conv_fwd<1, 1>), dim3((unsigned)a.n_items), dim3(256), 0, q, a);
            else
                hipLaunchKernelGGL((k_conv_fwd<2, 1>), dim3((unsigned)a.n_items), dim3(256), 0, q, a);
        }
    }
    // conv weight gradients: slabs (one region per layer), then ONE reduce launch into the gradient arena
    for (int i = 2; i >= 0; --i) {
        const ConvL& l = *cl[i];
        if (!h->planes) {
            ConvWgradArgs a = make_wgrad_args(h, i, nb);
            const int nit = a.CIe / 32, not_ = a.CO / 32;
            dim3 grid((unsigned)a.n_items);
            if (nit == 1 && not_ == 1) hipLaunchKernelGGL((k_conv_wgrad<1, 1>), grid, dim3(256), 0, q, a);
            else if (nit == 1 && not_ == 2) hipLaunchKernelGGL((k_conv_wgrad<1, 2>), grid, dim3(256), 0, q, a);
            else if (nit == 2 && not_ == 1) hipLaunchKernelGGL((k_conv_wgrad<2, 1>), grid, dim3(256), 0, q, a);
            else hipLaunchKernelGGL((k_conv_wgrad<2, 2>), grid, dim3(256), 0, q, a);
        }
        SlabSeg& g = r.seg[2 - i];
        fill_seg(h, i, g, nblk);
        (void)l;
        nblk += cdiv(g.wsize + g.bsize, 256);
    }
    for (int i = 0; i < 3; ++i) h->segs[i] = r.seg[i];
    if (!fuse_adam)  // two-phase step: the gradient arena must be complete (it gets all-reduced); the fused
        hipLaunchKernelGGL(k_slab_reduce, dim3((unsigned)nblk, K), dim3(256), 0, q, r);  // path sums in k_adam
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

int step_epilogue(idqn_handle_s* h, bool bump, hipStream_t q) {
    hipLaunchKernelGGL(k_step_epilogue, dim3(cdiv(h->cfg.n_heads, 64)), dim3(64), 0, q, h->count, h->losses, h->cum,
                       h->cfg.n_heads, bump ? 1 : 0);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
// impala handles (impala_kernels.h) are served by idqn_learn_on_batch, idqn_learn_on_replay_fc(_dev), idqn_q_values /
// idqn_best_action, idqn_act_host(_begin / _end), the target operations, idqn_apply_adam, idqn_set_per_buffers and the debug /
// profile reads.  Every other entry refuses them here, before anything is enqueued; the Python callers take their fallbacks.
#define IDQN_REFUSE_IMPALA(h, fn)                                                                                      \
    IDQN_REQUIRE(!((h) && (h)->cfg.arch == IDQN_ARCH_IMPALA),                                                           \
                 "%s: the impala architecture is not served by this entry (single calls of idqn_learn_on_batch / idqn_act_host are)", fn)

extern "C" int idqn_layout(const idqn_config_t* cfg, int32_t* n_leaves, idqn_leaf_t* leaves, int64_t* head_stride) {
    IDQN_REQUIRE(cfg && n_leaves && leaves && head_stride, "idqn_layout: null pointer");
    Layout L;
    int rc = build_layout(*cfg, L);
    if (rc) return rc;
    *n_leaves = L.n_leaves;
    memcpy(leaves, L.leaves, sizeof(idqn_leaf_t) * L.n_leaves);
    *head_stride = L.head_stride;
    return IDQN_OK;
}

extern "C" int idqn_create(const idqn_config_t* cfg, float* online_dev, float* target_dev, float* mu_dev, float* nu_dev,
                           float* grad_dev, int32_t* count_dev, float* losses_dev, double* cum_losses_dev,
                           idqn_handle_t* out) {
    IDQN_REQUIRE(cfg && out, "idqn_create: null pointer");
    IDQN_REQUIRE(online_dev && target_dev && mu_dev && nu_dev && grad_dev && count_dev && losses_dev && cum_losses_dev,
                 "idqn_create: every arena pointer is required");
    IDQN_REQUIRE(online_dev != target_dev, "idqn_create: online and target must be distinct buffers (the reference's "
                                           "aliasing at idqn.py:56 is only safe for immutable arrays)");
    int ndev = 0;
    IDQN_HIP_CHECK(hipGetDeviceCount(&ndev));
    IDQN_REQUIRE(ndev > 0, "idqn_create: no HIP device");
    // impala conv arithmetic: the vector-ALU kernels (the default), or the matrix-core kernel where a layer is eligible
    const char* imp_mode = getenv("IDQN_IMP_CONV");
    IDQN_REQUIRE(cfg->arch != IDQN_ARCH_IMPALA || imx_mode_of(imp_mode) != IMX_MODE_BAD, "IDQN_IMP_CONV must be valu or bf16x3, got '%s'", imp_mode);
    const char* imp_wmode = getenv("IDQN_IMP_WGRAD");  // the same for their weight gradients, independently
    IDQN_REQUIRE(cfg->arch != IDQN_ARCH_IMPALA || imx_mode_of(imp_wmode) != IMX_MODE_BAD, "IDQN_IMP_WGRAD must be valu or bf16x3, got '%s'", imp_wmode);
    const char* imp_d0mode = getenv("IDQN_IMP_D0");  // the head's Dense_0 forward: k_imp_d0_fwd, or the f32 matrix-core kernel
    IDQN_REQUIRE(cfg->arch != IDQN_ARCH_IMPALA || impd0_mode_of(imp_d0mode) != IMPD0_MODE_BAD, "IDQN_IMP_D0 must be valu or mfma, got '%s'", imp_d0mode);
    idqn_handle_s* h = new idqn_handle_s();
    h->cfg = *cfg;
    h->imp.d0mx = cfg->arch == IDQN_ARCH_IMPALA && impd0_mode_of(imp_d0mode) == IMPD0_MODE_MFMA;
    h->imp.mx = cfg->arch == IDQN_ARCH_IMPALA && imx_mode_of(imp_mode) == IMX_MODE_BF16X3;
    h->imp.wmx = cfg->arch == IDQN_ARCH_IMPALA && imx_mode_of(imp_wmode) == IMX_MODE_BF16X3;
    int rc = build_layout(*cfg, h->L);
    if (rc) { delete h; return rc; }
    h->online = online_dev; h->target = target_dev; h->mu = mu_dev; h->nu = nu_dev; h->grad = grad_dev;
    h->count = count_dev; h->losses = losses_dev; h->cum = cum_losses_dev;
    h->ad.lr_neg = (float)(-cfg->learning_rate);
    h->ad.b1 = (float)cfg->adam_b1; h->ad.b2 = (float)cfg->adam_b2;
    h->ad.omb1 = (float)(1.0 - cfg->adam_b1); h->ad.omb2 = (float)(1.0 - cfg->adam_b2);
    h->ad.eps = (float)cfg->adam_eps;
    h->gamma_n = (float)cfg->gamma_n;
    h->nb_max = cdiv(cfg->max_batch, 32);
    h->gP = h->L.head_stride;
    if (cfg->arch == IDQN_ARCH_CNN) {
        h->g_w0_begin = h->L.leaves[6].offset; h->g_w0_end = h->L.leaves[7].offset;  // Dense_0/kernel .. Dense_0/bias
        h->gP = h->L.head_stride - (h->g_w0_end - h->g_w0_begin);
    }
    h->g_w0_base = (long)cfg->n_heads * h->gP + 64;
    {  // conv arithmetic: f32-accurate products on the bf16 matrix cores (convp.h, the default), or the f32 MFMA kernels
        const char* mode = getenv("IDQN_CONV");
        h->planes = cfg->arch == IDQN_ARCH_CNN && !(mode && strcmp(mode, "f32") == 0);
        IDQN_REQUIRE(!mode || !strcmp(mode, "f32") || !strcmp(mode, "bf16x3"), "IDQN_CONV must be f32 or bf16x3, got '%s'", mode);
    }
    rc = alloc_zero(&h->bcinv, 2L * cfg->n_heads + 64, h, "bcinv");
    const bool general = cfg->arch == IDQN_ARCH_CNN && !cnn_fast_shape(*cfg);
    if (general) h->planes = false;
    if (!rc) rc = general ? gcnn_setup(h) : (cfg->arch == IDQN_ARCH_CNN ? cnn_setup(h) : cfg->arch == IDQN_ARCH_IMPALA ? impala_setup(h) : fc_setup(h));
    if (rc) { idqn_destroy(h); return rc; }
    h->ev.resize(2 * 2048);
    for (auto& e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) { idqn_set_error("hipEventCreate failed"); idqn_destroy(h); return IDQN_E_HIP; }
    IDQN_HIP_CHECK(hipDeviceSynchronize());
    *out = h;
    return IDQN_OK;
}

extern "C" int idqn_destroy(idqn_handle_t h) {
    if (!h) return IDQN_OK;
    (void)hipDeviceSynchronize();
    for (void* p : h->owned) (void)hipFree(p);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : h->tl_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& g : h->act_graphs) (void)hipGraphExecDestroy(g.second);
    for (auto& g : h->iact_graphs) (void)hipGraphExecDestroy(g.second);
    for (auto& g : h->step_graphs)
        if (g.second.second) (void)hipGraphExecDestroy(g.second.second);
    if (h->act_stream) (void)hipStreamDestroy(h->act_stream);
    if (h->act_mail) (void)hipHostFree(h->act_mail);
    h->many.release();
    h->steps.release();
    if (h->fact_planes) (void)hipFree(h->fact_planes);
    for (int32_t* p : h->iqn.bwd_items)
        if (p) (void)hipFree(p);
    delete h;
    return IDQN_OK;
}

// What issue(stream) enqueues, captured on a stream of the handle's own (the caller's may be the legacy default stream, which
// cannot capture) and instantiated; the graph is then launched on the caller's stream like any other work.  Nothing of a failed
// capture is kept: hipStreamEndCapture is always called, the hipGraph_t is destroyed on every path, and *exec is written only
// once instantiation has succeeded.
template <class Issue>
static int capture_exec(idqn_handle_t h, Issue&& issue, hipGraphExec_t* exec) {
    if (!h->act_stream) IDQN_HIP_CHECK(hipStreamCreateWithFlags(&h->act_stream, hipStreamNonBlocking));
    IDQN_HIP_CHECK(hipStreamBeginCapture(h->act_stream, hipStreamCaptureModeRelaxed));
    hipGraph_t graph = nullptr;
    hipGraphExec_t ex = nullptr;
    const int rc = issue(h->act_stream);
    const hipError_t e = hipStreamEndCapture(h->act_stream, &graph);
    const hipError_t ei = rc == IDQN_OK && e == hipSuccess ? hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0) : hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    IDQN_HIP_CHECK(e);
    IDQN_HIP_CHECK(ei);
    *exec = ex;
    return IDQN_OK;
}

// The step of the MFMA cnn path (plane conv by default): forward, backward with the fused Dense_0 update, Adam on every other leaf
static int cnn_learn(idqn_handle_t h, const StepIn& in, hipStream_t q) {
    auto issue = [&](hipStream_t qs) -> int {
        int r;
        if ((r = cnn_forward(h, h->train, (const uint8_t*)in.state, (const uint8_t*)in.next_state, in.batch, qs, true, in.frames ? &in : nullptr)))
            return r;
        if ((r = cnn_backward(h, in, qs))) return r;
        if (!in.grads_only()) {
            // every leaf except Dense_0/kernel (already updated by the fused weight-gradient kernel)
            const long w0_b = h->off_w0, w0_e = h->off_b0;
            if ((r = launch_adam(h, 0, h->L.head_stride, w0_b, w0_e, true, qs))) return r;
        }
        return IDQN_OK;  // count += 1 and cum_losses += losses already happened in k_td_dh
    };
    // A whole plain step is 13 launches whose arguments are pointers and sizes only: for a given set of batch buffers it
    // can be replayed as ONE hipGraph (opt-in).  The first call of a key runs eagerly (it builds the launch plans, which
    // allocate), the second is captured on the handle's private stream, every call from then on is one graph launch.
    static const bool step_graph = getenv("IDQN_STEP_GRAPH") && atoi(getenv("IDQN_STEP_GRAPH")) != 0;
    if (step_graph && in.flags == 0 && !in.frames) {  // (a replay-sourced step carries its slots as kernel arguments: not replayable)
        auto key = std::make_tuple(in.state, in.next_state, (const void*)in.action, (const void*)in.reward, (const void*)in.terminal,
                                   in.batch, in.mean_divisor, (const void*)in.is_weight, (const void*)in.td_abs);
        // bounded: a caller that hands over allocator-recycled buffers would otherwise instantiate a graph per pointer
        // tuple that ever recurs; past 32 keys everything is dropped and the cache starts again
        if (h->step_graphs.size() >= 32 && !h->step_graphs.count(key)) {
            // the last replay may still be running on the caller's stream: an executable graph is only destroyed idle
            IDQN_HIP_CHECK(hipStreamSynchronize(q));
            for (auto& g : h->step_graphs)
                if (g.second.second) (void)hipGraphExecDestroy(g.second.second);
            h->step_graphs.clear();
        }
        auto& ent = h->step_graphs[key];
        if (ent.first++ == 0) return issue(q);
        if (!ent.second) {
            if (const int rc = capture_exec(h, issue, &ent.second)) {  // nothing of a failed capture is kept
                h->step_graphs.erase(key);
                return rc;
            }
        }
        IDQN_HIP_CHECK(hipGraphLaunch(ent.second, q));
        return IDQN_OK;
    }
    return issue(q);
}

// The MLP step: ONE launch of the first kernel of the ladder that serves the net and the batch (+ Adam where the kernel has
// none of its own).  h->dominant names that kernel, template variant included (idqn_profile_read reports it).
static int fc_learn(idqn_handle_t h, const StepIn& in, hipStream_t q) {
    const bool grads_only = in.grads_only(), profile = in.profile();
    FcArgs a = fc_args(h, in.batch, in.mean_divisor, grads_only);
    a.s = (const float*)in.state; a.s2 = (const float*)in.next_state; a.action = in.action; a.reward = in.reward;
    a.terminal = in.terminal;
    a.is_weight = in.is_weight; a.td_abs = in.td_abs;
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used], q));
    const FcPlan& fp = h->fc_plan_;
    const size_t lds = (size_t)fp.floats * 4;
    const FcMfmaPlan& fm = h->fcm_plan_;
    const bool par = h->fcp_plan_.floats && in.batch <= 32;  // one launch: forwards side by side, Adam in the gradient epilogues
    if (par && in.frames) {  // the minibatch comes from the replay frame ring (learn_on_replay_fc): the same single launch
        h->dominant = "k_fc_step_par<ring>";
        if (in.slots_dev)
            fc_step_par_launch(h, q, a, grads_only, fc_ring_src(in.frames, in.rows, in.n_frames, in.frame_bytes, in.stack, RpsSlotsDev{in.slots_dev}));
        else
            fc_step_par_launch(h, q, a, grads_only, fc_ring_src(in.frames, in.rows, in.n_frames, in.frame_bytes, in.stack, in.slot_block<RpsSlotsPar>()));
    } else if (par) {
        h->dominant = "k_fc_step_par";
        fc_step_par_launch(h, q, a, grads_only, FcBatchSrc{});
    } else if (fm.floats && h->fcm_global_) {
        h->dominant = "k_fc_step_mfma<global>";
        hipLaunchKernelGGL(k_fc_step_mfma<true>, dim3(h->cfg.n_heads), dim3(FCM_T), (size_t)fm.floats * 4, q, a, fm.ldw, fm.drows, fm.w_floats);
    } else if (fm.floats) {
        h->dominant = "k_fc_step_mfma<lds>";
        hipLaunchKernelGGL(k_fc_step_mfma<false>, dim3(h->cfg.n_heads), dim3(FCM_T), (size_t)fm.floats * 4, q, a, fm.ldw, fm.drows, fm.w_floats);
    } else if (fp.BS == 32) {
        h->dominant = "k_fc_step_lds<32>";
        hipLaunchKernelGGL(k_fc_step_lds<32>, dim3(h->cfg.n_heads), dim3(FC_T), lds, q, a, fp.tw, fp.wfl);
    } else if (fp.BS == 16) {
        h->dominant = "k_fc_step_lds<16>";
        hipLaunchKernelGGL(k_fc_step_lds<16>, dim3(h->cfg.n_heads), dim3(FC_T), lds, q, a, fp.tw, fp.wfl);
    } else if (fp.BS == 8) {
        h->dominant = "k_fc_step_lds<8>";
        hipLaunchKernelGGL(k_fc_step_lds<8>, dim3(h->cfg.n_heads), dim3(FC_T), lds, q, a, fp.tw, fp.wfl);
    } else {
        h->dominant = "k_fc_step";
        hipLaunchKernelGGL(k_fc_step, dim3(h->cfg.n_heads), dim3(256), 0, q, a);
    }
    if (profile && h->ev_used + 2 <= (int)h->ev.size()) {
        IDQN_HIP_CHECK(hipEventRecord(h->ev[h->ev_used + 1], q));
        h->ev_used += 2;
    }
    tl_mark(h, q, h->dominant);
    IDQN_HIP_CHECK(hipGetLastError());
    if (!grads_only && !par) return launch_adam(h, 0, h->L.head_stride, 0, 0, false, q);
    return IDQN_OK;  // count += 1 and cum_losses += losses already happened in the step kernel (fused path)
}

// ---- i-IQN heads (extension; iqn_kernels.h, oracle/iqn_ref.py) --------------------------------------------------------
namespace {
// fraction blocks -> Dense_0 -> hidden + Dense_1 partials, for `V` virtual nets whose trunk features are psi [.][nb][F * 32]:
// NB = N x ceil(B / 32) blocks per virtual net, block s N + q = fraction q of sample block s
int iqn_heads_forward(idqn_handle_s* h, const float* const* wbase_v, int V, int K_for_index, const float* psi, const float* tau,
                      int B, hipStream_t q) {
    IqnWs& w = h->iqn;
    const int nb = cdiv(B, 32), NB = w.N * nb;
    IqnCosArgs ca;
    // the embedding on the bf16 matrix cores from operands split once per step
    ca.tau = tau; ca.cosp = w.cosp; ca.cosa = w.cosa; ca.K = K_for_index; ca.N = w.N; ca.B = B; ca.NB = NB;
    hipLaunchKernelGGL(k_iqn_cos, dim3((unsigned)(V * NB)), dim3(256), 0, q, ca);
    tl_mark(h, q, "iqn cos features");
    {   // fractions per wave: 8 when that still leaves >= 8 waves per SIMD to overlap, else fewer 
        int per = 8;
        while (per > 1 && (w.N % per != 0)) --per;
        const dim3 grid((unsigned)cdiv(h->F / 32, 4), (unsigned)V, (unsigned)(NB / per));  // (per divides N: a group stays in its sample block)
        {
            const int n_packed = std::min(V, 2 * K_for_index);  // virtual nets 2K .. 3K - 1 are the target nets again
            IqnWePackArgs pa;
            pa.wbase = wbase_v; pa.wep = w.wep; pa.we_off = w.off_we; pa.F = h->F;
            hipLaunchKernelGGL(k_iqn_we_pack, dim3((unsigned)(h->F / 32), (unsigned)n_packed), dim3(256), 0, q, pa);
            tl_mark(h, q, "iqn embedding kernel planes");
            IqnEmbed3Args e3;
            e3.cosp = w.cosp; e3.wep = w.wep; e3.wbase = wbase_v; e3.psi = psi; e3.x = w.xq; e3.be_off = w.off_be;
            e3.K = K_for_index; e3.N = w.N; e3.F = h->F; e3.n_packed = n_packed; e3.nb = nb;
            // cos fragments through LDS, once per workgroup
            hipLaunchKernelGGL(k_iqn_embed3l, grid, dim3(256), 2 * 12288, q, e3);
        }
    }
    tl_mark(h, q, "iqn embedding x features");
    DenseFwdArgs d;
    d.in = w.xq; d.part = w.part; d.wbase = wbase_v; d.w_off = h->off_w0;
    d.n_nets = V; d.nb = NB; d.NS = w.NS; d.n_jt = h->J / 128; d.F = h->F; d.J = h->J;
    d.n_items = (long)V * NB * d.NS * d.n_jt;
    d.net_rot = 0; d.bb_inner = 0; d.nt_from = 0;
    // >= 8 blocks per net: the tiled GEMM (iqn_gemm.h; fewer, or a count that is no multiple of 8: the per-block streaming kernel of the plain step)
    if (NB % 8 == 0 && h->J % 256 == 0 && h->F % 16 == 0) {
        IqnD0FwdArgs g;
        g.x = w.xq; g.wbase = wbase_v; g.part = w.part; g.w_off = h->off_w0;
        g.V = V; g.nb = NB; g.NS = w.NS; g.F = h->F; g.J = h->J; g.clk = (long long*)w.clk;
        const size_t lds = 2 * (size_t)IG_STAGE;
        const dim3 grid((unsigned)(V * (NB / 8) * w.NS * (h->J / 256)));
        static LdsAttrMark attr;
        if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_fwd<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_iqn_d0_fwd<2>, grid, dim3(512), lds, q, g);
    } else {
        hipLaunchKernelGGL(k_dense0_fwd3, dim3(cdiv(d.n_items, 4)), dim3(256), 0, q, d);
    }
    tl_mark(h, q, "iqn dense0 fwd");
    HiddenArgs hi;
    hi.part = w.part; hi.wbase = wbase_v; hi.b0_off = h->off_b0; hi.w1_off = h->off_w1; hi.nb = NB; hi.NS = w.NS;
    hi.J = h->J; hi.A = h->cfg.n_actions; hi.hbuf = w.hbuf; hi.qpart = w.qpart;
    hipLaunchKernelGGL(k_hidden, dim3(h->J / 32, (unsigned)(V * NB)), dim3(256), 0, q, hi);
    tl_mark(h, q, "iqn hidden");
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}
}  // namespace

static int iqn_learn(idqn_handle_t h, const StepIn& in, hipStream_t q);  // (below, with its public entry)

// ONE gradient step on handle h: what every step does once, then the step of the handle's path (a quantile step, in.tau set,
// is iqn_learn on its cnn handle).  Every learner entry ends here, its arguments checked under its own name.
static int learn_step(idqn_handle_t h, const StepIn& in, hipStream_t q) {
    h->pend_B = 0; h->pend_stage = 0;
    int rc;
    if ((rc = tl_begin(h, in.flags, q))) return rc;
    if (in.tau) return iqn_learn(h, in, q);
    if (h->imp.on) {
        rc = impala_learn(h, in, q);
    } else if (h->gc.on) {
        IDQN_REQUIRE(!(in.stop0() || in.stopb()), "the IDQN_F_STOP_* flags belong to the MFMA cnn path");
        rc = gcnn_learn(h, in, q);
    } else {
        return h->cfg.arch == IDQN_ARCH_CNN ? cnn_learn(h, in, q) : fc_learn(h, in, q);
    }
    if (rc || in.grads_only()) return rc;
    return launch_adam(h, 0, h->L.head_stride, 0, 0, false, q);
}

// The five device tensors of a batch entry, and the prioritized-replay buffers the caller set on the handle
static StepIn batch_step(idqn_handle_t h, const char* fn, const void* state_dev, const void* next_state_dev, const int32_t* action_dev,
                         const float* reward_dev, const uint8_t* terminal_dev, int32_t batch, int32_t mean_divisor, uint32_t flags) {
    StepIn in;
    in.fn = fn; in.batch = batch; in.mean_divisor = mean_divisor; in.flags = flags;
    in.state = state_dev; in.next_state = next_state_dev; in.action = action_dev; in.reward = reward_dev; in.terminal = terminal_dev;
    in.is_weight = h->is_weight; in.td_abs = h->td_abs;
    return in;
}

extern "C" int idqn_learn_on_batch(idqn_handle_t h, const void* state_dev, const void* next_state_dev,
                                   const int32_t* action_dev, const float* reward_dev, const uint8_t* terminal_dev,
                                   int32_t batch, int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(h && state_dev && next_state_dev && action_dev && reward_dev && terminal_dev, "idqn_learn_on_batch: null pointer");
    IDQN_REQUIRE(batch >= 1 && batch <= h->cfg.max_batch, "idqn_learn_on_batch: batch %d not in [1, %d]", batch, h->cfg.max_batch);
    IDQN_REQUIRE(batch_mean_divisor >= batch, "idqn_learn_on_batch: mean divisor %d < batch %d", batch_mean_divisor, batch);
    IDQN_REQUIRE(!(flags & (IDQN_F_STOP_AFTER_DENSE0 | IDQN_F_STOP_BEFORE_DENSE0_WGRAD)) || h->cfg.arch == IDQN_ARCH_CNN,
                 "the IDQN_F_STOP_* flags belong to the cnn path");
    return learn_step(h, batch_step(h, "idqn_learn_on_batch", state_dev, next_state_dev, action_dev, reward_dev, terminal_dev, batch,
                                    batch_mean_divisor, flags), (hipStream_t)stream);
}

// Everything learn_on_replay (below) refuses on its own account, before anything is enqueued or allocated (shared with
// idqn_per_learn_on_replay).
static int replay_check(idqn_handle_t h, const char* fn, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                        const int32_t* rows_dev, const int32_t* slots_host, const int32_t* slots_dev, int32_t batch, int32_t stack,
                        const float* tau_dev, uint32_t flags) {
    IDQN_REQUIRE(h && frame_ring_dev && rows_dev && (slots_host || slots_dev), "%s: null pointer", fn);
    IDQN_REFUSE_IMPALA(h, fn);
    if (tau_dev) {  // the quantile step (idqn_iqn_learn_on_replay*): the limits of idqn_iqn_learn_on_batch, under the caller's name
        IDQN_REQUIRE(h->iqn.N > 0, "%s: the handle was created without quantile heads (cfg.n_quantiles)", fn);
        IDQN_REQUIRE(!(flags & ~(IDQN_F_PROFILE | IDQN_F_PROFILE_ALL)), "%s: only the profile flags are supported", fn);
    }
    IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_CNN && h->planes && !h->gc.on, "%s: needs the cnn arch on the plane conv path", fn);
    IDQN_REQUIRE(batch >= 1 && batch <= 256 && batch <= h->cfg.max_batch, "%s: batch %d not in [1, min(256, %d)]", fn, batch,
                 h->cfg.max_batch);
    IDQN_REQUIRE(stack == 4 && h->cfg.obs_c == 4 && frame_bytes == (int64_t)h->cfg.obs_h * h->cfg.obs_w && frame_bytes % 16 == 0 &&
                     n_frames >= 1 && ((uintptr_t)frame_ring_dev & 15) == 0,
                 "%s: built for uint8 frames of obs_h x obs_w bytes (a multiple of 16), stack 4 == obs_c (got stack %d, "
                 "frame_bytes %ld, obs %d x %d x %d)", fn, stack, (long)frame_bytes, h->cfg.obs_h, h->cfg.obs_w, h->cfg.obs_c);
    return IDQN_OK;
}

// h->rp_action / rp_reward / rp_terminal, the scalars of the sampled rows, on a handle's first replay-sourced call (behind that
// call's refusals).  One set per handle whichever of the two callers comes first; learn_on_replay_fc's first call waits for the
// null stream once here and once more behind its own state buffers (a first call only).
static int ensure_replay_scalars(idqn_handle_t h) {
    if (h->rp_action) return IDQN_OK;
    const long mb = h->cfg.max_batch;
    float* f = nullptr;
    if (const int rc = alloc_zero(&f, 3L * mb + 64, h, "replay scalars")) return rc;
    IDQN_HIP_CHECK(hipStreamSynchronize(nullptr));  // (the zero-fill runs on the null stream)
    h->rp_action = (int32_t*)f; h->rp_reward = f + mb; h->rp_terminal = (uint8_t*)(f + 2L * mb);
    return IDQN_OK;
}

// iDQN.update_online_params (idqn.py:65-72) on the HBM frame ring: replay_buffer.py:215-230's sample() fused into the step.
// `in` names the ring (ring_step); exactly one of its slots_host / slots_dev is set.
//
// The ring is read by ONE launch (StepIn): the staging launch of cnn_forward (planes_stage), which writes the bf16 pixel planes
// and the sampled rows' scalars into buffers the handle owns; the TD kernel and everything later read those.  (The stream order
// still matters to the CALLER: the ring must not be overwritten before the staging launch has run.)
static int learn_on_replay(idqn_handle_t h, StepIn in, void* stream) {
    if (const int rc = replay_check(h, in.fn, (const uint8_t*)in.frames, in.n_frames, in.frame_bytes, in.rows, in.slots_host, in.slots_dev, in.batch,
                                    in.stack, in.tau, in.flags))
        return rc;
    if (const int rc = ensure_replay_scalars(h)) return rc;
    // (reported under the batch entry's name, and behind the first call's allocation, since the step first ran through that entry)
    IDQN_REQUIRE(in.tau || in.mean_divisor >= in.batch, "idqn_learn_on_batch: mean divisor %d < batch %d", in.mean_divisor, in.batch);
    // (the state pointers are what the staging launch is told beside the ring; it gathers from the ring)
    in.state = in.next_state = in.frames;
    in.action = h->rp_action; in.reward = h->rp_reward; in.terminal = h->rp_terminal;
    return learn_step(h, in, (hipStream_t)stream);
}

// The frame ring of a replay entry as a step's input.  `per`: the handle of a public entry, whose prioritized-replay buffers
// (idqn_set_per_buffers) the step takes; nullptr where the caller names the step's weights / |TD| itself, or has refused them
static StepIn ring_step(idqn_handle_t per, const char* fn, const void* frame_ring_dev, int64_t n_frames, int64_t frame_bytes, const int32_t* rows_dev,
                        const int32_t* slots_host, const int32_t* slots_dev, int32_t batch, int32_t stack, int32_t mean_divisor, uint32_t flags) {
    StepIn in;
    in.fn = fn; in.batch = batch; in.mean_divisor = mean_divisor; in.flags = flags;
    in.frames = frame_ring_dev; in.rows = rows_dev; in.n_frames = n_frames; in.frame_bytes = frame_bytes; in.stack = stack;
    in.slots_host = slots_dev ? nullptr : slots_host; in.slots_dev = slots_dev;
    if (per) { in.is_weight = per->is_weight; in.td_abs = per->td_abs; }
    return in;
}

extern "C" int idqn_learn_on_replay(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                    const int32_t* rows_dev, const int32_t* slots_host, int32_t batch, int32_t stack,
                                    int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_host, "idqn_learn_on_replay: null pointer");
    return learn_on_replay(h, ring_step(h, "idqn_learn_on_replay", frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host, nullptr, batch, stack,
                                        batch_mean_divisor, flags), stream);
}

extern "C" int idqn_learn_on_replay_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                        const int32_t* rows_dev, const int32_t* slots_dev, int32_t batch, int32_t stack,
                                        int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_dev, "idqn_learn_on_replay_dev: null pointer");
    return learn_on_replay(h, ring_step(h, "idqn_learn_on_replay_dev", frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, slots_dev, batch,
                                        stack, batch_mean_divisor, flags), stream);
}

// Everything learn_on_replay_fc refuses, before anything is enqueued or allocated (shared with idqn_learn_steps_on_replay_fc).
static int replay_fc_check(idqn_handle_t h, const char* fn, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                           const int32_t* rows_dev, const int32_t* slots_host, const int32_t* slots_dev, int32_t batch, int32_t stack,
                           int32_t batch_mean_divisor, uint32_t flags, long* obs_elems_out) {
    IDQN_REQUIRE(h && frame_ring_dev && rows_dev && (slots_host || slots_dev), "%s: null pointer", fn);
    const bool fc = h->cfg.arch == IDQN_ARCH_FC, gc = (h->cfg.arch == IDQN_ARCH_CNN && h->gc.on) || h->imp.on;
    IDQN_REQUIRE((fc || gc) && h->cfg.n_quantiles == 0 && h->iqn.N == 0,
                 "%s: serves MLP handles, general-shape cnn handles and impala handles (plane-path cnn handles: idqn_learn_on_replay; the f32 MFMA "
                 "conv mode and quantile heads: gather, then learn on the batch)", fn);
    IDQN_REQUIRE(batch >= 1 && batch <= h->cfg.max_batch, "%s: batch %d not in [1, %d]", fn, batch, h->cfg.max_batch);
    IDQN_REQUIRE(batch_mean_divisor >= batch, "%s: mean divisor %d < batch %d", fn, batch_mean_divisor, batch);
    IDQN_REQUIRE(!(flags & (IDQN_F_STOP_AFTER_DENSE0 | IDQN_F_STOP_BEFORE_DENSE0_WGRAD)), "%s: the IDQN_F_STOP_* flags belong to the MFMA cnn path", fn);
    IDQN_REQUIRE(n_frames >= 1 && frame_bytes >= 1, "%s: n_frames = %ld, frame_bytes = %ld", fn, (long)n_frames, (long)frame_bytes);
    long obs_elems;
    if (fc) {
        obs_elems = h->fc.d[0];
        IDQN_REQUIRE(stack >= 1 && stack <= 8 && frame_bytes % 4 == 0 && frame_bytes * stack == 4L * obs_elems && ((uintptr_t)frame_ring_dev & 3) == 0,
                     "%s: an MLP handle takes float32 frames with frame_bytes * stack == 4 * %ld and stack in 1..8 (got frame_bytes %ld, stack %d)",
                     fn, obs_elems, (long)frame_bytes, stack);
    } else {
        obs_elems = (long)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c;
        IDQN_REQUIRE(stack == h->cfg.obs_c && frame_bytes == (int64_t)h->cfg.obs_h * h->cfg.obs_w,
                     "%s: a general-shape cnn / impala handle takes uint8 frames of obs_h x obs_w bytes, stack == obs_c (got stack %d, frame_bytes %ld, "
                     "obs %d x %d x %d)", fn, stack, (long)frame_bytes, h->cfg.obs_h, h->cfg.obs_w, h->cfg.obs_c);
    }
    *obs_elems_out = obs_elems;
    return IDQN_OK;
}

// update_online_params on the frame ring for the handles learn_on_replay refuses: MLP ("fc") handles over float32 frames and
// general-shape cnn handles (h->gc.on) over uint8 frames.  Exactly one of slots_host / slots_dev is set.
//   * a batch that runs k_fc_step_par (<= 32 samples, a net that fits it): the ring is that launch's minibatch source
//     (k_fc_step_par) -- the one-launch step stays one launch.  IDQN_FC_REPLAY_STAGE=1 sends these batches through the
//     staging launch as well (the A/B of tools/bench_fc_learn_on_replay.py).
//   * everything else: ONE staging launch (k_rps_stage; per RPS_ARG_SLOTS samples when the slots travel as kernel arguments)
//     writes the stacked minibatches and the rows' scalars into buffers the handle owns and the plain step runs on those.
// Either way only that first launch reads the ring, the rows and the slots (StepIn).
// Every refusal comes before anything is enqueued.
static int learn_on_replay_fc(idqn_handle_t h, StepIn in, void* stream) {
    const int32_t *slots_host = in.slots_host, *slots_dev = in.slots_dev;
    const int batch = in.batch;
    long obs_elems;
    if (const int rc = replay_fc_check(h, in.fn, (const uint8_t*)in.frames, in.n_frames, in.frame_bytes, in.rows, slots_host, slots_dev, batch, in.stack,
                                       in.mean_divisor, in.flags, &obs_elems))
        return rc;
    const bool fc = h->cfg.arch == IDQN_ARCH_FC;
    if (const int rc = ensure_replay_scalars(h)) return rc;
    if (!h->rp_state) {
        const long words = ((long)h->cfg.max_batch * obs_elems * (fc ? 4 : 1) + 3) / 4;
        float *s = nullptr, *s2 = nullptr;
        int rc;
        if ((rc = alloc_zero(&s, words, h, "replay state"))) return rc;
        if ((rc = alloc_zero(&s2, words, h, "replay next_state"))) return rc;
        IDQN_HIP_CHECK(hipStreamSynchronize(nullptr));  // (the zero-fill runs on the null stream)
        h->rp_state = s; h->rp_next = s2;
    }
    // the step's kernel is told the handle-owned minibatch either way (k_fc_step_par reads the ring and the rows instead)
    in.state = h->rp_state; in.next_state = h->rp_next; in.action = h->rp_action; in.reward = h->rp_reward; in.terminal = h->rp_terminal;
    if (fc && h->fcp_plan_.floats && batch <= RPS_PAR_SLOTS && !fc_replay_always_stage()) return learn_step(h, in, (hipStream_t)stream);
    RpsStageArgs a;
    a.frames = (const uint8_t*)in.frames; a.rows = in.rows; a.n_frames = in.n_frames; a.frame_elems = fc ? in.frame_bytes / 4 : in.frame_bytes;
    a.stack = in.stack; a.B = batch; a.first = 0;
    a.s_out = h->rp_state; a.n_out = h->rp_next; a.a_out = h->rp_action; a.r_out = h->rp_reward; a.t_out = h->rp_terminal;
    hipStream_t q = (hipStream_t)stream;
    const long bytes = obs_elems * (fc ? 4 : 1);
    const unsigned chunks = (unsigned)std::min<long>(16, std::max<long>(1, (bytes + 4 * 256 - 1) / (4 * 256)));  // one iteration per lane up to 16 KB
    if (slots_dev) {
        const dim3 grid((unsigned)batch, 2, chunks);
        if (fc) hipLaunchKernelGGL((k_rps_stage<float, RpsSlotsDev>), grid, dim3(256), 0, q, a, RpsSlotsDev{slots_dev});
        else hipLaunchKernelGGL((k_rps_stage<uint8_t, RpsSlotsDev>), grid, dim3(256), 0, q, a, RpsSlotsDev{slots_dev});
    } else {
        for (int first = 0; first < batch; first += RPS_ARG_SLOTS) {  // (one launch for batches of <= 256 samples)
            const int n = std::min<int>(RPS_ARG_SLOTS, batch - first);
            RpsSlots sl;
            memset(&sl, 0, sizeof(sl));
            memcpy(sl.slot, slots_host + first, (size_t)n * 4);
            a.first = first;
            const dim3 grid((unsigned)n, 2, chunks);
            if (fc) hipLaunchKernelGGL((k_rps_stage<float, RpsSlots>), grid, dim3(256), 0, q, a, sl);
            else hipLaunchKernelGGL((k_rps_stage<uint8_t, RpsSlots>), grid, dim3(256), 0, q, a, sl);
        }
    }
    IDQN_HIP_CHECK(hipGetLastError());
    in.frames = nullptr;  // staged: the step runs on the handle-owned minibatch
    return learn_step(h, in, q);
}

extern "C" int idqn_learn_on_replay_fc(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                       const int32_t* rows_dev, const int32_t* slots_host, int32_t batch, int32_t stack,
                                       int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_host, "idqn_learn_on_replay_fc: null pointer");
    return learn_on_replay_fc(h, ring_step(h, "idqn_learn_on_replay_fc", frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host, nullptr, batch,
                                           stack, batch_mean_divisor, flags), stream);
}

extern "C" int idqn_learn_on_replay_fc_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                           const int32_t* rows_dev, const int32_t* slots_dev, int32_t batch, int32_t stack,
                                           int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_dev, "idqn_learn_on_replay_fc_dev: null pointer");
    return learn_on_replay_fc(h, ring_step(h, "idqn_learn_on_replay_fc_dev", frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, slots_dev,
                                           batch, stack, batch_mean_divisor, flags), stream);
}

// The handle's host-argument staging ring (idqn_learn_steps_on_replay_fc's slots, the uniforms of idqn_per_learn_on_replay and
// idqn_per_learn_steps_on_replay): `bytes`
// <= STEPS_BLOCK_BYTES of ordinary host memory are copied into the next pinned block and their upload into the block's device
// twin, h->steps.dev(), is enqueued on q.  The caller records h->steps.guard(q) behind the last launch that reads the twin.
// A block holds the largest of them: idqn_per_learn_steps_on_replay's IDQN_MAX_STEPS_PER_CALL x PER_STEP_MAX_N float64 uniforms.
static constexpr size_t STEPS_SLOTS_BYTES = (size_t)IDQN_MAX_STEPS_PER_CALL * RPS_PAR_SLOTS * 4;  // the slots of one idqn_learn_steps_on_replay_fc call
static constexpr size_t STEPS_BLOCK_BYTES = (size_t)IDQN_MAX_STEPS_PER_CALL * PER_STEP_MAX_N * 8;
static_assert(STEPS_BLOCK_BYTES >= STEPS_SLOTS_BYTES, "the slots fit a block too");
static int steps_stage(idqn_handle_t h, const void* host, size_t bytes, hipStream_t q) {
    if (const int rc = h->steps.acquire(STEPS_BLOCK_BYTES)) return rc;
    memcpy(h->steps.pin(), host, bytes);
    return h->steps.upload(bytes, q);
}

// n_steps consecutive update_online_params on the frame ring as ONE C call (include/idqn_hip.h).  Exactly one of slots_host /
// slots_dev is set, [n_steps][batch].
//   * persistent route -- what learn_on_replay_fc runs through the one-launch step (an fc handle whose plan fits, batch <= 32,
//     IDQN_FC_REPLAY_STAGE unset): ONE launch of k_fc_steps_par (fc_steps_kernels.h) reads the slots from a device block; host
//     slots reach it through the handle's staging ring (pinned block -> asynchronous copy -> device block, each block guarded by
//     an event that is waited on before the block is rewritten, so back-to-back calls need no synchronisation).
//   * loop route -- every other handle and batch learn_on_replay_fc serves: its n_steps steps enqueued here, one after the other.
//     IDQN_FC_LEARN_STEPS_LOOP=1 sends everything this way (the A/B of tools/bench_fc_learn_steps.py).
// Every refusal comes before anything is enqueued or allocated.
static int learn_steps_on_replay_fc(idqn_handle_t h, const char* fn, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                    const int32_t* rows_dev, const int32_t* slots_host, const int32_t* slots_dev, int32_t n_steps,
                                    int32_t batch, int32_t stack, int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(h && frame_ring_dev && rows_dev && (slots_host || slots_dev), "%s: null pointer", fn);
    IDQN_REQUIRE(n_steps >= 1 && n_steps <= IDQN_MAX_STEPS_PER_CALL, "%s: n_steps %d not in [1, %d]", fn, n_steps, IDQN_MAX_STEPS_PER_CALL);
    IDQN_REFUSE_IMPALA(h, fn);
    IDQN_REQUIRE(flags == 0, "%s: takes no flags (got 0x%x): profile or split a single step through idqn_learn_on_replay_fc", fn, flags);
    IDQN_REQUIRE(!h->is_weight && !h->td_abs,
                 "%s: the handle has prioritized-replay buffers set (idqn_set_per_buffers): weights and |TD| belong to one step", fn);
    long obs_elems;
    if (const int rc = replay_fc_check(h, fn, frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host, slots_dev, batch, stack, batch_mean_divisor,
                                       flags, &obs_elems))
        return rc;
    const bool persistent = h->cfg.arch == IDQN_ARCH_FC && h->fcs_plan_.floats && batch <= RPS_PAR_SLOTS && !fc_replay_always_stage() &&
                            !fc_steps_force_loop();
    if (!persistent) {
        for (int i = 0; i < n_steps; ++i) {  // (no weights, no |TD|: refused above)
            const long o = (long)i * batch;
            if (const int rc = learn_on_replay_fc(h, ring_step(nullptr, fn, frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host ? slots_host + o : nullptr,
                                                               slots_dev ? slots_dev + o : nullptr, batch, stack, batch_mean_divisor, 0), stream))
                return rc;
        }
        return IDQN_OK;
    }
    hipStream_t q = (hipStream_t)stream;
    const bool staged = !slots_dev;
    if (staged) {
        if (const int rc = steps_stage(h, slots_host, (size_t)n_steps * batch * 4, q)) return rc;
        slots_dev = (const int32_t*)h->steps.dev();
    }
    h->pend_B = 0; h->pend_stage = 0;
    h->tl_on = false;
    const FcArgs a = fc_args(h, batch, batch_mean_divisor, false);  // (the ring is the minibatch source: the batch pointers stay NULL)
    h->dominant = "k_fc_steps_par";  // (the loop route above leaves the single step's name)
    hipLaunchKernelGGL(k_fc_steps_par<FcRingSrc<RpsSlotsDev>>, dim3(h->cfg.n_heads), dim3(FCM_T), (size_t)h->fcs_plan_.floats * 4, q, a, h->fcs_plan_, h->ad,
                       h->online, h->mu, h->nu, (int)n_steps,
                       fc_ring_src(frame_ring_dev, rows_dev, n_frames, frame_bytes, stack, RpsSlotsDev{slots_dev}));
    IDQN_HIP_CHECK(hipGetLastError());
    return staged ? h->steps.guard(q) : IDQN_OK;
}

extern "C" int idqn_learn_steps_on_replay_fc(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                             const int32_t* rows_dev, const int32_t* slots_host, int32_t n_steps, int32_t batch, int32_t stack,
                                             int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_host, "idqn_learn_steps_on_replay_fc: null pointer");
    return learn_steps_on_replay_fc(h, "idqn_learn_steps_on_replay_fc", frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host, nullptr, n_steps,
                                    batch, stack, batch_mean_divisor, flags, stream);
}

extern "C" int idqn_learn_steps_on_replay_fc_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                                 const int32_t* rows_dev, const int32_t* slots_dev, int32_t n_steps, int32_t batch, int32_t stack,
                                                 int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_dev, "idqn_learn_steps_on_replay_fc_dev: null pointer");
    return learn_steps_on_replay_fc(h, "idqn_learn_steps_on_replay_fc_dev", frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, slots_dev, n_steps,
                                    batch, stack, batch_mean_divisor, flags, stream);
}

// iIQN.update_online_params on the HBM frame ring: the same helper, the quantile step behind the staging launch (k_iqn_loss reads
// action / reward / terminal from h->rp_action / rp_reward / rp_terminal like the plain TD kernel).
extern "C" int idqn_iqn_learn_on_replay(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                        const int32_t* rows_dev, const int32_t* slots_host, const float* tau_dev, int32_t batch,
                                        int32_t stack, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_host && tau_dev, "idqn_iqn_learn_on_replay: null pointer");
    StepIn in = ring_step(h, "idqn_iqn_learn_on_replay", frame_ring_dev, n_frames, frame_bytes, rows_dev, slots_host, nullptr, batch, stack, batch, flags);
    in.tau = tau_dev;
    return learn_on_replay(h, in, stream);
}

extern "C" int idqn_iqn_learn_on_replay_dev(idqn_handle_t h, const uint8_t* frame_ring_dev, int64_t n_frames, int64_t frame_bytes,
                                            const int32_t* rows_dev, const int32_t* slots_dev, const float* tau_dev, int32_t batch,
                                            int32_t stack, uint32_t flags, void* stream) {
    IDQN_REQUIRE(slots_dev && tau_dev, "idqn_iqn_learn_on_replay_dev: null pointer");
    StepIn in = ring_step(h, "idqn_iqn_learn_on_replay_dev", frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, slots_dev, batch, stack, batch, flags);
    in.tau = tau_dev;
    return learn_on_replay(h, in, stream);
}

// n_steps consecutive prioritized learner steps on the frame ring, the driver of idqn_per_learn_on_replay (n_steps == 1) and
// idqn_per_learn_steps_on_replay; P is idqn_per_step_t or idqn_per_steps_t (the same fields; tau_dev is the former's).  Between two
// steps the write-back of step i and the draw of step i + 1 are adjacent launches of which the first is one workgroup and the
// second must read the tree the first leaves: they are ONE launch, k_per_turn (per_turn_kernels.h).  Enqueued: one upload of the
// n_steps rows of uniforms (staging ring) -> k_per_draw on row 0 -> for every step the replay-sourced step of the handle's family
// on that step's rows of leaves, weights and |TD|, in force for that step only -> k_per_turn behind every step but the last ->
// k_per_write_back: 2 n_steps + 1 launches beside the steps' own.  `marks`: the sampler launches appear in the step timeline
// (IDQN_F_PROFILE_ALL; the single step has never listed them, and its callers read the table of the step alone).
// Every refusal -- the entries', this one's and the dispatched step's -- comes before anything is enqueued, allocated or staged.
template <class P>
static int per_learn_on_replay(idqn_handle_t h, const char* fn, const P& per, const float* tau_dev, const uint8_t* frame_ring_dev, int64_t n_frames,
                               int64_t frame_bytes, const int32_t* rows_dev, int32_t n_steps, int32_t batch, int32_t stack,
                               int32_t batch_mean_divisor, uint32_t flags, void* stream, bool marks) {
    IDQN_REFUSE_IMPALA(h, fn);
    IDQN_REQUIRE(!(flags & ~(IDQN_F_PROFILE | IDQN_F_PROFILE_ALL)), "%s: only the profile flags are supported (got 0x%x)", fn, flags);
    IDQN_REQUIRE(!h->is_weight && !h->td_abs,
                 "%s: the handle has prioritized-replay buffers set (idqn_set_per_buffers): the call sets its own for its duration", fn);
    IDQN_REQUIRE(batch >= 1 && batch <= PER_STEP_MAX_N && batch <= h->cfg.max_batch, "%s: batch %d not in [1, min(%d, %d)]", fn, batch,
                 PER_STEP_MAX_N, h->cfg.max_batch);
    const int K = h->cfg.n_heads;
    const char* bad = per_step_args_error(per_sampler_of(per, per.uniforms_host, K), batch);  // (uniforms: NULL or not)
    IDQN_REQUIRE(!bad, "%s: %s (depth %d, batch %d, n_items %ld)", fn, bad, per.depth, batch, (long)per.n_items);
    const bool quantile = h->iqn.N > 0, plane = h->cfg.arch == IDQN_ARCH_CNN && h->planes && !h->gc.on;
    IDQN_REQUIRE(quantile == (tau_dev != nullptr), "%s: tau_dev goes with quantile heads (the handle has n_quantiles = %d)", fn, h->iqn.N);
    if (quantile || plane) {
        if (const int rc = replay_check(h, fn, frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, per.leaves_dev, batch, stack, tau_dev, flags))
            return rc;
        IDQN_REQUIRE(quantile || batch_mean_divisor >= batch, "%s: mean divisor %d < batch %d", fn, batch_mean_divisor, batch);
    } else {
        long obs_elems;
        if (const int rc = replay_fc_check(h, fn, frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, per.leaves_dev, batch, stack,
                                           batch_mean_divisor, flags, &obs_elems))
            return rc;
    }
    hipStream_t q = (hipStream_t)stream;
    int rc;
    if ((rc = steps_stage(h, per.uniforms_host, (size_t)n_steps * batch * 8, q))) return rc;
    const double* u = (const double*)h->steps.dev();
    if (marks && (rc = tl_begin(h, flags, q))) return rc;
    if ((rc = per_draw(per.nodes_dev, per.depth, u, batch, per.stratified, per.n_items, per.beta, per.leaves_dev, per.weights_dev, stream)))
        return rc;
    if (marks) tl_mark(h, q, "k_per_draw");
    // the last launch that reads the staged uniforms: k_per_draw of a single step, else the last k_per_turn
    if (n_steps == 1 && (rc = h->steps.guard(q))) return rc;
    for (int i = 0; i < n_steps; ++i) {
        const long o = (long)i * batch;
        int32_t* leaves = per.leaves_dev + o;
        float* td = per.td_abs_dev + o * K;
        double* pri = per.priorities_dev ? per.priorities_dev + o : nullptr;
        StepIn in = ring_step(nullptr, fn, frame_ring_dev, n_frames, frame_bytes, rows_dev, nullptr, leaves, batch, stack,
                              quantile ? batch : batch_mean_divisor, flags);
        in.tau = tau_dev; in.is_weight = per.weights_dev + o; in.td_abs = td;
        if ((rc = quantile || plane ? learn_on_replay(h, in, stream) : learn_on_replay_fc(h, in, stream))) return rc;
        if (i + 1 < n_steps) {
            if ((rc = per_turn(per.nodes_dev, per.depth, leaves, td, K, batch, per.reduce_max, per.eps, per.alpha, pri, per.max_priority_dev,
                               per.tree_scratch_dev, u + o + batch, per.stratified, per.n_items, per.beta, leaves + batch,
                               per.weights_dev + o + batch, stream)))
                return rc;
            if (marks) tl_mark(h, q, "k_per_turn");
            if (i + 2 == n_steps && (rc = h->steps.guard(q))) return rc;
        } else {
            if ((rc = per_write_back(per.nodes_dev, per.depth, leaves, td, K, batch, per.reduce_max, per.eps, per.alpha, pri,
                                     per.max_priority_dev, per.tree_scratch_dev, stream)))
                return rc;
            if (marks) tl_mark(h, q, "k_per_write_back");
        }
    }
    return IDQN_OK;
}

// One prioritized learner step as ONE C call (include/idqn_hip.h): the driver at one step; handles with quantile heads take tau_dev.
extern "C" int idqn_per_learn_on_replay(idqn_handle_t h, const idqn_per_step_t* per, const uint8_t* frame_ring_dev, int64_t n_frames,
                                        int64_t frame_bytes, const int32_t* rows_dev, int32_t batch, int32_t stack,
                                        int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    const char* fn = "idqn_per_learn_on_replay";
    IDQN_REQUIRE(h && per && per->weights_dev && per->td_abs_dev, "%s: null pointer", fn);
    return per_learn_on_replay(h, fn, *per, per->tau_dev, frame_ring_dev, n_frames, frame_bytes, rows_dev, 1, batch, stack, batch_mean_divisor, flags,
                               stream, false);
}

// n_steps of them as ONE C call (include/idqn_hip.h): the driver, where n_steps calls of idqn_per_learn_on_replay make 3 n_steps
// sampler launches and n_steps uploads; handles with quantile heads are not served.
extern "C" int idqn_per_learn_steps_on_replay(idqn_handle_t h, const idqn_per_steps_t* per, const uint8_t* frame_ring_dev, int64_t n_frames,
                                              int64_t frame_bytes, const int32_t* rows_dev, int32_t n_steps, int32_t batch, int32_t stack,
                                              int32_t batch_mean_divisor, uint32_t flags, void* stream) {
    const char* fn = "idqn_per_learn_steps_on_replay";
    IDQN_REQUIRE(h && per && per->weights_dev && per->td_abs_dev, "%s: null pointer", fn);
    IDQN_REQUIRE(h->iqn.N == 0, "%s: handles with quantile heads are not served (n_quantiles = %d): idqn_per_learn_on_replay, step by step", fn,
                 h->iqn.N);
    IDQN_REQUIRE(n_steps >= 1 && n_steps <= IDQN_MAX_STEPS_PER_CALL, "%s: n_steps %d not in [1, %d]", fn, n_steps, IDQN_MAX_STEPS_PER_CALL);
    return per_learn_on_replay(h, fn, *per, nullptr, frame_ring_dev, n_frames, frame_bytes, rows_dev, n_steps, batch, stack, batch_mean_divisor,
                               flags, stream, true);
}

// One i-IQN gradient step (include/idqn_hip.h).  With idqn_set_per_buffers the loss launch takes the importance weights and
// writes the per-sample mean |pairwise TD error| (k_iqn_loss<true>); without them it is the plain launch.
extern "C" int idqn_iqn_learn_on_batch(idqn_handle_t h, const void* state_dev, const void* next_state_dev,
                                       const int32_t* action_dev, const float* reward_dev, const uint8_t* terminal_dev,
                                       const float* tau_dev, int32_t batch, uint32_t flags, void* stream) {
    IDQN_REQUIRE(h && state_dev && next_state_dev && action_dev && reward_dev && terminal_dev && tau_dev,
                 "idqn_iqn_learn_on_batch: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_iqn_learn_on_batch");
    IDQN_REQUIRE(h->iqn.N > 0, "idqn_iqn_learn_on_batch: the handle was created without quantile heads (cfg.n_quantiles)");
    IDQN_REQUIRE(batch >= 1 && batch <= 256 && batch <= h->cfg.max_batch, "idqn_iqn_learn_on_batch: batch %d not in [1, min(256, %d)]",
                 batch, h->cfg.max_batch);
    IDQN_REQUIRE(!(flags & ~(IDQN_F_PROFILE | IDQN_F_PROFILE_ALL)), "idqn_iqn_learn_on_batch: only the profile flags are supported");
    StepIn in = batch_step(h, "idqn_iqn_learn_on_batch", state_dev, next_state_dev, action_dev, reward_dev, terminal_dev, batch, batch, flags);
    in.tau = tau_dev;
    return learn_step(h, in, (hipStream_t)stream);
}

// The quantile step (in.tau): the plane trunk without its Dense_0, the fraction blocks of the i-IQN heads, the conv backward
static int iqn_learn(idqn_handle_t h, const StepIn& in, hipStream_t q) {
    const int batch = in.batch;
    const uint32_t flags = in.flags;
    const float* tau_dev = in.tau;
    IqnWs& w = h->iqn;
    const int K = h->cfg.n_heads, A = h->cfg.n_actions;
    const int nb = cdiv(batch, 32), NB = w.N * nb;  // blocks per virtual net: fraction q of sample block s is block s N + q
    int rc;
    // trunk of the 2K nets (online on s, target on s'), then the fraction blocks of the 3K virtual nets
    if ((rc = cnn_forward(h, h->train, (const uint8_t*)in.state, (const uint8_t*)in.next_state, batch, q, false, in.frames ? &in : nullptr))) return rc;
    if ((rc = iqn_heads_forward(h, w.wbase_v, w.V, K, h->train.a3, tau_dev, batch, q))) return rc;
    IqnZArgs za;
    za.qpart = w.qpart; za.wbase = w.wbase_v; za.z = w.z; za.b1_off = h->off_b1; za.N = NB; za.NJC = h->J / 32; za.A = A;
    hipLaunchKernelGGL(k_iqn_z, dim3((unsigned)(w.V * NB)), dim3(256), 0, q, za);
    tl_mark(h, q, "iqn quantile values");
    IqnLossArgs la;
    la.z = w.z; la.K = K; la.N = w.N; la.A = A; la.nb = nb; la.lpart = w.lpart;
    la.B = batch; la.Bdiv = batch; la.action = in.action; la.reward = in.reward; la.terminal = in.terminal; la.tau = tau_dev;
    la.gamma_n = h->gamma_n; la.dq = w.dq; la.losses = h->losses; la.count = h->count; la.cum = h->cum; la.finish_step = 1;
    la.dbg = w.dbg; la.gate_err = w.gate + 2L * K * cdiv(h->F, 256);
    la.is_weight = in.is_weight; la.td_abs = in.td_abs;
    // (N <= 64: at most 22 KB of dynamic LDS with the priority reduction buffer, inside the default limit)
    const size_t loss_lds = (size_t)(2 * w.N * 32 + 32 * 32 + 8 * 32) * 4;
    if (la.is_weight || la.td_abs) hipLaunchKernelGGL(k_iqn_loss<true>, dim3(K, nb), dim3(256), loss_lds + 8 * 32 * 4, q, la);
    else hipLaunchKernelGGL(k_iqn_loss<false>, dim3(K, nb), dim3(256), loss_lds, q, la);
    if (nb > 1) hipLaunchKernelGGL(k_iqn_loss_sum, dim3(1), dim3(256), 0, q, la);
    tl_mark(h, q, "iqn quantile huber loss");
    const long w0n = h->g_w0_end - h->g_w0_begin;
    IqnDhArgs da;
    da.hbuf = w.hbuf; da.dq = w.dq; da.wbase = w.wbase_v; da.w1_off = h->off_w1;
    da.K = K; da.N = NB; da.J = h->J; da.A = A; da.dh = w.dh; da.hpart = w.hpart;
    const int HG = w.HG * nb;  // groups of N / HG blocks each
    hipLaunchKernelGGL(k_iqn_dh, dim3(h->J / 32, K, HG), dim3(256), 0, q, da);
    tl_mark(h, q, "iqn dh + dense1 grads");
    {
        IqnHeadGradSumArgs hs;
        hs.hpart = w.hpart; hs.grad = h->grad; hs.gP = h->gP;
        hs.g_b0_off = h->off_b0 - w0n; hs.g_w1_off = h->off_w1 - w0n; hs.g_b1_off = h->off_b1 - w0n;
        hs.K = K; hs.J = h->J; hs.A = A; hs.QG = HG;
        hipLaunchKernelGGL(k_iqn_head_grad_sum, dim3((unsigned)cdiv((long)h->J * A + h->J + A, 256), K), dim3(256), 0, q, hs);
        tl_mark(h, q, "iqn head grads (group sums)");
    }
    bool wgrad_done = false;
    {   // W0 . dh for every block (plain rows)
        DenseDgradArgs dd;
        memset(&dd, 0, sizeof(dd));
        dd.dh = w.dh; dd.raw = w.dx; dd.wbase = h->train.wbase; dd.w_off = h->off_w0;
        dd.K = K; dd.nb = NB; dd.n_ft = h->F / 32; dd.F = h->F; dd.J = h->J; dd.C = h->conv[2].CO; dd.g = h->gda3;
        dd.n_items = (long)K * NB * cdiv(dd.n_ft, 4);
        if (NB % 8 == 0 && h->J % 16 == 0) {
            IqnD0DgradArgs g;
            g.dh = w.dh; g.wbase = h->train.wbase; g.dx = w.dx; g.w_off = h->off_w0; g.K = K; g.nb = NB; g.F = h->F; g.J = h->J;
            const size_t lds = 2 * (size_t)IG_STAGE;
            const int n_d = K * (NB / 8) * cdiv(h->F, 256);
            w.d0_adam_done = false;
            // the weight-gradient GEMM rides in the same launch
            if (w.g1 && w.bwd_items[nb - 1] && w.bwd_fuse[nb - 1] && debug_int("IDQN_IQN_ADAM_FUSE", 1)) {
                // one split, Adam in its epilogue (k_iqn_d0_bwd_adam): where the plan says it beats two splits + the Adam pass
                const int n_groups = K * cdiv(h->F, 256);
                IqnD0WgradArgs gw;
                gw.x = w.xq; gw.dh = w.dh; gw.g[0] = gw.g[1] = nullptr; gw.K = K; gw.nb = NB; gw.F = h->F; gw.J = h->J; gw.KS = 1;
                gw.theta = debug_on("IDQN_IQN_ADAM_SKIP") ? nullptr : h->online; gw.mu = h->mu; gw.nu = h->nu; gw.bcinv = h->bcinv; gw.ad = h->ad; gw.P = h->L.head_stride; gw.w_off = h->off_w0; gw.dump = reinterpret_cast<const char*>(w.g1);  // (g1: K * F * J floats, unused on this path)
                IqnD0Gate gate;
                gate.arrived = w.gate; gate.passed = w.gate + n_groups; gate.err = w.gate + 2L * n_groups;
                gate.prof = (h->cprof && h->cprof_role == 11) ? (long long*)h->cprof : nullptr;
                static LdsAttrMark attr;
                if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_bwd_adam<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(k_iqn_d0_bwd_adam<2>, dim3((unsigned)w.bwd_blocks[nb - 1]), dim3(512), lds, q, g, gw, gate, w.bwd_items[nb - 1]);
                wgrad_done = true;
                w.d0_adam_done = true;
            } else if (w.g1 && NB % 16 == 0) {
                IqnD0WgradArgs gw;
                memset(&gw, 0, sizeof(gw));
                gw.x = w.xq; gw.dh = w.dh; gw.g[0] = h->grad + h->g_w0_base; gw.g[1] = w.g1; gw.K = K; gw.nb = NB; gw.F = h->F; gw.J = h->J; gw.KS = 2;
                static LdsAttrMark attr;
                if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_bwd<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(k_iqn_d0_bwd<2>, dim3((unsigned)(n_d + K * cdiv(h->F, 256) * gw.KS * (h->J / 256))), dim3(512), lds, q, g, n_d, gw);
                wgrad_done = true;
            } else {
                static LdsAttrMark attr;
                if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_dgrad<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(k_iqn_d0_dgrad<2>, dim3((unsigned)n_d), dim3(512), lds, q, g);
            }
        } else {
            hipLaunchKernelGGL((k_dense0_dgrad<4>), dim3((unsigned)dd.n_items), dim3(256), h->J * 32 * 4, q, dd);
        }
        tl_mark(h, q, w.d0_adam_done ? "iqn dense0 dgrad + wgrad + adam" : wgrad_done ? "iqn dense0 dgrad + wgrad" : "iqn dense0 dgrad");
    }
    const int QG = w.QG;
    {  // (the forward of this step packed the embedding kernels and wrote the cos planes)
        IqnEmbedBwd3Args e3;
        e3.cosp = w.cosp; e3.cosa = w.cosa; e3.wep = w.wep; e3.wbase = w.wbase_v; e3.psi = h->train.a3; e3.dx = w.dx;
        e3.dpsi = w.dpsi; e3.gpart = w.gpart; e3.be_off = w.off_be; e3.K = K; e3.N = w.N; e3.F = h->F; e3.nb = nb;
        const size_t lds = 2 * 2 * 12 * 512 * 2;
        static LdsAttrMark attr;
        if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_embed_bwd3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_iqn_embed_bwd3, dim3((unsigned)cdiv(h->F / 32, 4), K, QG * nb), dim3(256), lds, q, e3);
    }
    tl_mark(h, q, "iqn embedding backward");
    {
        IqnEmbedGradSumArgs gs;
        gs.gpart = w.gpart; gs.grad = h->grad; gs.gP = h->gP; gs.g_we_off = w.off_we - w0n; gs.g_be_off = w.off_be - w0n;
        gs.K = K; gs.F = h->F; gs.QG = QG * nb;
        hipLaunchKernelGGL(k_iqn_embed_grad_sum, dim3((unsigned)cdiv(65L * h->F / 4, 256), K), dim3(256), 0, q, gs);
        tl_mark(h, q, "iqn embedding grads (group sums)");
    }
    {   // dL/dpsi of every sample block (the fraction groups' partials, in group order) -> ReLU mask, bf16 planes, per-position
        // sums: what the conv backward of the plain step reads
        Da3FinalizeArgs fa;
        fa.dpart = w.dpsi; fa.a3 = h->train.a3; fa.da3 = h->da3; fa.da3p = h->da3p; fa.pb = h->pbuf[2];
        fa.n_rows = (long)K * nb * h->F; fa.n_jt = QG; fa.F = h->F; fa.C = h->conv[2].CO; fa.K = K; fa.nb = nb; fa.g = h->gda3;
        hipLaunchKernelGGL(k_da3_finalize, dim3(cdiv(fa.n_rows * 8, 256)), dim3(256), 0, q, fa);
        tl_mark(h, q, "da3 finalize (sum, mask, planes)");
    }
    // Dense_0 weight gradient over the NB blocks of every head + Adam: inside the merged launch above, or as a GEMM with
    // two block splits and one streaming Adam pass (iqn_gemm.h), or (NB not a multiple of 16) the plain step's fused kernel
    if (w.d0_adam_done) {
    } else if (w.g1 && NB % 16 == 0) {
        const long n = (long)h->F * h->J;
        IqnD0WgradArgs g;
        memset(&g, 0, sizeof(g));
        g.x = w.xq; g.dh = w.dh; g.g[0] = h->grad + h->g_w0_base; g.g[1] = w.g1; g.K = K; g.nb = NB; g.F = h->F; g.J = h->J; g.KS = 2;
        const size_t lds = 2 * (size_t)IG_STAGE;
        static LdsAttrMark attr;
        if (attr.needs(lds)) IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_iqn_d0_wgrad<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (!wgrad_done) {
            hipLaunchKernelGGL(k_iqn_d0_wgrad<2>, dim3((unsigned)(K * cdiv(h->F, 256) * g.KS * (h->J / 256))), dim3(512), lds, q, g);
            tl_mark(h, q, "iqn dense0 wgrad");
        }
        IqnD0AdamArgs aa;
        aa.g[0] = g.g[0]; aa.g[1] = g.g[1]; aa.theta = h->online; aa.mu = h->mu; aa.nu = h->nu; aa.bcinv = h->bcinv; aa.ad = h->ad;
        aa.P = h->L.head_stride; aa.w_off = h->off_w0; aa.n = n; aa.KS = g.KS;
        hipLaunchKernelGGL(k_iqn_d0_adam, dim3((unsigned)cdiv(n / 4, 256), (unsigned)K), dim3(256), 0, q, aa);
        tl_mark(h, q, "iqn dense0 adam");
        IDQN_HIP_CHECK(hipGetLastError());
    } else if ((rc = launch_dense0_wgrad(h, w.xq, w.dh, NB, NB, 0, (long)NB * h->F * 32, (long)h->F * 32, 0, (long)NB * h->J * 32,
                                  (long)h->J * 32, true, (flags & IDQN_F_PROFILE) != 0, q, false)))
        return rc;
    if ((rc = cnn_backward_rest(h, batch, true, q))) return rc;
    return launch_adam(h, 0, h->L.head_stride, h->off_w0, h->off_b0, true, q);
}

extern "C" int idqn_iqn_q_values(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                                 const float* tau_dev, float* q_out_dev, int32_t* action_out_dev, void* stream) {
    IDQN_REQUIRE(h && states_dev && tau_dev && q_out_dev, "idqn_iqn_q_values: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_iqn_q_values");
    IDQN_REQUIRE(h->iqn.N > 0, "idqn_iqn_q_values: the handle was created without quantile heads (cfg.n_quantiles)");
    IDQN_REQUIRE(head >= 0 && head < h->cfg.n_heads && (which == 0 || which == 1), "idqn_iqn_q_values: bad head / which");
    IDQN_REQUIRE(n >= 1 && n <= h->cfg.max_batch, "idqn_iqn_q_values: n = %d, must be in [1, max_batch = %d]", n, h->cfg.max_batch);
    hipStream_t q = (hipStream_t)stream;
    IqnWs& w = h->iqn;
    const float* params = (which ? h->target : h->online) + (long)head * h->L.head_stride;
    h->infer.wbase = h->train.wbase + (which * h->cfg.n_heads + head);  // entry of the training table: no pointer upload
    h->infer_pbase = params;
    int rc;
    if ((rc = cnn_forward(h, h->infer, (const uint8_t*)states_dev, nullptr, n, q, false))) return rc;
    if ((rc = iqn_heads_forward(h, h->infer.wbase, 1, 1, h->infer.a3, tau_dev, n, q))) return rc;
    IqnQOutArgs qo;
    qo.qpart = w.qpart; qo.params = params; qo.b1_off = h->off_b1; qo.N = w.N; qo.NJC = h->J / 32; qo.A = h->cfg.n_actions;
    qo.n = n; qo.q_out = q_out_dev; qo.action = action_out_dev;
    hipLaunchKernelGGL(k_iqn_q_out, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, q, qo);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int idqn_backward_rest(idqn_handle_t h, void* stream) {
    IDQN_REFUSE_IMPALA(h, "idqn_backward_rest");
    IDQN_REQUIRE(h && h->pend_B > 0, "idqn_backward_rest: no backward pass is waiting (IDQN_F_STOP_* first)");
    const int B = h->pend_B;
    if (h->pend_stage == 2) h->pend_B = 0;  // stage 1 keeps B for idqn_export / idqn_finish_step_factored
    return cnn_backward_rest(h, B, false, (hipStream_t)stream);
}

extern "C" int idqn_export_dense0_factors(idqn_handle_t h, float* a3_out_dev, float* dh_out_dev, void* stream) {
    IDQN_REQUIRE(h && a3_out_dev && dh_out_dev, "idqn_export_dense0_factors: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_export_dense0_factors");
    IDQN_REQUIRE(h->pend_stage == 1 && h->pend_B > 0, "idqn_export_dense0_factors: needs IDQN_F_STOP_BEFORE_DENSE0_WGRAD first");
    const long nb = cdiv(h->pend_B, 32), K = h->cfg.n_heads;
    // the online nets are the first K * nb slots of the activation buffer
    IDQN_HIP_CHECK(hipMemcpyAsync(a3_out_dev, h->train.a3, (size_t)K * nb * h->F * 32 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    IDQN_HIP_CHECK(hipMemcpyAsync(dh_out_dev, dh_of(h, (int)nb), (size_t)K * nb * h->J * 32 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return IDQN_OK;
}

extern "C" int idqn_dense0_factors(idqn_handle_t h, float** factors_dev, int64_t* n_dh, int64_t* n_a3) {
    IDQN_REQUIRE(h && factors_dev && n_dh && n_a3, "idqn_dense0_factors: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_dense0_factors");
    IDQN_REQUIRE(h->pend_stage == 1 && h->pend_B > 0, "idqn_dense0_factors: needs IDQN_F_STOP_BEFORE_DENSE0_WGRAD first");
    const int nb = cdiv(h->pend_B, 32);
    *factors_dev = dh_of(h, nb);
    *n_dh = (int64_t)h->cfg.n_heads * nb * h->J * 32;
    *n_a3 = (int64_t)h->cfg.n_heads * nb * h->F * 32;
    return IDQN_OK;
}

extern "C" int idqn_finish_step_factored(idqn_handle_t h, const float* a3_all_dev, const float* dh_all_dev,
                                         int32_t nb_total, int32_t nb_inner, int64_t a3_outer, int64_t a3_head,
                                         int64_t a3_inner, int64_t dh_outer, int64_t dh_head, int64_t dh_inner,
                                         uint32_t phases, void* stream) {
    IDQN_REQUIRE(h && (phases & 3u) && !(phases & ~3u), "idqn_finish_step_factored: phases must be 1, 2 or 3");
    IDQN_REFUSE_IMPALA(h, "idqn_finish_step_factored");
    hipStream_t q = (hipStream_t)stream;
    int rc;
    if (phases & IDQN_FACTORED_DENSE0) {
        IDQN_REQUIRE(a3_all_dev && dh_all_dev, "idqn_finish_step_factored: null pointer");
        IDQN_REQUIRE(h->pend_stage == 1, "idqn_finish_step_factored: needs IDQN_F_STOP_BEFORE_DENSE0_WGRAD first");
        IDQN_REQUIRE(nb_total >= 1 && nb_inner >= 1 && nb_total % nb_inner == 0, "idqn_finish_step_factored: bad block counts");
        h->pend_stage = 3; h->pend_B = 0;
        if ((rc = launch_dense0_wgrad(h, a3_all_dev, dh_all_dev, nb_total, nb_inner, a3_outer, a3_head, a3_inner, dh_outer,
                                      dh_head, dh_inner, true, h->pend_profile, q)))
            return rc;
    }
    if (phases & IDQN_FACTORED_REST) {
        IDQN_REQUIRE(h->pend_stage == 3, "idqn_finish_step_factored: the Dense_0 phase has to come first");
        h->pend_stage = 0;
        // every other leaf, from grad_dev; count += 1 and cum_losses += losses ride in the same launch
        return launch_adam(h, 0, h->L.head_stride, h->off_w0, h->off_b0, false, q, h->cfg.arch == IDQN_ARCH_CNN);
    }
    return IDQN_OK;
}

int idqn_internal_dp_view(idqn_handle_t h, IdqnDpView* v) {  // (csrc/dp.hip)
    IDQN_REQUIRE(h && v, "null handle");
    IDQN_REFUSE_IMPALA(h, "the data-parallel step (idqn_dp_*)");
    IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_CNN && !h->gc.on && h->cfg.n_quantiles == 0,
                 "the data-parallel step is built for the MFMA cnn path of the i-DQN heads");
    v->grad = h->grad; v->losses = h->losses; v->td_abs = h->td_abs; v->n_small = (long)h->cfg.n_heads * h->gP + 64;
    v->K = h->cfg.n_heads; v->F = h->F; v->J = h->J;
    return IDQN_OK;
}

extern "C" int idqn_set_per_buffers(idqn_handle_t h, const float* weights_dev, float* td_abs_out_dev) {
    IDQN_REQUIRE(h, "idqn_set_per_buffers: null handle");
    h->is_weight = weights_dev;
    h->td_abs = td_abs_out_dev;
    return IDQN_OK;
}

extern "C" int idqn_apply_adam(idqn_handle_t h, void* stream) {
    IDQN_REQUIRE(h, "idqn_apply_adam: null handle");
    int rc = launch_adam(h, 0, h->L.head_stride, 0, 0, false, (hipStream_t)stream);
    if (rc) return rc;
    return step_epilogue(h, true, (hipStream_t)stream);
}

extern "C" int idqn_target_update(idqn_handle_t h, void* stream) {
    IDQN_REQUIRE(h, "idqn_target_update: null handle");
    hipStream_t q = (hipStream_t)stream;
    const long P = h->L.head_stride;
    const int K = h->cfg.n_heads;
    // idqn.py:78  target_params = params.copy()  -- a real copy, BEFORE the shift (idqn.py:80)
    IDQN_HIP_CHECK(hipMemcpyAsync(h->target, h->online, (size_t)K * P * 4, hipMemcpyDeviceToDevice, q));
    // idqn.py:13-17  params[k] <- params[k+1]; ascending k so every source is read before it is overwritten
    for (int k = 0; k + 1 < K; ++k)
        IDQN_HIP_CHECK(hipMemcpyAsync(h->online + (long)k * P, h->online + (long)(k + 1) * P, (size_t)P * 4,
                                      hipMemcpyDeviceToDevice, q));
    return IDQN_OK;
}

extern "C" int idqn_target_sync(idqn_handle_t h, void* stream) {
    IDQN_REQUIRE(h, "idqn_target_sync: null handle");
    const long P = h->L.head_stride;
    const int K = h->cfg.n_heads;
    // idqn.py:20-24  target[k] <- params[k-1] for k >= 1; target[0] stays frozen
    if (K > 1)
        IDQN_HIP_CHECK(hipMemcpyAsync(h->target + P, h->online, (size_t)(K - 1) * P * 4, hipMemcpyDeviceToDevice,
                                      (hipStream_t)stream));
    return IDQN_OK;
}

// argmax over the actions of each row, first maximum on ties (jnp.argmax, idqn.py:131)
__global__ void k_argmax_rows(const float* __restrict__ q, int n, int A, int32_t* __restrict__ out, volatile int32_t* mail,
                              unsigned* seq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int best = 0;
    float bv = q[(long)i * A];
    for (int ac = 1; ac < A; ++ac) {
        const float v = q[(long)i * A + ac];
        if (v > bv) { bv = v; best = ac; }
    }
    out[i] = best;
    if (mail && i == 0) {  // host mailbox of idqn_act_host (see k_act_head): the action, then the number that announces it
        const unsigned nn = seq[0] + 1u;
        seq[0] = nn;
        mail[0] = best;
        __threadfence_system();
        mail[1] = (int32_t)nn;
    }
}

// psi(s) of ONE state on the latency path (act_kernels.h): three k_act_conv launches, pixels and HWIO leaves as they are;
// the F features are left in h->act_a[2] in the order Dense_0's rows expect.
static int act_trunk(idqn_handle_t h, const float* params, const void* states_dev, hipStream_t q) {
    const float* in = nullptr;
    int ih = h->cfg.obs_h, iw = h->cfg.obs_w;
    for (int i = 0; i < 3; ++i) {
        const ConvL& l = h->conv[i];
        ActConvArgs a;
        a.in_u8 = i == 0 ? (const uint8_t*)states_dev : nullptr; a.in = in; a.params = params; a.out = h->act_a[i];
        a.w_off = l.w_off; a.b_off = l.b_off; a.IH = ih; a.IW = iw; a.CI = l.CI; a.OH = l.OH; a.OW = l.OW; a.CO = l.CO;
        a.K = l.K; a.S = l.S; a.PLh = l.PLh; a.PLw = l.PLw;
        a.KS = i == 0 ? 8 : 16;  // lane slices: layer 0 has 64 units of 4 channels, the others K*K*CI/32 units of 32
        const int per = 256 / a.KS;
        const dim3 grid(cdiv((long)l.OH * l.OW * l.CO, per));
        const int units = l.K * l.K * (l.CI % 32 == 0 ? l.CI / 32 : l.CI / 4), upt = cdiv(units, a.KS);
        IDQN_REQUIRE(l.CI % 32 == 0 || (l.CI == 4 && upt <= 8), "acting path: Conv_%d has %d input channels", i, l.CI);
        if (l.CI % 32 != 0) hipLaunchKernelGGL((k_act_conv<4, 8>), grid, dim3(256), 0, q, a);
        else if (upt <= 1) hipLaunchKernelGGL((k_act_conv<32, 1>), grid, dim3(256), 0, q, a);
        else if (upt <= 2) hipLaunchKernelGGL((k_act_conv<32, 2>), grid, dim3(256), 0, q, a);
        else { IDQN_REQUIRE(upt <= 4, "acting path: %d units per lane slice", upt); hipLaunchKernelGGL((k_act_conv<32, 4>), grid, dim3(256), 0, q, a); }
        in = h->act_a[i]; ih = l.OH; iw = l.OW;
    }
    return IDQN_OK;
}

static int q_values_impl(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                         float* q_out_dev, int32_t* action_out_dev, void* stream) {
    IDQN_REQUIRE(h && states_dev && q_out_dev, "idqn_q_values: null pointer");
    IDQN_REQUIRE(head >= 0 && head < h->cfg.n_heads && (which == 0 || which == 1), "idqn_q_values: bad head / which");
    IDQN_REQUIRE(n >= 1 && n <= 32, "idqn_q_values: n = %d, must be in [1, 32]", n);
    hipStream_t q = (hipStream_t)stream;
    const float* params = (which ? h->target : h->online) + (long)head * h->L.head_stride;
    if (h->imp.on) {  // impala: the three Stacks of the one net on the n states, then the generic dense forward
        const float* const* wb = h->train.wbase + (which * h->cfg.n_heads + head);
        int rc = impala_trunk(h, wb, 1, 1, n, (const uint8_t*)states_dev, (const uint8_t*)states_dev, h->imp.infer, q);
        if (rc) return rc;
        FcQArgs a;
        a.net = h->fc; a.params = params; a.s = h->imp.infer.x[2][2]; a.n = n; a.q_out = q_out_dev; a.ws = h->imp.inf_ws;
        if (h->imp.d0_split) {  // Dense_0 over the chip, the layers behind it in k_fc_q
            ImpD0Args d0;
            memset(&d0, 0, sizeof(d0));
            d0.x = h->imp.infer.x[2][2]; d0.hid = h->imp.inf_hid; d0.wbase = wb;
            d0.w_off = h->fc.w_off[0]; d0.b_off = h->fc.b_off[0]; d0.B = n; d0.F = h->F; d0.D = h->fc.d[1];
            if ((rc = imp_d0_forward(h, d0, 1, q))) return rc;
            a.net = h->imp.tail; a.s = h->imp.inf_hid;
        }
        hipLaunchKernelGGL(k_fc_q, dim3(1), dim3(256), 0, q, a);
        if (action_out_dev)
            hipLaunchKernelGGL(k_argmax_rows, dim3(1), dim3(64), 0, q, q_out_dev, n, h->cfg.n_actions, action_out_dev,
                               (volatile int32_t*)(h->act_use_mail ? h->act_mail_dev : nullptr), h->act_seq);
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    if (h->gc.on) {  // general-shape cnn: trunk of the one net on the n states, then the generic dense forward
        const float* const* wb = h->train.wbase + (which * h->cfg.n_heads + head);
        int rc = gcnn_trunk(h, wb, 1, 1, n, (const uint8_t*)states_dev, (const uint8_t*)states_dev, h->gc.inf_act, q);
        if (rc) return rc;
        FcQArgs a;
        a.net = h->fc; a.params = params; a.s = h->gc.inf_act[2]; a.n = n; a.q_out = q_out_dev; a.ws = h->gc.inf_ws;
        hipLaunchKernelGGL(k_fc_q, dim3(1), dim3(256), 0, q, a);
        if (action_out_dev)
            hipLaunchKernelGGL(k_argmax_rows, dim3(1), dim3(64), 0, q, q_out_dev, n, h->cfg.n_actions, action_out_dev,
                               (volatile int32_t*)(h->act_use_mail ? h->act_mail_dev : nullptr), h->act_seq);
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    if (h->cfg.arch == IDQN_ARCH_CNN && n == 1 && !act_generic() && h->J <= 512 && h->cfg.n_actions <= 32) {
        // one state: the latency path (act_kernels.h) -- pixels and parameter leaves as they are, five small launches
        int rc = act_trunk(h, params, states_dev, q);
        if (rc) return rc;
        ActDenseArgs d;
        d.a3 = h->act_a[2]; d.params = params; d.part = h->act_part; d.w_off = h->off_w0; d.F = h->F; d.J = h->J;
        d.NRG = std::max(1, 256 / (h->J / 128));  // one workgroup per CU
        hipLaunchKernelGGL(k_act_dense0, dim3(d.NRG * (h->J / 128)), dim3(256), 0, q, d);
        ActHeadArgs ha;
        ha.part = h->act_part; ha.params = params; ha.b0_off = h->off_b0; ha.w1_off = h->off_w1; ha.b1_off = h->off_b1;
        ha.NP = d.NRG; ha.J = h->J; ha.A = h->cfg.n_actions; ha.q_out = q_out_dev; ha.action = action_out_dev;
        ha.mail = h->act_use_mail ? h->act_mail_dev : nullptr; ha.seq = h->act_seq;
        hipLaunchKernelGGL(k_act_head, dim3(1), dim3(1024), 0, q, ha);
        IDQN_HIP_CHECK(hipGetLastError());
        return IDQN_OK;
    }
    if (h->cfg.arch == IDQN_ARCH_CNN) {
        // the acting net's parameter pointer is entry (which * K + head) of the training table: no pointer upload
        h->infer.wbase = h->train.wbase + (which * h->cfg.n_heads + head);
        h->infer_pbase = params;
        (void)params;
        int rc = cnn_forward(h, h->infer, (const uint8_t*)states_dev, nullptr, n, q);
        if (rc) return rc;
        HiddenArgs hi;
        hi.part = h->infer.part; hi.wbase = h->infer.wbase; hi.b0_off = h->off_b0; hi.w1_off = h->off_w1; hi.nb = 1;
        hi.NS = h->infer.NS; hi.J = h->J; hi.A = h->cfg.n_actions; hi.hbuf = h->infer_hbuf; hi.qpart = h->infer_qpart;
        hipLaunchKernelGGL(k_hidden, dim3(h->J / 32, 1), dim3(256), 0, q, hi);
        QOutArgs qo;
        qo.qpart = h->infer_qpart; qo.wbase = h->infer.wbase; qo.b1_off = h->off_b1; qo.NJC = h->J / 32;
        qo.A = h->cfg.n_actions; qo.n = n; qo.q_out = q_out_dev; qo.action = action_out_dev;
        hipLaunchKernelGGL(k_q_out, dim3(1), dim3(256), 0, q, qo);
    } else {
        FcQArgs a;
        a.net = h->fc; a.params = params; a.s = (const float*)states_dev; a.n = n; a.q_out = q_out_dev;
        a.ws = h->fc_ws + (long)h->cfg.n_heads * ((long)(h->fc.L + 3) * h->cfg.max_batch * h->fc.dmax + 2 * h->cfg.max_batch);
        if (n == 1 && h->fc.dmax <= FC_MAX_WIDTH) hipLaunchKernelGGL(k_fc_q1, dim3(1), dim3(512), 0, q, a);  // acting: one state
        else hipLaunchKernelGGL(k_fc_q, dim3(1), dim3(256), 0, q, a);
        if (action_out_dev)
            hipLaunchKernelGGL(k_argmax_rows, dim3(1), dim3(64), 0, q, q_out_dev, n, h->cfg.n_actions, action_out_dev,
                               (volatile int32_t*)(h->act_use_mail ? h->act_mail_dev : nullptr), h->act_seq);
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

extern "C" int idqn_q_values(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                             float* q_out_dev, void* stream) {
    return q_values_impl(h, which, head, states_dev, n, q_out_dev, nullptr, stream);
}

extern "C" int idqn_best_action(idqn_handle_t h, int32_t which, int32_t head, const void* states_dev, int32_t n,
                                float* q_out_dev, int32_t* action_out_dev, void* stream) {
    IDQN_REQUIRE(action_out_dev, "idqn_best_action: null pointer");
    return q_values_impl(h, which, head, states_dev, n, q_out_dev, action_out_dev, stream);
}

// The i-IQN chain behind idqn_iqn_act_host for the state in h->act_state and the fractions in h->iact_tau: cosines,
// trunk, embedding, Dense_0 partials, head (iqn_act_kernels.h).  Row groups of Dense_0: NRG * NP = 512, i.e. 1 MB of
// partials for J = 512 (6 % of the Dense_0 kernel they come from) -- the head's single CU has to read them all -- over
// NRG * J / 32 workgroups of 8 waves (256 for N <= 32, 128 for N <= 64).
static int iqn_act_chain(idqn_handle_t h, int32_t which, int32_t head, float* q_out_dev, hipStream_t q) {
    const float* params = (which ? h->target : h->online) + (long)head * h->L.head_stride;
    const int N = h->iqn.N, MT = N > 32 ? 2 : 1, NP = 32 * MT, NRG = 512 / NP;
    IqnActCosArgs ca;
    ca.tau = h->iact_tau; ca.cosv = h->iact_cos;
    hipLaunchKernelGGL(k_iqn_act_cos, dim3((unsigned)N), dim3(64), 0, q, ca);
    int rc = act_trunk(h, params, h->act_state, q);
    if (rc) return rc;
    IqnActEmbedArgs ea;
    ea.cosv = h->iact_cos; ea.psi = h->act_a[2]; ea.params = params; ea.x = h->iact_x; ea.we_off = h->iqn.off_we;
    ea.be_off = h->iqn.off_be; ea.F = h->F; ea.N = N; ea.NP = NP;
    hipLaunchKernelGGL(k_iqn_act_embed, dim3((unsigned)cdiv(h->F, 64), (unsigned)MT), dim3(256), 0, q, ea);
    IqnActDenseArgs d;
    d.x = h->iact_x; d.params = params; d.part = h->iact_part; d.w_off = h->off_w0; d.F = h->F; d.J = h->J; d.NP = NP; d.NRG = NRG;
    const dim3 dgrid((unsigned)(NRG * (h->J / 32)));
    if (MT == 1) hipLaunchKernelGGL(k_iqn_act_dense0<1>, dgrid, dim3(512), 0, q, d);
    else hipLaunchKernelGGL(k_iqn_act_dense0<2>, dgrid, dim3(512), 0, q, d);
    IqnActHeadArgs ha;
    ha.part = h->iact_part; ha.params = params; ha.b0_off = h->off_b0; ha.w1_off = h->off_w1; ha.b1_off = h->off_b1;
    ha.NRG = NRG; ha.J = h->J; ha.A = h->cfg.n_actions; ha.N = N; ha.NP = NP; ha.q_out = q_out_dev; ha.action = h->act_action;
    ha.mail = h->act_use_mail ? h->act_mail_dev : nullptr; ha.seq = h->act_seq;
    if (MT == 1) hipLaunchKernelGGL(k_iqn_act_head<1>, dim3(1), dim3(1024), 0, q, ha);
    else hipLaunchKernelGGL(k_iqn_act_head<2>, dim3(1), dim3(1024), 0, q, ha);
    IDQN_HIP_CHECK(hipGetLastError());
    return IDQN_OK;
}

// select_action's greedy branch for ONE state that lives on the host (slimdqn/sample_collection/utils.py:8-21: the
// reference uploads the state, runs best_action and blocks on `.item()`): upload from pinned memory, the five launches of
// the single-state path, the action back into pinned memory, one stream synchronisation -- replayed as ONE hipGraph per
// (net, buffers) after the first call (seven eager API calls cost more host time than the ~35 us of GPU work).
static int act_host_wait(idqn_handle_t h, int32_t* action_host_pinned, hipStream_t q);
// wait = false: the launch only (idqn_act_host_begin); the result is collected by act_host_wait (idqn_act_host_end)
// tau_host_pinned != nullptr: the i-IQN chain on that many fractions (idqn_iqn_act_host; its entry checked the arguments)
static int act_host_impl(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned, float* q_out_dev,
                         int32_t* action_host_pinned, void* stream, bool wait, const float* tau_host_pinned = nullptr) {
    IDQN_REQUIRE(h && state_host_pinned && q_out_dev && action_host_pinned, "idqn_act_host: null pointer");
    IDQN_REQUIRE(head >= 0 && head < h->cfg.n_heads && (which == 0 || which == 1), "idqn_act_host: bad head / which");
    const bool iqn = tau_host_pinned != nullptr;
    hipStream_t q = (hipStream_t)stream;
    const bool cnn = h->cfg.arch == IDQN_ARCH_CNN || h->imp.on;  // (pixel input)
    // bytes of one state: uint8 pixels (cnn, impala) or float32 features (fc)
    const size_t E = cnn ? (size_t)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c : (size_t)h->fc.d[0] * 4;
    if (!h->act_state) {  // (fc handles: a few floats)
        IDQN_HIP_CHECK(hipMalloc((void**)&h->act_state, E + 64));
        h->owned.push_back((void*)h->act_state);
        IDQN_HIP_CHECK(hipMalloc((void**)&h->act_action, 64));
        h->owned.push_back((void*)h->act_action);
    }
    // The single-state path ends in a kernel that can write the action straight into mapped host memory, followed by a
    // sequence number the host polls (IDQN_ACT_POLL=0: a device-to-host copy and a stream synchronisation instead).
    // (the i-IQN chain always ends in k_iqn_act_head, which writes the mailbox: it never takes the generic route, so
    // IDQN_ACT_GENERIC has no say in it)
    const bool poll = !act_no_poll() && (iqn || ((cnn && !h->gc.on && !h->imp.on) ? (!act_generic() && h->J <= 512 && h->cfg.n_actions <= 32) : true));
    if (iqn && !h->iact_tau) {
        const long NP = h->iqn.N > 32 ? 64 : 32;
        float* p = nullptr;
        IDQN_HIP_CHECK(hipMalloc((void**)&p, (size_t)(64 + 64 * IQN_ACT_EMBED + (long)h->F * NP + 512L * h->J) * 4));
        h->owned.push_back((void*)p);
        h->iact_tau = p; h->iact_cos = p + 64; h->iact_x = h->iact_cos + 64 * IQN_ACT_EMBED; h->iact_part = h->iact_x + (long)h->F * NP;
    }
    if (poll && !h->act_mail) {
        IDQN_HIP_CHECK(hipHostMalloc((void**)&h->act_mail, 64, hipHostMallocMapped | hipHostMallocCoherent));
        memset(h->act_mail, 0, 64);
        IDQN_HIP_CHECK(hipHostGetDevicePointer((void**)&h->act_mail_dev, h->act_mail, 0));
        IDQN_HIP_CHECK(hipMalloc((void**)&h->act_seq, 4));
        IDQN_HIP_CHECK(hipMemset(h->act_seq, 0, 4));
        IDQN_HIP_CHECK(hipStreamSynchronize(nullptr));  // (the memset runs on the null stream, which does not order against qs)
        h->owned.push_back((void*)h->act_seq);
    }
    // The MLP's state is a few floats: the kernel reads them from the caller's pinned buffer itself (one copy node fewer in front of a
    // 3 us kernel); pixels are read many times over by the first conv layer and are copied to HBM first.
    const void* direct = nullptr;
    if (!cnn && E <= 256) {
        void* dptr = nullptr;
        if (hipHostGetDevicePointer(&dptr, const_cast<void*>(state_host_pinned), 0) == hipSuccess) direct = dptr;
        else (void)hipGetLastError();
    }
    auto issue = [&](hipStream_t qs) -> int {
        if (!direct) IDQN_HIP_CHECK(hipMemcpyAsync(h->act_state, state_host_pinned, E, hipMemcpyHostToDevice, qs));
        if (iqn) IDQN_HIP_CHECK(hipMemcpyAsync(h->iact_tau, tau_host_pinned, (size_t)h->iqn.N * 4, hipMemcpyHostToDevice, qs));
        h->act_use_mail = poll;
        int rc = iqn ? iqn_act_chain(h, which, head, q_out_dev, qs)
                     : q_values_impl(h, which, head, direct ? direct : (const void*)h->act_state, 1, q_out_dev, h->act_action, (void*)qs);
        h->act_use_mail = false;
        if (rc) return rc;
        if (!poll) IDQN_HIP_CHECK(hipMemcpyAsync(action_host_pinned, h->act_action, 4, hipMemcpyDeviceToHost, qs));
        return IDQN_OK;
    };
    int rc = IDQN_OK;
    if (act_use_graph()) {
        const int net = which * h->cfg.n_heads + head;
        hipGraphExec_t exec = nullptr;
        if (iqn) {
            auto key = std::make_tuple(net, state_host_pinned, (const void*)tau_host_pinned, (void*)q_out_dev, (void*)action_host_pinned);
            auto it = h->iact_graphs.find(key);
            if (it == h->iact_graphs.end()) {
                if ((rc = capture_exec(h, issue, &exec))) return rc;
                it = h->iact_graphs.emplace(key, exec).first;
            }
            exec = it->second;
        } else {
            auto key = std::make_tuple(net, state_host_pinned, (void*)q_out_dev, (void*)action_host_pinned);
            auto it = h->act_graphs.find(key);
            if (it == h->act_graphs.end()) {
                if ((rc = capture_exec(h, issue, &exec))) return rc;
                it = h->act_graphs.emplace(key, exec).first;
            }
            exec = it->second;
        }
        IDQN_HIP_CHECK(hipGraphLaunch(exec, q));
    } else {
        rc = issue(q);
        if (rc) return rc;
    }
    h->act_pending = poll ? 1 : 2;  // 1: the mailbox announces the action; 2: a device-to-host copy is queued, synchronise
    if (!wait) return IDQN_OK;
    return act_host_wait(h, action_host_pinned, q);
}

// The host side of an acting mailbox: spins until mail[seq_index] shows the sequence number `want` -- far longer than any step
// queued in front of the launch takes -- and asks every 2^20 spins whether q ran dry (or failed) without the number, reading
// once more if so.  false: the launch finished without delivering.
static bool mailbox_wait(volatile int32_t* mail, int seq_index, unsigned want, hipStream_t q) {
    for (long spin = 0; spin < (1L << 34); ++spin) {
        if ((unsigned)mail[seq_index] == want) return true;
        __builtin_ia32_pause();
        if ((spin & 0xfffff) == 0xfffff && hipStreamQuery(q) != hipErrorNotReady) return (unsigned)mail[seq_index] == want;
    }
    return false;
}

static int act_host_wait(idqn_handle_t h, int32_t* action_host_pinned, hipStream_t q) {
    IDQN_REQUIRE(h->act_pending != 0, "idqn_act_host_end: no acting launch is pending");
    const bool poll = h->act_pending == 1;
    h->act_pending = 0;
    if (poll) {
        volatile int32_t* mail = h->act_mail;
        if (!mailbox_wait(mail, 1, ++h->act_expected, q)) {  // resynchronise the two counters, then report
            IDQN_HIP_CHECK(hipStreamSynchronize(q));
            IDQN_HIP_CHECK(hipMemcpy(&h->act_expected, h->act_seq, 4, hipMemcpyDeviceToHost));
            IDQN_REQUIRE(false, "idqn_act_host: the acting launch finished without delivering its action");
        }
        *action_host_pinned = mail[0];
        return IDQN_OK;
    }
    IDQN_HIP_CHECK(hipStreamSynchronize(q));
    return IDQN_OK;
}

extern "C" int idqn_act_host(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned, float* q_out_dev,
                             int32_t* action_host_pinned, void* stream) {
    IDQN_REQUIRE(h && h->act_pending == 0, "idqn_act_host: null handle, or an idqn_act_host_begin is still waiting for its _end");
    return act_host_impl(h, which, head, state_host_pinned, q_out_dev, action_host_pinned, stream, true);
}
extern "C" int idqn_act_host_begin(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned, float* q_out_dev,
                                   int32_t* action_host_pinned, void* stream) {
    IDQN_REQUIRE(h && h->act_pending == 0, "idqn_act_host_begin: null handle, or an acting launch is already pending");
    return act_host_impl(h, which, head, state_host_pinned, q_out_dev, action_host_pinned, stream, false);
}
// argument checks of the two i-IQN entries, under their own names: everything is refused before anything is enqueued (the
// same tests at the head of act_host_impl then cannot fire for them).  The last clause is an invariant, not a case: idqn_create
// accepts quantile heads only on shapes the MFMA path is built for, all of which satisfy it.
static int iqn_act_check(idqn_handle_t h, const char* fn, int32_t which, int32_t head, const void* state_host_pinned,
                         const float* tau_host_pinned, float* q_out_dev, int32_t* action_host_pinned) {
    IDQN_REQUIRE(h && state_host_pinned && tau_host_pinned && q_out_dev && action_host_pinned, "%s: null pointer", fn);
    IDQN_REFUSE_IMPALA(h, fn);
    IDQN_REQUIRE(h->iqn.N > 0, "%s: the handle was created without quantile heads (cfg.n_quantiles)", fn);
    IDQN_REQUIRE(head >= 0 && head < h->cfg.n_heads && (which == 0 || which == 1), "%s: bad head / which", fn);
    IDQN_REQUIRE(h->act_pending == 0, "%s: an acting launch is already pending (idqn_act_host_end collects it)", fn);
    IDQN_REQUIRE(h->F % 2 == 0 && h->J % 32 == 0 && h->J <= 512 && h->cfg.n_actions <= 32 && h->iqn.N <= 64,
                 "%s: the single-state kernels take even F, J = 32 m <= 512, <= 32 actions, <= 64 fractions", fn);
    return IDQN_OK;
}
extern "C" int idqn_iqn_act_host(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned,
                                 const float* tau_host_pinned, float* q_out_dev, int32_t* action_host_pinned, void* stream) {
    int rc = iqn_act_check(h, "idqn_iqn_act_host", which, head, state_host_pinned, tau_host_pinned, q_out_dev, action_host_pinned);
    if (rc) return rc;
    return act_host_impl(h, which, head, state_host_pinned, q_out_dev, action_host_pinned, stream, true, tau_host_pinned);
}
extern "C" int idqn_iqn_act_host_begin(idqn_handle_t h, int32_t which, int32_t head, const void* state_host_pinned,
                                       const float* tau_host_pinned, float* q_out_dev, int32_t* action_host_pinned, void* stream) {
    int rc = iqn_act_check(h, "idqn_iqn_act_host_begin", which, head, state_host_pinned, tau_host_pinned, q_out_dev, action_host_pinned);
    if (rc) return rc;
    return act_host_impl(h, which, head, state_host_pinned, q_out_dev, action_host_pinned, stream, false, tau_host_pinned);
}
extern "C" int idqn_act_host_end(idqn_handle_t h, int32_t* action_host_pinned, void* stream) {
    IDQN_REQUIRE(h && action_host_pinned, "idqn_act_host_end: null pointer");
    return act_host_wait(h, action_host_pinned, (hipStream_t)stream);
}

// Acting for n <= 32 host states in one call: idqn_act_host_many (MFMA cnn handles), idqn_act_host_many_fc (MLP and
// general-shape cnn handles) and idqn_iqn_act_host_many (quantile heads).  The states are copied behind a head (the head /
// group table; for i-IQN the fractions too) in the handle's pinned block, ONE copy node uploads the block, the entry's
// launches follow, and the n actions come back through the slot's mailbox.  One linear hipGraph per (n, buffers) serves every
// head assignment, both parameter sets and every set of fractions.  Each entry checks its own arguments and domain, fills the
// block and hands its launches to act_many_run; everything else is shared.
static int act_many_conv_plan(idqn_handle_t h, int i, int* KS, int* upt, const char* fn = "idqn_act_host_many") {
    const ConvL& l = h->conv[i];
    *KS = i == 0 ? 8 : 16;  // as act_trunk
    const int units = l.K * l.K * (l.CI % 32 == 0 ? l.CI / 32 : l.CI / 4);
    *upt = cdiv(units, *KS);
    IDQN_REQUIRE(l.CI % 32 == 0 ? *upt <= 4 : (l.CI == 4 && *upt <= 8), "%s: Conv_%d is outside the acting kernels' shapes", fn, i);
    return IDQN_OK;
}
static int act_many_conv_plans(idqn_handle_t h, const char* fn = "idqn_act_host_many") {  // the entries' check, before anything is enqueued
    for (int i = 0; i < 3; ++i) {
        int ks = 0, upt = 0;
        int rc = act_many_conv_plan(h, i, &ks, &upt, fn);
        if (rc) return rc;
    }
    return IDQN_OK;
}

// The slot of the handle's entry, on its first call: the pinned block and its device copy for a head of head_bytes and 32
// states, ONE float workspace of floats[0 .. n_floats) carved in that order into a[0], a[1], a[2], (n_floats == 6: cos, x,)
// part, action[32] plus the two counters, and the mapped mailbox.  Everything goes into locals first: a failure part-way
// frees what it got and leaves every field of the slot null.
static int act_many_alloc(ActManySlot& s, std::vector<void*>& owned, size_t head_bytes, size_t state_bytes, const long* floats, int n_floats) {
    const size_t block = head_bytes + ACT_MANY_MAX * state_bytes + 64;
    long total = 0;
    for (int i = 0; i < n_floats; ++i) total += floats[i];
    uint8_t *pin = nullptr, *dev = nullptr;
    float* f = nullptr;
    int32_t *act = nullptr, *mail = nullptr, *mail_dev = nullptr;
    auto alloc = [&]() -> int {
        IDQN_HIP_CHECK(hipHostMalloc((void**)&pin, block, hipHostMallocDefault));
        IDQN_HIP_CHECK(hipHostMalloc((void**)&mail, 256, hipHostMallocMapped | hipHostMallocCoherent));
        memset(mail, 0, 256);
        IDQN_HIP_CHECK(hipHostGetDevicePointer((void**)&mail_dev, mail, 0));
        IDQN_HIP_CHECK(hipMalloc((void**)&f, (size_t)total * 4));
        IDQN_HIP_CHECK(hipMalloc((void**)&act, 256));  // actions [32], then the two counters
        IDQN_HIP_CHECK(hipMemset(act, 0, 256));
        IDQN_HIP_CHECK(hipMalloc((void**)&dev, block));
        IDQN_HIP_CHECK(hipStreamSynchronize(nullptr));  // (the memset runs on the null stream, which does not order against q)
        return IDQN_OK;
    };
    if (const int rc = alloc()) {
        if (pin) (void)hipHostFree(pin);
        if (mail) (void)hipHostFree(mail);
        if (f) (void)hipFree(f);
        if (act) (void)hipFree(act);
        if (dev) (void)hipFree(dev);
        return rc;
    }
    owned.push_back((void*)f);
    owned.push_back((void*)act);
    owned.push_back((void*)dev);
    s.pin = pin; s.head_bytes = head_bytes; s.mail = mail; s.mail_dev = mail_dev; s.ws = f;
    float* sub[6];
    for (int i = 0; i < n_floats; ++i) { sub[i] = f; f += floats[i]; }
    s.a[0] = sub[0]; s.a[1] = sub[1]; s.a[2] = sub[2]; s.part = sub[n_floats - 1];
    if (n_floats == 6) { s.cos = sub[3]; s.x = sub[4]; }
    s.action = act; s.ctr = (unsigned*)(act + ACT_MANY_MAX);
    s.block = dev;
    return IDQN_OK;
}
static int act_many_alloc(idqn_handle_t h, size_t head_bytes, size_t state_bytes, const long* floats, int n_floats) {
    return act_many_alloc(h->many, h->owned, head_bytes, state_bytes, floats, n_floats);
}

// grouped: the states sorted into groups by head, in state order within a group (the Dense_0 kernels of the cnn and i-IQN
// chains walk them); otherwise n, which and head[] only -- every state is a workgroup of its own
static void act_many_fill_table(ActManyTable* tb, int which, const int32_t* heads, int n, int K, bool grouped) {
    tb->n = n; tb->which = which; tb->pad = 0;
    int ng = 0, pos = 0;
    for (int k = 0; grouped && k < K && pos < n; ++k) {
        const int start = pos;
        for (int e = 0; e < n; ++e)
            if (heads[e] == k) tb->order[pos++] = e;
        if (pos > start) { tb->g_head[ng] = k; tb->g_start[ng] = start; tb->g_count[ng] = pos - start; ++ng; }
    }
    tb->n_groups = ng;
    for (int e = 0; e < n; ++e) tb->head[e] = heads[e];
}

static ActManyNets act_many_nets(idqn_handle_t h) {  // (an IqnActManyBlock begins with its table)
    ActManyNets nets;
    nets.tab = (const ActManyTable*)h->many.block; nets.online = h->online; nets.target = h->target; nets.pstride = h->L.head_stride;
    return nets;
}

// the three conv launches of the cnn and i-IQN chains (k_act_many_conv) and of an acting group (k_act_group_conv: the same body,
// the parameter bases from the group's table): uint8 states [n][..] -> out[0] -> out[1] -> out[2]
template <int CIU, int UPT>
static void act_many_conv_launch(const ActManyConvArgs& a, dim3 grid, hipStream_t q) {
    hipLaunchKernelGGL((k_act_many_conv<CIU, UPT>), grid, dim3(256), 0, q, a);
}
template <int CIU, int UPT>
static void act_many_conv_launch(const ActGroupConvArgs& a, dim3 grid, hipStream_t q) {
    hipLaunchKernelGGL((k_act_group_conv<CIU, UPT>), grid, dim3(256), 0, q, a);
}
template <class Nets>
static int act_many_convs(idqn_handle_t h, const Nets& nets, const uint8_t* states_u8, float* const out[3], int n, hipStream_t q) {
    const float* in = nullptr;
    int ih = h->cfg.obs_h, iw = h->cfg.obs_w;
    for (int i = 0; i < 3; ++i) {
        const ConvL& l = h->conv[i];
        ActManyConvArgsT<Nets> a;
        a.nets = nets; a.in_u8 = i == 0 ? states_u8 : nullptr; a.in = in; a.out = out[i];
        a.w_off = l.w_off; a.b_off = l.b_off; a.IH = ih; a.IW = iw; a.CI = l.CI; a.OH = l.OH; a.OW = l.OW; a.CO = l.CO;
        a.K = l.K; a.S = l.S; a.PLh = l.PLh; a.PLw = l.PLw;
        int upt = 0;
        int rc = act_many_conv_plan(h, i, &a.KS, &upt);
        if (rc) return rc;
        const dim3 grid(cdiv((long)l.OH * l.OW * l.CO, 256 / a.KS), n);
        if (l.CI % 32 != 0) act_many_conv_launch<4, 8>(a, grid, q);
        else if (upt <= 1) act_many_conv_launch<32, 1>(a, grid, q);
        else if (upt <= 2) act_many_conv_launch<32, 2>(a, grid, q);
        else act_many_conv_launch<32, 4>(a, grid, q);
        in = out[i]; ih = l.OH; iw = l.OW;
    }
    return IDQN_OK;
}

// What the three entries do once the block is filled: the copy node that uploads head and n states, chain(stream, mail) --
// the entry's launches, whose last kernel delivers to `mail` unless it is null -- as a replayed graph per (n, buffers) or
// eagerly (IDQN_ACT_GRAPH=0), then the wait on the slot's mailbox (IDQN_ACT_POLL=0: a device-to-host copy of the actions and a
// stream synchronisation instead) and the n actions into the caller's buffer.  `s` is the handle's slot, or a group's own
// (idqn_group_act_host_fc), which captures on the stream of the handle it passes.
template <class Chain>
static int act_many_run(idqn_handle_t h, ActManySlot& s, const char* fn_name, int n, size_t state_bytes, float* q_out_dev,
                        int32_t* actions_host_pinned, hipStream_t q, Chain&& chain) {
    const bool poll = !act_no_poll();
    auto issue = [&](hipStream_t qs) -> int {
        IDQN_HIP_CHECK(hipMemcpyAsync(s.block, s.pin, s.head_bytes + (size_t)n * state_bytes, hipMemcpyHostToDevice, qs));
        const int rc = chain(qs, poll ? s.mail_dev : nullptr);
        if (rc) return rc;
        IDQN_HIP_CHECK(hipGetLastError());
        if (!poll) IDQN_HIP_CHECK(hipMemcpyAsync(actions_host_pinned, s.action, (size_t)n * 4, hipMemcpyDeviceToHost, qs));
        return IDQN_OK;
    };
    int rc = IDQN_OK;
    if (act_use_graph()) {
        auto key = std::make_tuple(n, (void*)q_out_dev, (void*)actions_host_pinned);
        auto it = s.graphs.find(key);
        if (it == s.graphs.end()) {
            hipGraphExec_t exec = nullptr;
            if ((rc = capture_exec(h, issue, &exec))) return rc;
            it = s.graphs.emplace(key, exec).first;
        }
        IDQN_HIP_CHECK(hipGraphLaunch(it->second, q));
    } else if ((rc = issue(q))) {
        return rc;
    }
    if (!poll) {
        IDQN_HIP_CHECK(hipStreamSynchronize(q));
        return IDQN_OK;
    }
    volatile int32_t* mail = s.mail;
    if (!mailbox_wait(mail, ACT_MANY_MAX, ++s.expected, q)) {  // resynchronise the counters, then report
        IDQN_HIP_CHECK(hipStreamSynchronize(q));
        IDQN_HIP_CHECK(hipMemcpy(&s.expected, s.ctr, 4, hipMemcpyDeviceToHost));
        IDQN_HIP_CHECK(hipMemset(s.ctr + 1, 0, 4));
        IDQN_REQUIRE(false, "%s: the acting launch finished without delivering its actions", fn_name);
    }
    for (int e = 0; e < n; ++e) actions_host_pinned[e] = mail[e];
    return IDQN_OK;
}
template <class Chain>
static int act_many_run(idqn_handle_t h, const char* fn_name, int n, size_t state_bytes, float* q_out_dev, int32_t* actions_host_pinned,
                        hipStream_t q, Chain&& chain) {
    return act_many_run(h, h->many, fn_name, n, state_bytes, q_out_dev, actions_host_pinned, q, chain);
}

// select_action's greedy branch on the MFMA cnn path (act_many_kernels.h): five launches behind the copy node -- three conv
// layers, Dense_0 per group of states with one head, the head kernel per state.
static int act_many_chain(idqn_handle_t h, int n, float* q_out_dev, int32_t* mail_dev, hipStream_t q) {
    const ActManySlot& s = h->many;
    const ActManyNets nets = act_many_nets(h);
    int rc = act_many_convs(h, nets, s.block + s.head_bytes, s.a, n, q);
    if (rc) return rc;
    ActManyDenseArgs d;
    d.nets = nets; d.a3 = s.a[2]; d.part = s.part; d.w_off = h->off_w0; d.F = h->F; d.J = h->J;
    d.NRG = std::max(1, 256 / (h->J / 128));  // as the single-state path
    hipLaunchKernelGGL(k_act_many_dense0, dim3(d.NRG * (h->J / 128), std::min(n, h->cfg.n_heads)), dim3(256), 0, q, d);
    ActManyHeadArgs ha;
    ha.nets = nets; ha.part = s.part; ha.b0_off = h->off_b0; ha.w1_off = h->off_w1; ha.b1_off = h->off_b1;
    ha.NP = d.NRG; ha.J = h->J; ha.A = h->cfg.n_actions; ha.n = n; ha.q_out = q_out_dev; ha.action = s.action;
    ha.mail = mail_dev; ha.ctr = s.ctr;
    hipLaunchKernelGGL(k_act_many_head, dim3(n), dim3(1024), 0, q, ha);
    return IDQN_OK;
}

extern "C" int idqn_act_host_many(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                                  float* q_out_dev, int32_t* actions_host_pinned, void* stream) {
    IDQN_REQUIRE(h && heads_host && states_host_pinned && q_out_dev && actions_host_pinned, "idqn_act_host_many: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_act_host_many");
    IDQN_REQUIRE(n >= 1 && n <= ACT_MANY_MAX, "idqn_act_host_many: n = %d, must be in [1, %d]", n, ACT_MANY_MAX);
    IDQN_REQUIRE(which == 0 || which == 1, "idqn_act_host_many: which = %d", which);
    const int K = h->cfg.n_heads;
    for (int e = 0; e < n; ++e) IDQN_REQUIRE(heads_host[e] >= 0 && heads_host[e] < K, "idqn_act_host_many: head %d of state %d", heads_host[e], e);
    IDQN_REQUIRE(h->act_pending == 0, "idqn_act_host_many: an idqn_act_host_begin is still waiting for its _end");
    IDQN_REQUIRE(h->iqn.N == 0, "idqn_act_host_many: the handle was created with quantile heads");
    IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_CNN && !h->gc.on && !act_generic() && h->J <= 512 && h->J % 128 == 0 && h->cfg.n_actions <= 32,
                 "idqn_act_host_many: the handle is outside the single-state cnn acting path (fc, general shapes, IDQN_ACT_GENERIC, J > 512, A > 32)");
    int rc = act_many_conv_plans(h);
    if (rc) return rc;
    const size_t sb = (size_t)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c;  // bytes of one state
    IDQN_REQUIRE(sb % 4 == 0, "idqn_act_host_many: %zu bytes per state", sb);
    if (!h->many.block) {
        const long NRG = std::max(1, 256 / (h->J / 128));
        long fl[4] = {0, 0, 0, ACT_MANY_MAX * NRG * h->J};
        for (int i = 0; i < 3; ++i) fl[i] = (long)ACT_MANY_MAX * h->conv[i].OH * h->conv[i].OW * h->conv[i].CO;
        if ((rc = act_many_alloc(h, sizeof(ActManyTable), sb, fl, 4))) return rc;
    }
    act_many_fill_table((ActManyTable*)h->many.pin, which, heads_host, n, K, true);
    memcpy(h->many.pin + sizeof(ActManyTable), states_host_pinned, (size_t)n * sb);
    return act_many_run(h, "idqn_act_host_many", n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream,
                        [&](hipStream_t qs, int32_t* mail_dev) { return act_many_chain(h, n, q_out_dev, mail_dev, qs); });
}

// idqn_act_host_many for the handles it refuses (fc_act_many_kernels.h): MLP handles run ONE launch behind the copy node
// (k_fc_act_many1 when every width fits its LDS rows, as the single-state path picks k_fc_q1; k_fc_act_many otherwise);
// general-shape cnn handles run three k_gconv_fwd_many launches and k_fc_act_many on the flattened features.
static int fc_act_many_chain(idqn_handle_t h, int n, float* q_out_dev, int32_t* mail_dev, hipStream_t q) {
    const ActManySlot& s = h->many;
    const ActManyNets nets = act_many_nets(h);
    const uint8_t* states = s.block + s.head_bytes;
    FcActManyArgs a;
    a.net = h->fc; a.nets = nets; a.s = (const float*)states; a.s_ld = h->fc.d[0]; a.ws = s.part; a.q_out = q_out_dev;
    a.action = s.action; a.mail = mail_dev; a.ctr = s.ctr; a.n = n;
    if (h->gc.on) {
        for (int i = 0; i < 3; ++i) {
            const ConvL& l = h->conv[i];
            GConvManyArgs g;
            g.nets = nets; g.in_u8 = i == 0 ? states : nullptr; g.in = i == 0 ? nullptr : s.a[i - 1]; g.out = s.a[i];
            g.w_off = l.w_off; g.b_off = l.b_off; g.IH = l.IH; g.IW = l.IW; g.CI = l.CI; g.OH = l.OH; g.OW = l.OW; g.CO = l.CO;
            g.KS = l.K; g.S = l.S; g.PLh = l.PLh; g.PLw = l.PLw;
            hipLaunchKernelGGL(k_gconv_fwd_many, dim3(ggrid((long)l.OH * l.OW * l.CO), n), dim3(256), 0, q, g);
        }
        a.s = s.a[2];  // row stride = flattened feature count = d[0]
        hipLaunchKernelGGL(k_fc_act_many, dim3(n), dim3(256), 0, q, a);
    } else if (h->fc.dmax <= FC_MAX_WIDTH) {
        hipLaunchKernelGGL(k_fc_act_many1, dim3(n), dim3(512), 0, q, a);
    } else {
        hipLaunchKernelGGL(k_fc_act_many, dim3(n), dim3(256), 0, q, a);
    }
    return IDQN_OK;
}

extern "C" int idqn_act_host_many_fc(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                                     float* q_out_dev, int32_t* actions_host_pinned, void* stream) {
    IDQN_REQUIRE(h && heads_host && states_host_pinned && q_out_dev && actions_host_pinned, "idqn_act_host_many_fc: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_act_host_many_fc");
    IDQN_REQUIRE(n >= 1 && n <= ACT_MANY_MAX, "idqn_act_host_many_fc: n = %d, must be in [1, %d]", n, ACT_MANY_MAX);
    IDQN_REQUIRE(which == 0 || which == 1, "idqn_act_host_many_fc: which = %d", which);
    const int K = h->cfg.n_heads;
    for (int e = 0; e < n; ++e) IDQN_REQUIRE(heads_host[e] >= 0 && heads_host[e] < K, "idqn_act_host_many_fc: head %d of state %d", heads_host[e], e);
    IDQN_REQUIRE(h->act_pending == 0, "idqn_act_host_many_fc: an idqn_act_host_begin is still waiting for its _end");
    IDQN_REQUIRE(h->iqn.N == 0, "idqn_act_host_many_fc: the handle was created with quantile heads");
    const bool cnn = h->cfg.arch == IDQN_ARCH_CNN;
    IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_FC || (cnn && h->gc.on),
                 "idqn_act_host_many_fc: the handle runs the MFMA cnn path (idqn_act_host_many serves it)");
    // bytes of one state: uint8 pixels (general-shape cnn) or float32 features (fc)
    const size_t sb = cnn ? (size_t)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c : (size_t)h->fc.d[0] * 4;
    if (!h->many.block) {
        long fl[4] = {0, 0, 0, (long)ACT_MANY_MAX * 2 * h->fc.dmax};
        if (cnn)
            for (int i = 0; i < 3; ++i) fl[i] = (long)ACT_MANY_MAX * h->conv[i].OH * h->conv[i].OW * h->conv[i].CO;
        if (const int rc = act_many_alloc(h, sizeof(ActManyTable), sb, fl, 4)) return rc;
    }
    act_many_fill_table((ActManyTable*)h->many.pin, which, heads_host, n, K, false);
    memcpy(h->many.pin + sizeof(ActManyTable), states_host_pinned, (size_t)n * sb);
    return act_many_run(h, "idqn_act_host_many_fc", n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream,
                        [&](hipStream_t qs, int32_t* mail_dev) { return fc_act_many_chain(h, n, q_out_dev, mail_dev, qs); });
}

// The i-IQN acting rule, N fractions per state (iqn_act_many_kernels.h): seven launches behind the copy node -- three conv
// layers, cosines, embedding, Dense_0 per group of states with one head, the head kernel per state.  NRG as iqn_act_chain.
static int iqn_act_many_chain(idqn_handle_t h, int n, float* q_out_dev, int32_t* mail_dev, hipStream_t q) {
    const ActManySlot& s = h->many;
    const IqnActManyBlock* blk = (const IqnActManyBlock*)s.block;
    const ActManyNets nets = act_many_nets(h);
    int rc = act_many_convs(h, nets, s.block + s.head_bytes, s.a, n, q);
    if (rc) return rc;
    const int N = h->iqn.N, MT = N > 32 ? 2 : 1, NP = 32 * MT, NRG = 512 / NP;
    IqnActManyCosArgs ca;
    ca.tau = &blk->tau[0][0]; ca.cosv = s.cos;
    hipLaunchKernelGGL(k_iqn_act_many_cos, dim3((unsigned)N, (unsigned)n), dim3(64), 0, q, ca);
    IqnActManyEmbedArgs ea;
    ea.nets = nets; ea.cosv = s.cos; ea.psi = s.a[2]; ea.x = s.x; ea.we_off = h->iqn.off_we;
    ea.be_off = h->iqn.off_be; ea.F = h->F; ea.N = N; ea.NP = NP;
    hipLaunchKernelGGL(k_iqn_act_many_embed, dim3((unsigned)cdiv(h->F, 64), (unsigned)MT, (unsigned)n), dim3(256), 0, q, ea);
    IqnActManyDenseArgs d;
    d.nets = nets; d.x = s.x; d.part = s.part; d.w_off = h->off_w0; d.F = h->F; d.J = h->J; d.NP = NP; d.NRG = NRG;
    const dim3 dgrid((unsigned)(NRG * (h->J / 32)), (unsigned)std::min(n, h->cfg.n_heads));
    if (MT == 1) hipLaunchKernelGGL(k_iqn_act_many_dense0<1>, dgrid, dim3(512), 0, q, d);
    else hipLaunchKernelGGL(k_iqn_act_many_dense0<2>, dgrid, dim3(512), 0, q, d);
    IqnActManyHeadArgs ha;
    ha.nets = nets; ha.part = s.part; ha.b0_off = h->off_b0; ha.w1_off = h->off_w1; ha.b1_off = h->off_b1;
    ha.NRG = NRG; ha.J = h->J; ha.A = h->cfg.n_actions; ha.N = N; ha.NP = NP; ha.n = n; ha.q_out = q_out_dev;
    ha.action = s.action; ha.mail = mail_dev; ha.ctr = s.ctr;
    if (MT == 1) hipLaunchKernelGGL(k_iqn_act_many_head<1>, dim3(n), dim3(1024), 0, q, ha);
    else hipLaunchKernelGGL(k_iqn_act_many_head<2>, dim3(n), dim3(1024), 0, q, ha);
    return IDQN_OK;
}

extern "C" int idqn_iqn_act_host_many(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned,
                                      const float* taus_host_pinned, int32_t n, float* q_out_dev, int32_t* actions_host_pinned,
                                      void* stream) {
    IDQN_REQUIRE(h && heads_host && states_host_pinned && taus_host_pinned && q_out_dev && actions_host_pinned,
                 "idqn_iqn_act_host_many: null pointer");
    IDQN_REFUSE_IMPALA(h, "idqn_iqn_act_host_many");
    IDQN_REQUIRE(n >= 1 && n <= ACT_MANY_MAX, "idqn_iqn_act_host_many: n = %d, must be in [1, %d]", n, ACT_MANY_MAX);
    IDQN_REQUIRE(which == 0 || which == 1, "idqn_iqn_act_host_many: which = %d", which);
    IDQN_REQUIRE(h->iqn.N > 0, "idqn_iqn_act_host_many: the handle was created without quantile heads (cfg.n_quantiles)");
    const int K = h->cfg.n_heads, N = h->iqn.N;
    for (int e = 0; e < n; ++e) IDQN_REQUIRE(heads_host[e] >= 0 && heads_host[e] < K, "idqn_iqn_act_host_many: head %d of state %d", heads_host[e], e);
    IDQN_REQUIRE(h->act_pending == 0, "idqn_iqn_act_host_many: an acting launch is still pending (idqn_act_host_end collects it)");
    IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_CNN && !h->gc.on && h->F % 2 == 0 && h->J % 32 == 0 && h->J <= 512 &&
                     h->cfg.n_actions <= 32 && N <= 64,
                 "idqn_iqn_act_host_many: the single-state kernels take even F, J = 32 m <= 512, <= 32 actions, <= 64 fractions");
    int rc = act_many_conv_plans(h);
    if (rc) return rc;
    const size_t sb = (size_t)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c;  // bytes of one state
    IDQN_REQUIRE(sb % 4 == 0, "idqn_iqn_act_host_many: %zu bytes per state", sb);
    if (!h->many.block) {
        const long NP = N > 32 ? 64 : 32;
        long fl[6] = {0, 0, 0, (long)ACT_MANY_MAX * 64 * IQN_ACT_EMBED, (long)ACT_MANY_MAX * h->F * NP, (long)ACT_MANY_MAX * 512 * h->J};
        for (int i = 0; i < 3; ++i) fl[i] = (long)ACT_MANY_MAX * h->conv[i].OH * h->conv[i].OW * h->conv[i].CO;
        if ((rc = act_many_alloc(h, sizeof(IqnActManyBlock), sb, fl, 6))) return rc;
    }
    IqnActManyBlock* blk = (IqnActManyBlock*)h->many.pin;  // the table, the fractions, the states
    act_many_fill_table(&blk->tab, which, heads_host, n, K, true);
    for (int e = 0; e < n; ++e) memcpy(blk->tau[e], taus_host_pinned + (size_t)e * N, (size_t)N * 4);
    memcpy(h->many.pin + sizeof(IqnActManyBlock), states_host_pinned, (size_t)n * sb);
    return act_many_run(h, "idqn_iqn_act_host_many", n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream,
                        [&](hipStream_t qs, int32_t* mail_dev) { return iqn_act_many_chain(h, n, q_out_dev, mail_dev, qs); });
}

// select_action's greedy branch on an impala handle (imp_act_many_kernels.h): behind the copy node, the one-workgroup launch
// that resolves the n parameter bases from the uploaded table, the trunk's launches on n nets of one image each in the acting
// workspace, Dense_0 per group of states with one head (a head with a hidden layer), the tail per state.
static int imp_act_many_chain(idqn_handle_t h, int n, float* q_out_dev, int32_t* mail_dev, hipStream_t q) {
    const ActManySlot& s = h->many;
    const ActManyNets nets = act_many_nets(h);
    const uint8_t* states = s.block + s.head_bytes;
    ImpActManyBasesArgs ba;
    ba.nets = nets; ba.wbase = (const float**)s.a[0];
    hipLaunchKernelGGL(k_imp_act_many_bases, dim3(1), dim3(64), 0, q, ba);
    int rc = impala_trunk(h, (const float* const*)s.a[0], n, n, 1, states, states, h->imp.infer, q, true);
    if (rc) return rc;
    ImpActManyTailArgs t;
    memset(&t, 0, sizeof(t));
    t.f.net = h->fc; t.f.nets = nets; t.f.s = h->imp.infer.x[2][2]; t.f.s_ld = h->F; t.f.ws = h->imp.inf_ws; t.f.q_out = q_out_dev;
    t.f.action = s.action; t.f.mail = mail_dev; t.f.ctr = s.ctr; t.f.n = n;
    if (h->imp.d0_split) {
        const imp_act_many_d0_plan_t pl = imp_act_many_d0_plan(h->F, h->fc.d[1]);
        ImpActManyD0Args d;
        d.nets = nets; d.x = h->imp.infer.x[2][2]; d.part = s.part; d.w_off = h->fc.w_off[0]; d.F = h->F; d.D = h->fc.d[1]; d.NP = pl.n_pass;
        hipLaunchKernelGGL(k_imp_act_many_d0, dim3((unsigned)pl.col_blocks, (unsigned)pl.ranges, (unsigned)std::min(n, h->cfg.n_heads)), dim3(256),
                           0, q, d);
        t.f.net = h->imp.tail; t.part = s.part; t.b0_off = h->fc.b_off[0]; t.NP = pl.n_pass; t.D = d.D;
    }
    hipLaunchKernelGGL(k_imp_act_many_tail, dim3(n), dim3(256), 0, q, t);
    return IDQN_OK;
}

extern "C" int idqn_act_host_many_impala(idqn_handle_t h, int32_t which, const int32_t* heads_host, const void* states_host_pinned, int32_t n,
                                         float* q_out_dev, int32_t* actions_host_pinned, void* stream) {
    IDQN_REQUIRE(h, "idqn_act_host_many_impala: null pointer");
    IDQN_REQUIRE(h->imp.on, "idqn_act_host_many_impala: serves impala handles only (idqn_act_host_many, idqn_act_host_many_fc and "
                            "idqn_iqn_act_host_many serve the other architectures)");
    const int K = h->cfg.n_heads;
    int at = -1;
    const char* bad = imp_act_many_args_error(n, K, which, heads_host, states_host_pinned, q_out_dev, actions_host_pinned, &at);
    IDQN_REQUIRE(!bad, "idqn_act_host_many_impala: %s (n = %d, which = %d, state %d)", bad, n, which, at);
    IDQN_REQUIRE(h->act_pending == 0, "idqn_act_host_many_impala: an idqn_act_host_begin is still waiting for its _end");
    const size_t sb = (size_t)h->cfg.obs_h * h->cfg.obs_w * h->cfg.obs_c;  // bytes of one state
    if (!h->many.block) {  // the bases' array, nothing, nothing, the Dense_0 pass sums
        long fl[4] = {2 * ACT_MANY_MAX, 0, 0, h->imp.d0_split ? (long)imp_act_many_d0_plan(h->F, h->fc.d[1]).part_floats : 0};
        if (const int rc = act_many_alloc(h, sizeof(ActManyTable), sb, fl, 4)) return rc;
    }
    ActManyTable* tb = (ActManyTable*)h->many.pin;
    act_many_fill_table(tb, which, heads_host, n, K, true);
    bad = imp_act_many_table_error(n, K, heads_host, tb->head, tb->n_groups, tb->order, tb->g_head, tb->g_start, tb->g_count, &at);
    IDQN_REQUIRE(!bad, "idqn_act_host_many_impala: the head table is inconsistent: %s (at %d)", bad, at);
    memcpy(h->many.pin + sizeof(ActManyTable), states_host_pinned, (size_t)n * sb);
    return act_many_run(h, "idqn_act_host_many_impala", n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream,
                        [&](hipStream_t qs, int32_t* mail_dev) { return imp_act_many_chain(h, n, q_out_dev, mail_dev, qs); });
}

extern "C" int idqn_debug_conv_items(const int64_t* p, int32_t n_params, int32_t n_items, void* out_host) {
    IDQN_REQUIRE(p && out_host && n_params == 38 && n_items >= 1, "idqn_debug_conv_items: 38 parameters, at least one item");
    CFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.items_per_slot = (int)p[0]; a.range_major = (int)p[1]; a.nb = (int)p[2]; a.n_var = (int)p[3]; a.in_split = (int)p[4];
    a.S = (int)p[5]; a.row_bytes = (int)p[6]; a.pix_bytes = (int)p[7]; a.in_slot = p[8]; a.wq_stride = p[9];
    IDQN_REQUIRE(a.nb >= 1 && a.n_var >= 1 && a.n_var <= 4, "idqn_debug_conv_items: %d blocks, %d variants", a.nb, a.n_var);
    for (int v = 0; v < 4; ++v) {
        const int64_t* q = p + 10 + 7 * v;
        a.r_begin[v] = (int)q[0]; a.r_cnt[v] = (int)q[1]; a.var[v].OH = (int)q[2]; a.var[v].OW = (int)q[3];
        a.var[v].in_off_h = (int)q[4]; a.var[v].in_off_w = (int)q[5]; a.var[v].w_off = q[6];
        IDQN_REQUIRE(v >= a.n_var || (a.r_cnt[v] >= 1 && a.var[v].OH >= 1 && a.var[v].OW >= 1), "idqn_debug_conv_items: variant %d is empty", v);
    }
    IDQN_REQUIRE(convp_fill_fwd_items(a, n_items, (CFwdDesc*)out_host), "idqn_debug_conv_items: an item does not fit its descriptor");
    return IDQN_OK;
}

extern "C" int idqn_debug_buffer(idqn_handle_t h, const char* name, void** ptr_dev, int64_t* nbytes) {
    IDQN_REQUIRE(h && name && ptr_dev && nbytes, "idqn_debug_buffer: null pointer");
    if (!strcmp(name, "dh") && h->cfg.arch == IDQN_ARCH_CNN && h->dh_nb > 0) {  // placed per batch size (dh_of)
        const int nb = h->dh_nb;
        *ptr_dev = (void*)dh_of(h, nb);
        *nbytes = (int64_t)h->cfg.n_heads * nb * h->J * 32 * 4;
        return IDQN_OK;
    }
    for (auto& e : h->dbg)
        if (e.first == name) {
            *ptr_dev = e.second.first;
            *nbytes = e.second.second;
            return IDQN_OK;
        }
    IDQN_REQUIRE(false, "idqn_debug_buffer: no buffer named '%s'", name);
}

extern "C" int idqn_profile_table(idqn_handle_t h, char* out, int32_t out_bytes) {
    IDQN_REQUIRE(h && out && out_bytes > 0, "idqn_profile_table: null pointer");
    std::vector<std::pair<std::string, std::pair<double, int>>> rows;  // first-seen order
    for (int i = 1; i < h->tl_used; ++i) {
        if (!h->tl_name[i]) continue;  // a step's start marker: nothing was launched before it
        float ms = 0;
        IDQN_HIP_CHECK(hipEventSynchronize(h->tl_ev[i]));
        IDQN_HIP_CHECK(hipEventElapsedTime(&ms, h->tl_ev[i - 1], h->tl_ev[i]));
        size_t r = 0;
        for (; r < rows.size(); ++r)
            if (rows[r].first == h->tl_name[i]) break;
        if (r == rows.size()) rows.push_back({h->tl_name[i], {0.0, 0}});
        rows[r].second.first += ms;
        rows[r].second.second += 1;
    }
    std::string txt;
    char line[160];
    for (auto& r : rows) {
        snprintf(line, sizeof line, "%s\t%.3f\t%d\n", r.first.c_str(), 1e3 * r.second.first / r.second.second, r.second.second);
        txt += line;
    }
    snprintf(out, (size_t)out_bytes, "%s", txt.c_str());
    h->tl_used = 0;
    return IDQN_OK;
}

extern "C" int idqn_profile_read(idqn_handle_t h, double* mean_ms, int32_t* n_launches, char* kernel_name) {
    IDQN_REQUIRE(h && mean_ms && n_launches, "idqn_profile_read: null pointer");
    double total = 0;
    int n = h->ev_used / 2;
    for (int i = 0; i < n; ++i) {
        float ms = 0;
        IDQN_HIP_CHECK(hipEventSynchronize(h->ev[2 * i + 1]));
        IDQN_HIP_CHECK(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
        total += ms;
    }
    *mean_ms = n ? total / n : 0.0;
    *n_launches = n;
    if (kernel_name) snprintf(kernel_name, 64, "%s", h->dominant);
    h->ev_used = 0;
    return IDQN_OK;
}

// ---- seed groups: S independent fc handles learn and act in one launch (fc_group_kernels.h; include/idqn_hip.h) ---------
// A group owns no parameters: the members keep their arenas, and every member may still be driven alone between two group
// calls.  What the group owns: ONE staging ring (staging_ring.h) of per-call blocks -- {FcGroupMember[S], slots}, as
// idqn_learn_steps_on_replay_fc stages its slots, or a prioritized call's records and uniforms (group_per_learn); the four
// learner entries interleave on it, each block behind its own event -- and ONE acting slot of its own.
struct idqn_group_s {
    std::vector<idqn_handle_t> m;
    size_t block_bytes = 0, slots_off = 0;  // a block holds the largest call of any of the four learner entries
    StagingRing ring;
    ActManySlot many;
    std::vector<void*> owned;
};

// Member c of a group (seed or acting) has the shape of member 0
static bool same_member_shape(const idqn_config_t& c, const idqn_config_t& c0, bool with_max_batch) {
    bool same = c.obs_h == c0.obs_h && c.obs_w == c0.obs_w && c.obs_c == c0.obs_c && c.n_features == c0.n_features &&
                c.n_actions == c0.n_actions && c.n_heads == c0.n_heads && (!with_max_batch || c.max_batch == c0.max_batch);
    for (int i = 0; same && i < c.n_features; ++i) same = c.features[i] == c0.features[i];
    return same;
}

extern "C" int idqn_group_create(const idqn_handle_t* members, int32_t n_members, idqn_group_t* out) {
    IDQN_REQUIRE(members && out, "idqn_group_create: null pointer");
    IDQN_REQUIRE(n_members >= 1 && n_members <= ACT_MANY_MAX, "idqn_group_create: %d members, must be in [1, %d]", n_members, ACT_MANY_MAX);
    for (int g = 0; g < n_members; ++g) {
        const idqn_handle_t h = members[g];
        IDQN_REQUIRE(h, "idqn_group_create: member %d is null", g);
        IDQN_REFUSE_IMPALA(h, "idqn_group_create");
        IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_FC && h->cfg.n_quantiles == 0 && h->iqn.N == 0,
                     "idqn_group_create: member %d is not an MLP (fc) handle: groups serve fc handles only", g);
        IDQN_REQUIRE(h->fcp_plan_.floats != 0,
                     "idqn_group_create: member %d is outside the one-launch step (layer widths <= 128, heads of <= %d parameters)", g, 512 * FCP_NPT);
        IDQN_REQUIRE(same_member_shape(h->cfg, members[0]->cfg, true),
                     "idqn_group_create: member %d differs from member 0 in shape (obs, features, n_actions, n_heads, max_batch)", g);
        for (int j = 0; j < g; ++j)
            IDQN_REQUIRE(members[j] != h && members[j]->online != h->online,
                         "idqn_group_create: members %d and %d are the same handle or share an arena: one arena would have two writers", j, g);
    }
    const idqn_handle_t h0 = members[0];
    IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_group_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(h0->fcp_plan_.floats * 4)));
    if (h0->fcs_plan_.floats)
        IDQN_HIP_CHECK(hipFuncSetAttribute((const void*)k_fc_group_steps, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(h0->fcs_plan_.floats * 4)));
    idqn_group_s* G = new idqn_group_s();
    G->m.assign(members, members + n_members);
    G->slots_off = ((size_t)n_members * sizeof(FcGroupMember) + 15) & ~(size_t)15;
    // the larger of the plain layout {FcGroupMember[S], slots} and the prioritized one (per_group_args.h) at its limits
    G->block_bytes = std::max(G->slots_off + (size_t)n_members * STEPS_SLOTS_BYTES,
                              per_group_steps_block(sizeof(FcGroupMember), n_members, IDQN_MAX_STEPS_PER_CALL, PER_GROUP_MAX_N).bytes);
    *out = G;
    return IDQN_OK;
}

extern "C" int idqn_group_destroy(idqn_group_t G) {
    if (!G) return IDQN_OK;
    (void)hipDeviceSynchronize();
    for (void* p : G->owned) (void)hipFree(p);
    G->many.release();
    G->ring.release();
    delete G;
    return IDQN_OK;
}

// Everything a group learner call refuses, before anything is enqueued, allocated or staged
static int group_learn_check(idqn_group_t G, const char* fn, const idqn_group_ring_t* rings, const int32_t* slots_host, int32_t n_steps, int32_t batch,
                             int32_t mean_divisor, uint32_t flags) {
    IDQN_REQUIRE(G && rings && slots_host, "%s: null pointer", fn);
    IDQN_REQUIRE(n_steps >= 1 && n_steps <= IDQN_MAX_STEPS_PER_CALL, "%s: n_steps %d not in [1, %d]", fn, n_steps, IDQN_MAX_STEPS_PER_CALL);
    IDQN_REQUIRE(batch <= RPS_PAR_SLOTS, "%s: batch %d: a group runs the one-launch step, batches of <= %d samples", fn, batch, RPS_PAR_SLOTS);
    IDQN_REQUIRE((flags & ~(uint32_t)IDQN_F_GRADS_ONLY) == 0, "%s: flags 0x%x: a group call takes IDQN_F_GRADS_ONLY only (profile a member alone)", fn, flags);
    for (size_t g = 0; g < G->m.size(); ++g) {
        const idqn_handle_t h = G->m[g];
        const idqn_group_ring_t& r = rings[g];
        IDQN_REQUIRE(!h->is_weight && !h->td_abs,
                     "%s: member %d has prioritized-replay buffers set (idqn_set_per_buffers): prioritized groups are not served", fn, (int)g);
        long obs_elems;
        if (const int rc = replay_fc_check(h, fn, (const uint8_t*)r.frames_dev, r.n_frames, r.frame_bytes, r.rows_dev, slots_host, nullptr, batch, r.stack,
                                           mean_divisor, flags, &obs_elems))
            return rc;
    }
    return IDQN_OK;
}

// Record g of the table: what a solo launch on member h and ring r receives as kernel arguments (the ring is the minibatch
// source, so the batch pointers stay NULL; weights and |TD| too, unless the prioritized call sets them afterwards)
static void group_fill_member(FcGroupMember& m, idqn_handle_t h, const idqn_group_ring_t& r, bool steps_plan, int32_t batch, int32_t mean_divisor,
                              bool grads_only, const int32_t* slots_dev) {
    h->pend_B = 0; h->pend_stage = 0;
    h->tl_on = false;
    memset(&m, 0, sizeof(m));
    m.a = fc_args(h, batch, mean_divisor, grads_only);
    m.plan = steps_plan ? h->fcs_plan_ : h->fcp_plan_;
    m.ad = h->ad;
    m.theta = h->online; m.mu = h->mu; m.nu = h->nu;
    m.src = fc_ring_src(r.frames_dev, r.rows_dev, r.n_frames, r.frame_bytes, r.stack, RpsSlotsDev{slots_dev});
}

// One launch of grid (K, S): block = {FcGroupMember[S], slots [S][n_steps][batch]}, n_steps == 0: the single step k_fc_group_step
static int group_launch(idqn_group_t G, const idqn_group_ring_t* rings, const int32_t* slots_host, long member_stride, int n_steps, int32_t batch,
                        int32_t mean_divisor, bool grads_only, hipStream_t q) {
    const int S = (int)G->m.size(), ns = std::max(n_steps, 1);
    StagingRing& R = G->ring;
    if (const int rc = R.acquire(G->block_bytes)) return rc;
    FcGroupMember* tab = (FcGroupMember*)R.pin();
    int32_t* slots_pin = (int32_t*)(R.pin() + G->slots_off);
    const int32_t* slots_dev = (const int32_t*)(R.dev() + G->slots_off);
    const long per = (long)ns * batch;
    for (int g = 0; g < S; ++g) {
        const idqn_group_ring_t& r = rings[g];
        memcpy(slots_pin + g * per, slots_host + g * member_stride, (size_t)per * 4);
        group_fill_member(tab[g], G->m[g], r, n_steps != 0, batch, mean_divisor, grads_only, slots_dev + g * per);
    }
    if (const int rc = R.upload(G->slots_off + (size_t)S * per * 4, q)) return rc;
    const idqn_handle_t h0 = G->m[0];
    const dim3 grid((unsigned)h0->cfg.n_heads, (unsigned)S);
    if (n_steps) hipLaunchKernelGGL(k_fc_group_steps, grid, dim3(FCM_T), (size_t)h0->fcs_plan_.floats * 4, q, (const FcGroupMember*)R.dev(), n_steps);
    else hipLaunchKernelGGL(k_fc_group_step, grid, dim3(FCM_T), (size_t)h0->fcp_plan_.floats * 4, q, (const FcGroupMember*)R.dev(), grads_only ? 0 : 1);
    IDQN_HIP_CHECK(hipGetLastError());
    return R.guard(q);
}

extern "C" int idqn_group_learn_on_replay_fc(idqn_group_t G, const idqn_group_ring_t* rings, const int32_t* slots_host, int32_t batch,
                                             int32_t mean_divisor, uint32_t flags, void* stream) {
    if (const int rc = group_learn_check(G, "idqn_group_learn_on_replay_fc", rings, slots_host, 1, batch, mean_divisor, flags)) return rc;
    return group_launch(G, rings, slots_host, batch, 0, batch, mean_divisor, (flags & IDQN_F_GRADS_ONLY) != 0, (hipStream_t)stream);
}

// n_steps prioritized steps of every member, the driver of idqn_group_per_learn_on_replay_fc (n_steps == 1) and
// idqn_group_per_learn_steps_on_replay_fc; P is idqn_per_step_t or idqn_per_steps_t (the same fields; tau_dev is the former's and
// is refused).  Block = {FcGroupMember[n_steps][S], PerSampler[n_steps][S], uniforms [S][n_steps][batch]} (per_group_args.h) in
// the group's staging ring -> one copy of the bytes the call fills -> k_per_group_draw (S) on row 0 -> for every step
// k_fc_group_step (K, S) on that step's records, which carry the members' leaves, weights and |TD| (the members' own
// h->is_weight / h->td_abs stay unset) -> k_per_group_turn (S) behind every step but the last -> k_per_group_write_back (S):
// 2 n_steps + 1 launches.  The persistent k_fc_group_steps cannot serve: every step's draw depends on the previous step's |TD|.
// Every refusal -- the entries' and this one's -- comes before anything is enqueued, allocated or staged.
static_assert(PER_GROUP_MAX_N == RPS_PAR_SLOTS, "a prioritized group batch is a batch of the one-launch step");
template <class P>
static int group_per_learn(idqn_group_t G, const char* fn, const idqn_group_ring_t* rings, const P* per, int32_t n_steps, int32_t batch,
                           int32_t mean_divisor, uint32_t flags, void* stream) {
    IDQN_REQUIRE(batch >= 1 && batch <= PER_GROUP_MAX_N, "%s: batch %d not in [1, %d]: a group runs the one-launch step", fn, batch, PER_GROUP_MAX_N);
    IDQN_REQUIRE(flags == 0, "%s: takes no flags (got 0x%x): profile or split a member's %s alone", fn, flags,
                 std::is_same<P, idqn_per_steps_t>::value ? "steps" : "step");
    const int S = (int)G->m.size(), K = G->m[0]->cfg.n_heads;
    for (int g = 0; g < S; ++g)
        IDQN_REQUIRE(!G->m[g]->is_weight && !G->m[g]->td_abs,
                     "%s: member %d has prioritized-replay buffers set (idqn_set_per_buffers): the call carries the members' weights and |TD| itself", fn, g);
    int bad_g = -1, bad_j = -1;
    const char* bad = per_group_args_error(per, S, n_steps, batch, K, &bad_g, &bad_j);
    IDQN_REQUIRE(!bad || bad_j < 0, "%s: members %d and %d: %s", fn, bad_j, bad_g, bad ? bad : "");
    IDQN_REQUIRE(!bad, "%s: member %d: %s (depth %d, batch %d, n_items %ld)", fn, bad_g, bad, bad_g >= 0 ? per[bad_g].depth : 0, batch,
                 bad_g >= 0 ? (long)per[bad_g].n_items : 0L);
    for (int g = 0; g < S; ++g) {
        const idqn_group_ring_t& r = rings[g];
        long obs_elems;
        if (const int rc = replay_fc_check(G->m[g], fn, (const uint8_t*)r.frames_dev, r.n_frames, r.frame_bytes, r.rows_dev, nullptr, per[g].leaves_dev, batch,
                                           r.stack, mean_divisor, flags, &obs_elems))
            return rc;
    }
    hipStream_t q = (hipStream_t)stream;
    StagingRing& R = G->ring;
    if (const int rc = R.acquire(G->block_bytes)) return rc;
    const PerGroupStepsBlock lay = per_group_steps_block(sizeof(FcGroupMember), S, n_steps, batch);
    uint8_t *pin = R.pin(), *dev = R.dev();
    FcGroupMember* tab = (FcGroupMember*)pin;
    PerSampler* ptab = (PerSampler*)(pin + lay.samplers_off);
    double* uni_pin = (double*)(pin + lay.uniforms_off);
    const double* uni_dev = (const double*)(dev + lay.uniforms_off);
    for (int g = 0; g < S; ++g) {
        const P& p = per[g];
        const size_t rows = (size_t)g * n_steps * batch;  // member g's rows of uniforms
        memcpy(uni_pin + rows, p.uniforms_host, (size_t)n_steps * batch * 8);
        group_fill_member(tab[g], G->m[g], rings[g], false, batch, mean_divisor, false, p.leaves_dev);
        for (int i = 0; i < n_steps; ++i) {  // step i's records: that step's rows of leaves (== slots), weights, |TD|, priorities
            const long o = (long)i * batch;
            FcGroupMember& m = tab[(size_t)i * S + g];
            if (i) m = tab[g];
            m.src.sl.slot = p.leaves_dev + o;
            m.a.is_weight = p.weights_dev + o;
            m.a.td_abs = p.td_abs_dev + o * K;
            PerSampler& s = ptab[(size_t)i * S + g];
            s = per_sampler_of(p, uni_dev + rows + o, K);
            s.leaves += o; s.weights += o; s.td_abs += o * K;
            if (s.priorities) s.priorities += o;
        }
    }
    if (const int rc = R.upload(lay.bytes, q)) return rc;
    const idqn_handle_t h0 = G->m[0];
    const FcGroupMember* tab_dev = (const FcGroupMember*)dev;
    const PerSampler* ptab_dev = (const PerSampler*)(dev + lay.samplers_off);
    const int m2 = st_pow2_at_least(batch);
    hipLaunchKernelGGL(k_per_group_draw, dim3((unsigned)S), dim3(PER_GROUP_DRAW_T), 0, q, ptab_dev, (int)batch);
    for (int i = 0; i < n_steps; ++i) {
        hipLaunchKernelGGL(k_fc_group_step, dim3((unsigned)K, (unsigned)S), dim3(FCM_T), (size_t)h0->fcp_plan_.floats * 4, q, tab_dev + (size_t)i * S, 1);
        if (i + 1 < n_steps)
            hipLaunchKernelGGL(k_per_group_turn, dim3((unsigned)S), dim3(ST_THREADS), 0, q, ptab_dev + (size_t)i * S, ptab_dev + (size_t)(i + 1) * S,
                               (int)batch, m2);
        else
            hipLaunchKernelGGL(k_per_group_write_back, dim3((unsigned)S), dim3(ST_THREADS), 0, q, ptab_dev + (size_t)i * S, (int)batch, m2);
    }
    IDQN_HIP_CHECK(hipGetLastError());
    return R.guard(q);
}

// The prioritized step of every member as ONE call (include/idqn_hip.h): the driver at one step.
extern "C" int idqn_group_per_learn_on_replay_fc(idqn_group_t G, const idqn_group_ring_t* rings, const idqn_per_step_t* per, int32_t batch,
                                                 int32_t mean_divisor, uint32_t flags, void* stream) {
    const char* fn = "idqn_group_per_learn_on_replay_fc";
    IDQN_REQUIRE(G && rings && per, "%s: null pointer", fn);
    return group_per_learn(G, fn, rings, per, 1, batch, mean_divisor, flags, stream);
}

// n_steps of them as ONE call (include/idqn_hip.h): the driver, where n_steps single calls make 3 n_steps launches and n_steps uploads.
extern "C" int idqn_group_per_learn_steps_on_replay_fc(idqn_group_t G, const idqn_group_ring_t* rings, const idqn_per_steps_t* per, int32_t n_steps,
                                                       int32_t batch, int32_t mean_divisor, uint32_t flags, void* stream) {
    const char* fn = "idqn_group_per_learn_steps_on_replay_fc";
    IDQN_REQUIRE(G && rings && per, "%s: null pointer", fn);
    IDQN_REQUIRE(n_steps >= 1 && n_steps <= IDQN_MAX_STEPS_PER_CALL, "%s: n_steps %d not in [1, %d]", fn, n_steps, IDQN_MAX_STEPS_PER_CALL);
    return group_per_learn(G, fn, rings, per, n_steps, batch, mean_divisor, flags, stream);
}

// n_steps steps of every member: ONE launch of k_fc_group_steps (what the members' own idqn_learn_steps_on_replay_fc would run
// persistently), or -- IDQN_FC_LEARN_STEPS_LOOP=1 -- n_steps launches of k_fc_group_step enqueued here, one after the other
extern "C" int idqn_group_learn_steps_on_replay_fc(idqn_group_t G, const idqn_group_ring_t* rings, const int32_t* slots_host, int32_t n_steps,
                                                   int32_t batch, int32_t mean_divisor, uint32_t flags, void* stream) {
    const char* fn = "idqn_group_learn_steps_on_replay_fc";
    IDQN_REQUIRE(flags == 0, "%s: takes no flags (got 0x%x): split a single step through idqn_group_learn_on_replay_fc", fn, flags);
    if (const int rc = group_learn_check(G, fn, rings, slots_host, n_steps, batch, mean_divisor, flags)) return rc;
    if (G->m[0]->fcs_plan_.floats && !fc_steps_force_loop())
        return group_launch(G, rings, slots_host, (long)n_steps * batch, n_steps, batch, mean_divisor, false, (hipStream_t)stream);
    for (int i = 0; i < n_steps; ++i)
        if (const int rc = group_launch(G, rings, slots_host + (long)i * batch, (long)n_steps * batch, 0, batch, mean_divisor, false, (hipStream_t)stream))
            return rc;
    return IDQN_OK;
}

// idqn_act_host_many_fc over the members of a group: state e on head heads[e] of member member[e]; the fc chain is ONE launch
// (every member fits k_fc_act_many1: widths <= 128) behind the copy node, on the group's own slot
extern "C" int idqn_group_act_host_fc(idqn_group_t G, int32_t which, const int32_t* member_host, const int32_t* heads_host,
                                      const void* states_host_pinned, int32_t n, float* q_out_dev, int32_t* actions_host_pinned, void* stream) {
    const char* fn = "idqn_group_act_host_fc";
    IDQN_REQUIRE(G && member_host && heads_host && states_host_pinned && q_out_dev && actions_host_pinned, "%s: null pointer", fn);
    IDQN_REQUIRE(n >= 1 && n <= ACT_MANY_MAX, "%s: n = %d, must be in [1, %d]", fn, n, ACT_MANY_MAX);
    IDQN_REQUIRE(which == 0 || which == 1, "%s: which = %d", fn, which);
    const idqn_handle_t h0 = G->m[0];
    const int K = h0->cfg.n_heads, S = (int)G->m.size();
    for (int e = 0; e < n; ++e) {
        IDQN_REQUIRE(member_host[e] >= 0 && member_host[e] < S, "%s: member %d of state %d", fn, member_host[e], e);
        IDQN_REQUIRE(heads_host[e] >= 0 && heads_host[e] < K, "%s: head %d of state %d", fn, heads_host[e], e);
    }
    const size_t sb = (size_t)h0->fc.d[0] * 4;
    ActManySlot& s = G->many;
    if (!s.block) {
        long fl[4] = {0, 0, 0, (long)ACT_MANY_MAX * 2 * h0->fc.dmax};
        if (const int rc = act_many_alloc(s, G->owned, sizeof(FcGroupActTable), sb, fl, 4)) return rc;
    }
    FcGroupActTable* gt = (FcGroupActTable*)s.pin;
    act_many_fill_table(&gt->tab, which, heads_host, n, K, false);
    for (int e = 0; e < ACT_MANY_MAX; ++e) {  // (entries past n: state 0's, never read)
        const idqn_handle_t h = G->m[member_host[e < n ? e : 0]];
        gt->params[e] = (which ? h->target : h->online) + (long)heads_host[e < n ? e : 0] * h->L.head_stride;
    }
    memcpy(s.pin + sizeof(FcGroupActTable), states_host_pinned, (size_t)n * sb);
    return act_many_run(h0, s, fn, n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream, [&](hipStream_t qs, int32_t* mail_dev) {
        FcActManyArgs a;
        a.net = h0->fc;
        a.nets.tab = (const ActManyTable*)s.block; a.nets.online = nullptr; a.nets.target = nullptr; a.nets.pstride = 0;  // (the bases are in the table)
        a.s = (const float*)(s.block + s.head_bytes); a.s_ld = h0->fc.d[0]; a.ws = s.part; a.q_out = q_out_dev;
        a.action = s.action; a.mail = mail_dev; a.ctr = s.ctr; a.n = n;
        hipLaunchKernelGGL(k_fc_group_act_many1, dim3(n), dim3(512), 0, qs, a, (const FcGroupActTable*)s.block);
        return IDQN_OK;
    });
}

// ---- acting groups: the greedy actions of S MFMA-cnn agents in one call (act_many_kernels.h, act_group_args.h) ----------------
// The chain of idqn_act_host_many -- one copy node, three conv launches, Dense_0 per group of states, the head kernel per state
// -- with every state's parameter base read from a table in the uploaded block (ActGroupTable: member, parameter set and head
// resolved here) instead of one handle's arena.  The group owns ONE acting slot and nothing else; it allocates nothing on a
// member, writes no member memory, and a member may be driven alone between two group calls.  The chain is captured on member
// 0's capture stream and reads member 0's shapes, which every member shares.
static_assert(ACT_GROUP_MAX == ACT_MANY_MAX, "act_group_args.h restates ACT_MANY_MAX");
struct idqn_act_group_s {
    std::vector<idqn_handle_t> m;
    ActManySlot many;
    std::vector<void*> owned;
};

extern "C" int idqn_act_group_create(const idqn_handle_t* members, int32_t n_members, idqn_act_group_t* out) {
    const char* fn = "idqn_act_group_create";
    IDQN_REQUIRE(members && out, "%s: null pointer", fn);
    IDQN_REQUIRE(n_members >= 1 && n_members <= ACT_MANY_MAX, "%s: %d members, must be in [1, %d]", fn, n_members, ACT_MANY_MAX);
    IDQN_REQUIRE(!act_generic(), "%s: IDQN_ACT_GENERIC routes acting through the batched forward: no acting groups", fn);
    for (int g = 0; g < n_members; ++g) {
        const idqn_handle_t h = members[g];
        IDQN_REQUIRE(h, "%s: member %d is null", fn, g);
        IDQN_REFUSE_IMPALA(h, fn);
        IDQN_REQUIRE(h->cfg.n_quantiles == 0 && h->iqn.N == 0, "%s: member %d was created with quantile heads", fn, g);
        IDQN_REQUIRE(h->cfg.arch == IDQN_ARCH_CNN, "%s: member %d is an MLP (fc) handle: idqn_group_create serves those", fn, g);
        // (idqn_create sends J > 512 and A > 32 down the general-shape path: named first, under their own texts)
        const int J_cfg = h->cfg.features[h->cfg.n_features - 1];
        IDQN_REQUIRE(J_cfg <= 512, "%s: member %d has J = %d > 512: the acting kernels take J = 128 m <= 512", fn, g, J_cfg);
        IDQN_REQUIRE(h->cfg.n_actions <= 32, "%s: member %d has A = %d > 32 actions: the acting kernels take A <= 32", fn, g, h->cfg.n_actions);
        IDQN_REQUIRE(!h->gc.on, "%s: member %d is a general-shape cnn handle: outside the single-state MFMA cnn acting path", fn, g);
        if (const int rc = act_many_conv_plans(h, fn)) return rc;
        IDQN_REQUIRE(same_member_shape(h->cfg, members[0]->cfg, false), "%s: member %d differs from member 0 in shape (obs, features, n_actions, n_heads)", fn, g);
        for (int j = 0; j < g; ++j) IDQN_REQUIRE(members[j] != h, "%s: members %d and %d are the same handle", fn, j, g);
    }
    IDQN_REQUIRE(((size_t)members[0]->cfg.obs_h * members[0]->cfg.obs_w * members[0]->cfg.obs_c) % 4 == 0, "%s: bytes per state must be a multiple of 4", fn);
    idqn_act_group_s* G = new idqn_act_group_s();
    G->m.assign(members, members + n_members);
    *out = G;
    return IDQN_OK;
}

extern "C" int idqn_act_group_destroy(idqn_act_group_t G) {
    if (!G) return IDQN_OK;
    (void)hipDeviceSynchronize();
    for (void* p : G->owned) (void)hipFree(p);
    G->many.release();
    delete G;
    return IDQN_OK;
}

extern "C" int idqn_act_group_host(idqn_act_group_t G, int32_t which, const int32_t* member_host, const int32_t* heads_host,
                                   const void* states_host_pinned, int32_t n, float* q_out_dev, int32_t* actions_host_pinned, void* stream) {
    const char* fn = "idqn_act_group_host";
    IDQN_REQUIRE(G && member_host && heads_host && states_host_pinned && q_out_dev && actions_host_pinned, "%s: null pointer", fn);
    const idqn_handle_t h0 = G->m[0];
    const int K = h0->cfg.n_heads, S = (int)G->m.size();
    int bad = -1;
    if (const char* why = act_group_args_error(n, S, K, which, member_host, heads_host, &bad)) {
        if (bad >= 0) IDQN_REQUIRE(false, "%s: %s: state %d, member %d, head %d (%d members, %d heads)", fn, why, bad, member_host[bad], heads_host[bad], S, K);
        IDQN_REQUIRE(false, "%s: %s (n = %d, which = %d)", fn, why, n, which);
    }
    for (int g = 0; g < S; ++g)
        IDQN_REQUIRE(G->m[g]->act_pending == 0, "%s: member %d has an idqn_act_host_begin still waiting for its _end", fn, g);
    const size_t sb = (size_t)h0->cfg.obs_h * h0->cfg.obs_w * h0->cfg.obs_c;  // bytes of one state (a multiple of 4: _create)
    const long NRG = std::max(1, 256 / (h0->J / 128));
    ActManySlot& s = G->many;
    if (!s.block) {
        long fl[4] = {0, 0, 0, ACT_MANY_MAX * NRG * h0->J};
        for (int i = 0; i < 3; ++i) fl[i] = (long)ACT_MANY_MAX * h0->conv[i].OH * h0->conv[i].OW * h0->conv[i].CO;
        if (const int rc = act_many_alloc(s, G->owned, sizeof(ActGroupTable), sb, fl, 4)) return rc;
    }
    ActGroupTable* gt = (ActGroupTable*)s.pin;
    ActManyTable* tb = &gt->tab;
    int32_t g_member[ACT_MANY_MAX];
    tb->n = n; tb->which = which; tb->pad = 0;
    tb->n_groups = act_group_build(n, member_host, heads_host, tb->order, g_member, tb->g_head, tb->g_start, tb->g_count);
    for (int e = 0; e < ACT_MANY_MAX; ++e) {  // (entries past n: state 0's, never read)
        const int src = e < n ? e : 0;
        const idqn_handle_t h = G->m[member_host[src]];
        tb->head[e] = heads_host[src];
        gt->params[e] = (which ? h->target : h->online) + (long)heads_host[src] * h->L.head_stride;
    }
    memcpy(s.pin + sizeof(ActGroupTable), states_host_pinned, (size_t)n * sb);
    const int max_groups = (int)std::min<long>(std::min<long>(n, (long)S * K), ACT_MANY_MAX);
    return act_many_run(h0, s, fn, n, sb, q_out_dev, actions_host_pinned, (hipStream_t)stream, [&](hipStream_t qs, int32_t* mail_dev) -> int {
        ActGroupNets nets;
        nets.gt = (const ActGroupTable*)s.block;
        if (const int rc = act_many_convs(h0, nets, s.block + s.head_bytes, s.a, n, qs)) return rc;
        ActGroupDenseArgs d;
        d.nets = nets; d.a3 = s.a[2]; d.part = s.part; d.w_off = h0->off_w0; d.F = h0->F; d.J = h0->J; d.NRG = (int)NRG;
        hipLaunchKernelGGL(k_act_group_dense0, dim3(d.NRG * (h0->J / 128), max_groups), dim3(256), 0, qs, d);
        ActGroupHeadArgs ha;
        ha.nets = nets; ha.part = s.part; ha.b0_off = h0->off_b0; ha.w1_off = h0->off_w1; ha.b1_off = h0->off_b1;
        ha.NP = d.NRG; ha.J = h0->J; ha.A = h0->cfg.n_actions; ha.n = n; ha.q_out = q_out_dev; ha.action = s.action;
        ha.mail = mail_dev; ha.ctr = s.ctr;
        hipLaunchKernelGGL(k_act_group_head, dim3(n), dim3(1024), 0, qs, ha);
        return IDQN_OK;
    });
}
