// Reduced-ResNet18 / SupConResNet engine: owns the layer table, the workspace layout and the kernel sequences of
// forward (train / eval) and backward.  Mirrors models/resnet.py:69-116 (ResNet(BasicBlock,[2,2,2,2],nf=20)) and
// :140-168 (SupConResNet) of the reference; parameters stay in PyTorch's named_parameters() order and OIHW layout.
#include "conv.h"
#include <chrono>
#include <limits.h>
#include <string.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <map>
#include <algorithm>
#include <tuple>
#include <array>

using namespace ocl;

namespace {

const int kGmax = 8;  // BN groups per forward (SCR uses 2)
const int kBnFusedReps = 8;  // replicas of the one-pass BatchNorm backward's accumulators ([rep][2 groups][2][C]; its arrival counters follow them)

struct TensorInfo {
    std::string name;
    int64_t off;
    int ndim;
    int64_t shape[4];
    int64_t numel;
};
struct BnInfo {
    std::string name;
    int C;
    int gamma_t, beta_t;  // tensor indices
    int64_t stat_off;     // into the running flat array: mean[C], var[C]
    int64_t arena_off;    // into per-BN arenas of size kGmax*2*C (doubles) / 2*C floats for the fold
    int64_t barena_off;   // the backward's reduction arena: 2*kGmax*2*C cells, two BatchNorms sharing dz ([set][G][2][C]) at every G <= kGmax
    int64_t fused_off;    // one-pass BatchNorm backward: replicated accumulators + arrival counter (doubles, in the bsums arena)
    int64_t save_off;     // into the slot's saved mean/invstd area (floats): mean[kGmax*C], invstd[kGmax*C]
};
struct ConvInfo : ConvShape {
    int w_t;          // weight tensor index
    int bn;           // following BatchNorm
    int64_t tf_off, td_off;  // K-grouped weight packs in the arena (floats): forward, data gradient
    int64_t y_off;    // raw output inside a slot (floats)
    int xf_src;       // conv2 of a block: its block's conv1, whose BatchNorm + ReLU this convolution can apply itself (-1: none)
};
struct BlockInfo {
    int conv1, conv2, convs;  // convs = -1: identity shortcut
    int64_t a1_off, z_off;    // post-ReLU activations inside a slot
};

struct PlanSet {
    std::vector<ConvPlan> fwd;                  // per conv
    std::vector<std::vector<ConvPlan>> dgrad;   // per conv: 0 (stem), 1 or 4 launches
    std::vector<WgradPlan> wgrad;
    std::vector<int64_t> partial_off;           // per conv: its own slab region (batched reduction), floats
    bool batched_reduce = false;                // every layer's slabs fit the workspace side by side
    std::vector<char> dgrad_bnb;                // per conv: its data-gradient plan follows the BatchNorm groups and has room for the EPI_BNB table
    std::vector<int> wgrad_target;              // per conv: plan_wgrad's wg_target (> 0: split for the merged launch of the pass)
};

}  // namespace

struct ocl_net {
    ocl_net_desc d;
    std::vector<TensorInfo> tensors;
    std::vector<BnInfo> bns;
    std::vector<ConvInfo> convs;
    std::vector<BlockInfo> blocks;
    int64_t n_params = 0, n_stats = 0;
    int feat_dim = 0, out_dim = 0, Hf = 0, Wf = 0;
    int t_linear_w = -1, t_linear_b = -1, t_h0_w = -1, t_h0_b = -1, t_h2_w = -1, t_h2_b = -1;

    // workspace layout (bytes)
    int64_t ws_bytes = 0;
    int64_t slot_bytes = 0, slot_base = 0;
    int64_t x4_off = 0, zstem_off = 0, save_off_base = 0, feat_off = 0, h1_off = 0, h2_off = 0, norms_off = 0, out_off = 0;  // floats in slot
    int64_t slot_floats = 0;
    int64_t gbuf_floats = 0;
    int64_t off_g[5] = {0, 0, 0, 0, 0};
    static const int kDyRing = 6;        // dL/dy buffers handed to the weight-gradient stream (see ocl_net_backward)
    int64_t off_dy[6] = {0, 0, 0, 0, 0, 0};
    // one dL/dy buffer per layer for replay-sized passes: their weight gradients wait for the end of the backward and leave in one launch
    static const int kDyKeep = 24;
    int64_t off_dykeep = 0, dykeep_floats = 0;   // floats per buffer
    int64_t off_partial = 0, partial_floats = 0;
    int64_t off_stats = 0, stats_doubles = 0, stats_rep_stride = 0;
    int64_t off_bsums = 0, bsums_doubles = 0;
    int64_t off_pack = 0, pack_floats = 0;
    int64_t off_fold = 0, fold_floats = 0;
    int64_t off_descs = 0;
    int64_t off_head = 0, head_floats = 0;  // dh2, dh1, dfeat, eval feat scratch
    int64_t max_act_floats = 0;

    // bound storage
    float* params = nullptr;
    float* grads = nullptr;
    float* running = nullptr;
    int64_t* nbt = nullptr;
    unsigned char* ws = nullptr;
    bool bound = false;
    bool descs_uploaded = false;
    const float* pack_src = nullptr;   // parameter array the weight-pack arena was last written from (by a forward)
    int pack_have = 0;                 // PACK_* bits of the packs that hold `pack_src`'s weights
    hipStream_t pack_stream = nullptr; // stream the packs were last written on: a forward elsewhere has no dependency on them
    bool bsums_clean = false;          // the backward's statistics arena was cleared by the last forward's pack launch and not used since
    int pack_need_fwd = 0, pack_need_bwd = 0;   // packs the plans made so far read (forward pack; data-gradient pack once a backward is planned)

    int dbg_stop = -1;            // debug: return from backward right after stage (block*10 + step)
    float* dbg_role[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<int> slot_n, slot_groups;
    std::vector<bool> slot_valid, slot_frozen, slot_fused;   // fused: bn1 + ReLU of every block ran inside conv2 (no a1 on the tape)
    std::map<std::pair<int, int>, PlanSet> plans;
    PlanArena plan_arena;         // device tables of the plans (written at a plan's first launch)

    float* slotf(int slot) const { return (float*)(ws + slot_base + (int64_t)slot * slot_bytes); }
    float* gbuf(int i) const { return (float*)(ws + off_g[i]); }
    float* dybuf(int i) const { return (float*)(ws + off_dy[i]); }
    float* dykeep(int i) const { return (float*)(ws + off_dykeep) + (int64_t)i * dykeep_floats; }
    float* partialbuf() const { return (float*)(ws + off_partial); }
    StatCell* statsbuf() const { return (StatCell*)(ws + off_stats); }
    StatCell* bsumsbuf() const { return (StatCell*)(ws + off_bsums); }

    // second stream for the weight gradients + events (created on first backward)
    hipStream_t s2 = nullptr;
    std::vector<hipEvent_t> ev_ready;      // main -> s2: a dL/dy buffer has been written
    hipEvent_t ev_done[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // s2 -> main: ring slot no longer read
    bool ev_done_pending[6] = {false, false, false, false, false, false};
    hipEvent_t ev_join = nullptr, ev_fork = nullptr;
    int dy_next = 0;
    size_t ev_next = 0;

    // launch-sequence replay (OCL_GRAPH=1): the kernel sequence of a forward / backward with given shapes, slot and flags is captured
    // once into a hipGraph and replayed, so that the host pays one graph launch instead of 60 - 100 kernel launches + events
    struct GraphKey {
        int kind, N, G, slot, a, b, c;
        uint64_t p;
        bool operator<(const GraphKey& o) const {   // field by field: the struct has padding bytes a copy need not preserve
            return std::tie(kind, N, G, slot, a, b, c, p) < std::tie(o.kind, o.N, o.G, o.slot, o.a, o.b, o.c, o.p);
        }
    };
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        int seen = 0;
        bool failed = false;
    };
    std::map<GraphKey, GraphSlot> graphs;
    bool capturing = false;
    // device tables of the merged weight-gradient launches, per (images, groups, tape slot): [form set]
    std::map<std::tuple<int, int, const float*>, std::array<WgradMultiTable, 2>> wgrad_tables;
};

// Every address of one BatchNorm, for the parameter array P, the gradient array Gr (null in a forward) and the tape slot S of a pass.  The
// only place that knows save_off, kGmax * C, stat_off, arena_off, barena_off and fused_off: the kernel-argument structs are filled from it.
struct BnView {
    int C;
    const float *gamma, *beta;
    float *dgamma, *dbeta;
    float *save_mean, *save_invstd;      // [kGmax][C] each, in the slot
    float *running_mean, *running_var;
    int64_t* nbt;
    StatCell* stats;                     // forward: [kStatReps][G][2][C], replica stride stats_rep_stride
    StatCell* bsums;                     // backward: [set][G][2][C], two BatchNorms sharing dz fit at every G <= kGmax
    StatCell* fsums;                     // backward, <= 2 groups: the one-pass kernel's replicas / the data-gradient epilogue's sums
    unsigned* barrier;                   // ... and the arrival counters behind them
};
static BnView bn_view(const ocl_net* n, const float* P, float* Gr, float* S, int bn) {
    const BnInfo& b = n->bns[bn];
    const int64_t g = n->tensors[b.gamma_t].off, be = n->tensors[b.beta_t].off;
    BnView v;
    v.C = b.C;
    v.gamma = P + g; v.beta = P + be;
    v.dgamma = Gr ? Gr + g : nullptr; v.dbeta = Gr ? Gr + be : nullptr;
    v.save_mean = S + b.save_off; v.save_invstd = S + b.save_off + (int64_t)kGmax * b.C;
    v.running_mean = n->running + b.stat_off; v.running_var = n->running + b.stat_off + b.C;
    v.nbt = n->nbt + bn;
    v.stats = n->statsbuf() + b.arena_off;
    v.bsums = n->bsumsbuf() + b.barena_off;
    v.fsums = n->bsumsbuf() + b.fused_off;
    v.barrier = (unsigned*)(v.fsums + (int64_t)kBnFusedReps * 2 * 2 * b.C);
    return v;
}

// -----------------------------------------------------------------------------------------------------
static int add_tensor(ocl_net* n, const std::string& name, std::initializer_list<int64_t> shape) {
    TensorInfo t;
    t.name = name;
    t.off = n->n_params;
    t.ndim = (int)shape.size();
    t.numel = 1;
    int i = 0;
    for (auto s : shape) {
        t.shape[i++] = s;
        t.numel *= s;
    }
    for (; i < 4; ++i) t.shape[i] = 1;
    n->n_params += t.numel;
    n->tensors.push_back(t);
    return (int)n->tensors.size() - 1;
}
static int add_bn(ocl_net* n, const std::string& prefix, int C) {
    BnInfo b;
    b.name = prefix;
    b.C = C;
    b.gamma_t = add_tensor(n, prefix + ".weight", {C});
    b.beta_t = add_tensor(n, prefix + ".bias", {C});
    b.stat_off = n->n_stats;
    n->n_stats += 2 * C;
    n->bns.push_back(b);
    return (int)n->bns.size() - 1;
}
static int add_conv(ocl_net* n, const std::string& name, int Cin, int Cout, int k, int stride, int Hin, int Win) {
    ConvInfo c;
    memset((void*)&c, 0, sizeof(c));
    c.Cin = Cin;
    c.CinT = Cin == 3 ? 4 : Cin;
    c.Cout = Cout;
    c.k = k;
    c.stride = stride;
    c.Hin = Hin;
    c.Win = Win;
    const int pad = k == 3 ? 1 : 0;
    c.Ho = (Hin + 2 * pad - k) / stride + 1;
    c.Wo = (Win + 2 * pad - k) / stride + 1;
    c.w_t = add_tensor(n, name + ".weight", {Cout, Cin, k, k});
    c.bn = -1;
    c.xf_src = -1;
    n->convs.push_back(c);
    return (int)n->convs.size() - 1;
}

static int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
// the size of a pass of N images, as the thresholds below state it: images x input pixels
static int64_t in_pixels(const ocl_net* n, int N) { return (int64_t)N * n->d.in_h * n->d.in_w; }

static const int kTwoStreamMinBatch = 48;
static int build_layout(ocl_net* n) {
    const ocl_net_desc& d = n->d;
    const std::string pre = d.head == 0 ? "" : "encoder.";
    int H = d.in_h, W = d.in_w;
    // stem
    int c = add_conv(n, pre + "conv1", 3, d.nf, 3, 1, H, W);
    n->convs[c].bn = add_bn(n, pre + "bn1", d.nf);
    int in_planes = d.nf;
    for (int layer = 0; layer < 4; ++layer) {
        const int planes = d.nf << layer;
        for (int b = 0; b < 2; ++b) {
            const int stride = (b == 0 && layer > 0) ? 2 : 1;
            const std::string bp = pre + "layer" + std::to_string(layer + 1) + "." + std::to_string(b);
            BlockInfo bi;
            memset(&bi, 0, sizeof(bi));
            bi.conv1 = add_conv(n, bp + ".conv1", in_planes, planes, 3, stride, H, W);
            n->convs[bi.conv1].bn = add_bn(n, bp + ".bn1", planes);
            const int Ho = n->convs[bi.conv1].Ho, Wo = n->convs[bi.conv1].Wo;
            bi.conv2 = add_conv(n, bp + ".conv2", planes, planes, 3, 1, Ho, Wo);
            n->convs[bi.conv2].bn = add_bn(n, bp + ".bn2", planes);
            n->convs[bi.conv2].xf_src = bi.conv1;
            bi.convs = -1;
            if (stride != 1 || in_planes != planes) {
                bi.convs = add_conv(n, bp + ".shortcut.0", in_planes, planes, 1, stride, H, W);
                // nn.Sequential(conv, bn): parameter names shortcut.0.weight, shortcut.1.weight, shortcut.1.bias
                n->convs[bi.convs].bn = add_bn(n, bp + ".shortcut.1", planes);
            }
            n->blocks.push_back(bi);
            in_planes = planes;
            H = Ho;
            W = Wo;
        }
    }
    n->Hf = H;
    n->Wf = W;
    const int PH = H / 4, PW = W / 4;
    OCL_REQUIRE(PH >= 1 && PW >= 1, "net: input %dx%d too small for avg_pool2d(4)", d.in_h, d.in_w);
    n->feat_dim = in_planes * PH * PW;
    // SupConResNet always builds encoder = Reduced_ResNet18(100): its (unused) linear is [100, nf*8] even for 84x84
    // inputs (models/resnet.py:144); the plain ResNet's linear is replaced to match the feature size
    // (utils/setup_elements.py:63-66).
    const int lin_in = d.head == 0 ? n->feat_dim : in_planes;
    n->t_linear_w = add_tensor(n, pre + "linear.weight", {d.n_classes, lin_in});
    n->t_linear_b = add_tensor(n, pre + "linear.bias", {d.n_classes});
    OCL_REQUIRE(n->tensors[n->t_linear_b].off == n->tensors[n->t_linear_w].off + n->tensors[n->t_linear_w].numel, "net: linear.weight / linear.bias not adjacent");
    if (d.head == 0) {
        n->out_dim = d.n_classes;
    } else if (d.head == 1) {
        n->t_h0_w = add_tensor(n, "head.0.weight", {n->feat_dim, n->feat_dim});
        n->t_h0_b = add_tensor(n, "head.0.bias", {n->feat_dim});
        n->t_h2_w = add_tensor(n, "head.2.weight", {d.feat_dim, n->feat_dim});
        n->t_h2_b = add_tensor(n, "head.2.bias", {d.feat_dim});
        n->out_dim = d.feat_dim;
    } else if (d.head == 2) {
        n->t_h2_w = add_tensor(n, "head.weight", {d.feat_dim, n->feat_dim});
        n->t_h2_b = add_tensor(n, "head.bias", {d.feat_dim});
        n->out_dim = d.feat_dim;
    } else {
        n->out_dim = n->feat_dim;
    }

    // ---- pack arena -------------------------------------------------------------------------------
    int64_t pk = 0;
    for (auto& cv : n->convs) {
        cv.CoutP = pack_width(cv.Cout);
        cv.tf_off = pk;
        pk += (int64_t)cv.k * cv.k * cv.CinT * cv.CoutP;
        if (cv.Cin != 3) {
            cv.CiP = pack_width(cv.Cin);
            pk = align_up(pk, 64);
            cv.td_off = pk;
            pk += (int64_t)cv.k * cv.k * cv.Cout * cv.CiP;
        } else {
            cv.CiP = 0;
            cv.td_off = -1;
        }
        pk = align_up(pk, 64);
    }
    n->pack_floats = pk;

    // ---- slot layout (floats) -------------------------------------------------------------------------
    const int64_t N = d.max_batch;
    int64_t o = 0;
    auto take = [&](int64_t nfl) {
        const int64_t r = o;
        o = align_up(o + nfl, 64);
        return r;
    };
    n->x4_off = take(N * d.in_h * d.in_w * 4);
    int64_t max_act = N * d.in_h * d.in_w * 4;
    for (auto& cv : n->convs) {
        const int64_t sz = N * cv.Ho * cv.Wo * cv.Cout;
        cv.y_off = take(sz);
        max_act = std::max(max_act, sz);
    }
    n->zstem_off = take(N * n->convs[0].Ho * n->convs[0].Wo * n->convs[0].Cout);
    for (auto& b : n->blocks) {
        const ConvInfo& c1 = n->convs[b.conv1];
        const int64_t sz = N * c1.Ho * c1.Wo * c1.Cout;
        b.a1_off = take(sz);
        b.z_off = take(sz);
    }
    n->save_off_base = o;
    for (auto& b : n->bns) {
        b.save_off = take((int64_t)2 * kGmax * b.C);
    }
    n->feat_off = take(N * n->feat_dim);
    n->h1_off = take(N * n->feat_dim);
    n->h2_off = take(N * std::max(n->out_dim, 1));
    n->norms_off = take(N);
    n->out_off = take(N * n->out_dim);
    n->slot_floats = o;
    n->max_act_floats = max_act;

    // ---- global workspace (bytes) ---------------------------------------------------------------------
    int64_t w = 0;
    auto takeb = [&](int64_t bytes) {
        const int64_t r = w;
        w = align_up(w + bytes, 256);
        return r;
    };
    n->gbuf_floats = max_act;
    for (int i = 0; i < 5; ++i) n->off_g[i] = takeb(max_act * 4);
    for (int i = 0; i < ocl_net::kDyRing; ++i) n->off_dy[i] = takeb(max_act * 4);
    n->dykeep_floats = align_up(max_act, 64);
    n->off_dykeep = takeb(n->dykeep_floats * 4 * ocl_net::kDyKeep);
    // wgrad partial: worst case over layers for the largest batch
    int64_t pmax = 0;
    for (auto& cv : n->convs) {
        WgradPlan wp;
        int rc = plan_wgrad((int)N, cv.Hin, cv.Win, cv.CinT, cv.Ho, cv.Wo, cv.Cout, cv.k, cv.stride, &wp);
        if (rc != OCL_OK) return rc;
        pmax = std::max<int64_t>(pmax, (int64_t)wp.partial_floats);
    }
    // plan_wgrad caps the split-K slabs at 12 MB for every batch size (the split differs per batch): size for the cap
    // (and for the side-by-side slab regions of the batched reduction of replay-sized batches: 64 MB)
    n->partial_floats = std::max<int64_t>(pmax, (int64_t)(64ll << 20) / 4) + 1024;
    n->off_partial = takeb(n->partial_floats * 4);
    int64_t so = 0;
    for (auto& b : n->bns) {
        b.arena_off = so;
        so += (int64_t)kGmax * 2 * b.C;
    }
    n->stats_doubles = so * kStatReps;   // kStatReps replicas of the whole arena, replica stride `so`
    n->stats_rep_stride = so;
    n->off_stats = takeb(n->stats_doubles * (int64_t)sizeof(StatCell));   // (counts are in accumulator cells)
    // backward: [2 sets][G][2][C] per BN, followed by the one-pass kernel's arenas (8 replicas x 2 groups x 2 x C + counter per BN)
    int64_t fo = 0;
    for (auto& b : n->bns) {
        b.barena_off = fo;
        fo += (int64_t)2 * kGmax * 2 * b.C;
    }
    for (auto& b : n->bns) {
        b.fused_off = fo;
        fo += (int64_t)kBnFusedReps * 2 * 2 * b.C + 8;   // + 9 arrival counters (unsigned)
    }
    n->bsums_doubles = fo;
    n->off_bsums = takeb(fo * (int64_t)sizeof(StatCell));
    n->off_pack = takeb(n->pack_floats * 4);
    n->fold_floats = n->n_stats;  // scale[C], shift[C] per BN, same layout as running stats
    n->off_fold = takeb(n->fold_floats * 4);
    n->off_descs = takeb((int64_t)(n->convs.size() * sizeof(PackDesc) + n->bns.size() * sizeof(BnFoldDesc) + 256));
    n->head_floats = N * ((int64_t)n->feat_dim * 3 + n->out_dim * 3 + 64);   // dfeat, dh1, dh2 (<= max(feat_dim, out_dim) each), staged dout
    n->off_head = takeb(n->head_floats * 4);
    n->slot_base = w;
    n->slot_bytes = align_up(n->slot_floats * 4, 256);
    w += n->slot_bytes * d.n_slots;
    n->ws_bytes = w;
    n->slot_n.assign(d.n_slots, 0);
    n->slot_groups.assign(d.n_slots, 1);
    n->slot_valid.assign(d.n_slots, false);
    n->slot_frozen.assign(d.n_slots, false);
    n->slot_fused.assign(d.n_slots, false);
    return OCL_OK;
}

// Stage 2 of the BatchNorm-backward epilogue (the stem's BatchNorm and layer1.0.bn2 through the data gradient that completes their dL/dz)
// pays on passes of up to ~160 x 32 x 32 input pixels (20 images: -20 us per pass, 20 x 84 x 84: -10 us) and loses at SCR's 220 views
// (+17 us: the epilogue's y / mask loads on 18 MB tensors are exposed once per launch): profiles/r5_switches_netcheck.txt
static const int64_t kBnbEpi2MaxPix = 160 * 1024;

// The plans of one pass: every layer's forward, data-gradient and weight-gradient geometry and the planner's choice for it.  Host only
// (no device state is touched): get_plans caches its result per (N, groups), ocl_test_net_forms lists it for the planner-coverage test.
static int make_plan_set(const ocl_net* n, int N, int groups, PlanSet* out) {
    PlanSet& ps = *out;
    ps.fwd.resize(n->convs.size());
    ps.dgrad.resize(n->convs.size());
    ps.wgrad.resize(n->convs.size());
    ps.dgrad_bnb.assign(n->convs.size(), 0);
    ps.wgrad_target.assign(n->convs.size(), 0);
    // BatchNorm backward of bn1: its two batch sums in the epilogue of conv2's data gradient (EPI_BNB) + a streaming apply kernel instead
    // of the one-pass kernel with its grid-wide arrival (OCL_BNB_EPI=0: the one-pass kernel).  The replicated arena holds <= 2 groups.
    static const bool env_bnb = env_not_off("OCL_BNB_EPI");
    for (size_t i = 0; i < n->convs.size(); ++i) {
        const ConvInfo& c = n->convs[i];
        ConvGeomDesc g;
        geom_fwd(c, N, groups, &g);
        g.xf = c.xf_src >= 0 ? 1 : 0;   // room for the input-transform table (used by train-mode passes only)
        int rc = plan_conv(g, &ps.fwd[i]);
        if (rc != OCL_OK) return rc;
        if (c.Cin != 3) {
            std::vector<ConvGeomDesc> dg;
            // (stage 2, passes up to kBnbEpi2MaxPix: the data gradient of conv1 of an identity block completes dL/dz of the block in front
            // of it -- or of the stem -- and carries the reduction half of THAT BatchNorm's backward (bn2 of a block without a projection
            // shortcut, the stem's) the same way; see trunk_backward)
            const bool size_bnb2 = in_pixels(n, N) <= kBnbEpi2MaxPix;
            bool bnb2 = false;
            if (env_bnb && size_bnb2 && c.stride == 1 && groups <= 2)
                for (size_t k = 0; k < n->blocks.size(); ++k)
                    if (n->blocks[k].conv1 == (int)i && n->blocks[k].convs < 0 && (k == 0 || n->blocks[k - 1].convs < 0)) bnb2 = true;
            const bool bnb = (env_bnb && c.xf_src >= 0 && c.stride == 1 && groups <= 2) || bnb2;   // conv2 of a block: its data gradient enters bn1's backward
            // stride-2 3x3: the four parity classes as one launch where conv_t_kernel can take them (else four launches)
            geom_dgrad(c, N, &dg, true, bnb ? groups : 1);
            if (bnb && dg.size() == 1) {
                dg[0].bnb = 1;
                ps.dgrad_bnb[i] = 1;
            }
            if (dg.size() == 1 && dg[0].ncls > 1) {
                ConvPlan p;
                if (plan_conv(dg[0], &p) != OCL_OK) geom_dgrad(c, N, &dg, false);
            }
            for (auto& q : dg) {
                ConvPlan p;
                rc = plan_conv(q, &p);
                if (rc != OCL_OK) return rc;
                ps.dgrad[i].push_back(p);
            }
        }
        // (a pass whose weight gradients leave in one launch -- trunk_backward's `defer` -- splits every layer's pixels less)
        // (96 workgroups per layer: the merged launch 111 -> ~70 us, the 20-image pass 746 -> 706 us, ER 0.818 -> 0.779 ms; 192 / 128 / 64 / 48 / 32:
        // 0.790 / 0.790 / 0.785 / 0.786 / 0.801 ms -- profiles/r6_wgrad_multi_target.txt; 0 = split as for a launch of its own)
        static const int env_mt = env_int("OCL_WGRAD_MULTI_TARGET", 96);
        const bool merged = env_mt > 0 && N < kTwoStreamMinBatch && in_pixels(n, N) < (int64_t)kTwoStreamMinBatch * 1024;
        ps.wgrad_target[i] = merged ? env_mt : 0;
        rc = plan_wgrad(N, c.Hin, c.Win, c.CinT, c.Ho, c.Wo, c.Cout, c.k, c.stride, &ps.wgrad[i], c.xf_src >= 0 ? groups : 0, ps.wgrad_target[i]);
        if (rc != OCL_OK) return rc;
        if ((int64_t)ps.wgrad[i].partial_floats > n->partial_floats) {
            set_error("net: wgrad partial workspace too small (%zu > %lld floats)", ps.wgrad[i].partial_floats,
                      (long long)n->partial_floats);
            return OCL_ERR_STATE;
        }
    }
    {
        int64_t off = 0;
        ps.partial_off.resize(n->convs.size());
        for (size_t i = 0; i < n->convs.size(); ++i) {
            ps.partial_off[i] = off;
            off += (int64_t)((ps.wgrad[i].partial_floats + 63) / 64) * 64;
        }
        ps.batched_reduce = off <= n->partial_floats && (int)n->convs.size() <= kMaxReduceLayers;
    }
    return OCL_OK;
}

static int get_plans(ocl_net* n, int N, int groups, PlanSet** out) {
    auto key = std::make_pair(N, groups);
    auto it = n->plans.find(key);
    if (it != n->plans.end()) {
        *out = &it->second;
        return OCL_OK;
    }
    const auto t_plan0 = std::chrono::steady_clock::now();
    struct PlanLog {
        bool on; int N, groups; std::chrono::steady_clock::time_point t0; size_t* count;
        ~PlanLog() {
            if (on) fprintf(stderr, "[ocl] plan set %zu made for N=%d groups=%d: %.2f ms host\n", *count, N, groups,
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    };
    static size_t n_sets = 0;
    ++n_sets;
    PlanLog plog{log_plans(), N, groups, t_plan0, &n_sets};
    PlanSet ps;
    int rc = make_plan_set(n, N, groups, &ps);
    if (rc != OCL_OK) return rc;
    n->pack_need_fwd |= PACK_TF;
    for (auto& d : ps.dgrad)
        if (!d.empty()) n->pack_need_bwd |= PACK_TD;
    auto res = n->plans.emplace(key, std::move(ps));
    *out = &res.first->second;
    return OCL_OK;
}

// -----------------------------------------------------------------------------------------------------
// the two device tables of a network: one PackDesc per convolution, one BnFoldDesc per BatchNorm (also what ocl_test_pack_all / ocl_test_aux's
// bn_fold launch with, through net_test_tables)
static void make_descs(const ocl_net* n, std::vector<PackDesc>* pdv, std::vector<BnFoldDesc>* fdv) {
    std::vector<PackDesc>& pd = *pdv;
    std::vector<BnFoldDesc>& fd = *fdv;
    pd.assign(n->convs.size(), PackDesc());
    for (size_t i = 0; i < n->convs.size(); ++i) {
        const ConvInfo& c = n->convs[i];
        pd[i].w_off = n->tensors[c.w_t].off;
        pd[i].tf_off = c.tf_off;
        pd[i].td_off = c.td_off;
        pd[i].Cout = c.Cout;
        pd[i].Cin = c.Cin;
        pd[i].ntaps = c.k * c.k;
        pd[i].CinP = c.CinT;
        pd[i].CoutP = c.CoutP;
        pd[i].CiP = c.CiP;
    }
    fd.assign(n->bns.size(), BnFoldDesc());
    for (size_t i = 0; i < n->bns.size(); ++i) {
        fd[i].gamma_off = n->tensors[n->bns[i].gamma_t].off;
        fd[i].beta_off = n->tensors[n->bns[i].beta_t].off;
        fd[i].stat_off = n->bns[i].stat_off;
        fd[i].out_off = n->bns[i].stat_off;
        fd[i].C = n->bns[i].C;
    }
}
// (the grid of the pack launch is sized for the largest layer)
static int pack_max_elems(const ocl_net* n) {
    int max_elems = 0;
    for (auto& c : n->convs) max_elems = std::max(max_elems, c.Cout * c.Cin * c.k * c.k);
    return max_elems;
}
static int upload_descs(ocl_net* n, hipStream_t s) {
    std::vector<PackDesc> pd;
    std::vector<BnFoldDesc> fd;
    make_descs(n, &pd, &fd);
    unsigned char* dst = n->ws + n->off_descs;
    OCL_HIP(hipMemcpyAsync(dst, pd.data(), pd.size() * sizeof(PackDesc), hipMemcpyHostToDevice, s));
    OCL_HIP(hipMemcpyAsync(dst + align_up((int64_t)(pd.size() * sizeof(PackDesc)), 64), fd.data(), fd.size() * sizeof(BnFoldDesc),
                           hipMemcpyHostToDevice, s));
    OCL_HIP(hipMemsetAsync(n->ws + n->off_pack, 0, n->pack_floats * 4, s));
    OCL_HIP(hipStreamSynchronize(s));  // host vectors go out of scope
    n->descs_uploaded = true;
    return OCL_OK;
}
// the pack arena now holds the layouts `mask` (PACK_* bits) of the weights in P, written on stream s
static void note_packed(ocl_net* n, const float* P, int mask, hipStream_t s) {
    n->pack_src = P;
    n->pack_have = mask;
    n->pack_stream = s;
}
static const PackDesc* pack_descs(const ocl_net* n) { return (const PackDesc*)(n->ws + n->off_descs); }
static const BnFoldDesc* fold_descs(const ocl_net* n) {
    return (const BnFoldDesc*)(n->ws + n->off_descs + align_up((int64_t)(n->convs.size() * sizeof(PackDesc)), 64));
}

// the BatchNorm whose backward starts in a data gradient's epilogue (ConvArgs::bnb_*, EPI_BNB)
struct BnbEpi {
    const float *y, *z, *mean, *invstd, *gamma, *beta;
    StatCell* sums;          // [kStatReps][G][2][C], replica stride rep_stride cells, zeroed
    int64_t rep_stride;
};

// the producer-side BatchNorm a convolution applies to its own input (ConvArgs::xf)
struct XfBn {
    const StatCell* stats;
    const float *gamma, *beta;
    float *save_mean, *save_invstd, *running_mean, *running_var;
    int64_t* nbt;
    int64_t m_per_group;
};

static int run_conv(ocl_net* n, ConvPlan& cached, const float* in, const float* wT, float* out, int flags, StatCell* stats,
                    const float* scale, const float* shift, const float* res, const float* resmask, hipStream_t s, const XfBn* xf = nullptr,
                    const BnbEpi* be = nullptr) {
    if (!cached.a.blob) {   // first launch of this plan: its tables go to the device, on this stream, in front of the launch
        int rc = conv_plan_finalize(&cached, &n->plan_arena, s);
        if (rc != OCL_OK) return rc;
    }
    // the tables were uploaded asynchronously on the stream of the plan's first launch: any other stream (the side stream's projection
    // shortcuts, a different caller stream) orders itself behind that copy
    if (cached.ready && s != cached.ready_stream && !n->capturing) OCL_HIP(hipStreamWaitEvent(s, cached.ready, 0));
    ConvPlan p = cached;
    if (xf) {
        p.a.xf = 1;
        p.a.xf_stats = xf->stats;
        p.a.xf_rep_stride = n->stats_rep_stride;
        p.a.xf_m_per_group = xf->m_per_group;
        p.a.xf_gamma = xf->gamma; p.a.xf_beta = xf->beta;
        p.a.xf_save_mean = xf->save_mean; p.a.xf_save_invstd = xf->save_invstd;
        p.a.xf_running_mean = xf->running_mean; p.a.xf_running_var = xf->running_var; p.a.xf_nbt = xf->nbt;
        p.a.xf_momentum = 0.1f; p.a.xf_eps = 1e-5f;
    }
    p.a.stat_rep_stride = n->stats_rep_stride;
    p.a.in = in;
    p.a.wT = wT;
    p.a.out = out;
    p.a.flags = flags;
    p.a.stats = stats;
    p.a.scale = scale;
    p.a.shift = shift;
    p.a.res = res;
    p.a.resmask = resmask;
    if (be) {
        if (p.a.bnb_lds < 0) {
            set_error("run_conv: plan has no room for the BatchNorm-backward epilogue");
            return OCL_ERR_STATE;
        }
        p.a.flags |= EPI_BNB;
        p.a.stats = be->sums;
        p.a.stat_rep_stride = be->rep_stride;
        p.a.bnb_y = be->y; p.a.bnb_z = be->z;
        p.a.bnb_mean = be->mean; p.a.bnb_invstd = be->invstd; p.a.bnb_gamma = be->gamma; p.a.bnb_beta = be->beta;
    }
    return launch_conv(p, s);
}

static int head_forward(ocl_net* n, const float* P, float* feat, float* h1, float* h2, float* norms, float* out, int N,
                        hipStream_t s, float* out2, bool* wrote_out2) {
    const int FD = n->feat_dim;
    auto T = [&](int t) { return P + n->tensors[t].off; };
    int rc = OCL_OK;
    switch (n->d.head) {
        case 0:
            rc = ocl_gemm_small(feat, FD, 1, T(n->t_linear_w), 1, FD, out, n->out_dim, N, n->out_dim, FD, T(n->t_linear_b), 0, 0, s);
            break;
        case 1:
            rc = ocl_gemm_small(feat, FD, 1, T(n->t_h0_w), 1, FD, h1, FD, N, FD, FD, T(n->t_h0_b), 1, 0, s);
            if (rc) return rc;
            rc = ocl_gemm_small(h1, FD, 1, T(n->t_h2_w), 1, FD, h2, n->out_dim, N, n->out_dim, FD, T(n->t_h2_b), 0, 0, s);
            if (rc) return rc;
            rc = launch_l2norm_fwd(h2, out, norms, N, n->out_dim, s, out2);
            *wrote_out2 = true;
            break;
        case 2:
            rc = ocl_gemm_small(feat, FD, 1, T(n->t_h2_w), 1, FD, h2, n->out_dim, N, n->out_dim, FD, T(n->t_h2_b), 0, 0, s);
            if (rc) return rc;
            rc = launch_l2norm_fwd(h2, out, norms, N, n->out_dim, s, out2);
            *wrote_out2 = true;
            break;
        default:
            rc = launch_l2norm_fwd(feat, out, norms, N, FD, s, out2);
            *wrote_out2 = true;
            break;
    }
    return rc;
}

// trailing layers of a large pass's backward handed to the weight-gradient stream one by one (OCL_WGRAD_FLUSH_TAIL; trunk_backward)
constexpr int kWgradFlushTail = 5;
// projection shortcut / head weight gradients on the side stream from 96 x 32 x 32 input pixels on (OCL_SIDE_EXTRA_MIN: A/B, profiles/r6_side_extra_ab.txt)
static const int kSideExtraMinBatch = env_int("OCL_SIDE_EXTRA_MIN", 96);

static int ensure_side_stream(ocl_net* n) {
    if (n->s2) return OCL_OK;
    {   // the weight gradients are needed by nobody until the optimiser step: their stream yields to the dependent chain when both
        // have workgroups to place
        int lo = 0, hi = 0;
        OCL_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least urgent (numerically greatest)
        OCL_HIP(hipStreamCreateWithPriority(&n->s2, hipStreamNonBlocking, lo));
    }
    for (int i = 0; i < ocl_net::kDyRing; ++i) OCL_HIP(hipEventCreateWithFlags(&n->ev_done[i], hipEventDisableTiming));
    OCL_HIP(hipEventCreateWithFlags(&n->ev_join, hipEventDisableTiming));
    OCL_HIP(hipEventCreateWithFlags(&n->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < 48; ++i) {   // rolling pool for side_wait / side_join; created up front: none during capture
        hipEvent_t e;
        OCL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        n->ev_ready.push_back(e);
    }
    return OCL_OK;
}

// the side stream waits for everything issued on `s` so far (rolling pool of events; a wait captures the event's state at the call)
static int side_wait(ocl_net* n, hipStream_t s) {
    hipEvent_t e = n->ev_ready[n->ev_next++ % n->ev_ready.size()];
    OCL_HIP(hipEventRecord(e, s));
    OCL_HIP(hipStreamWaitEvent(n->s2, e, 0));
    return OCL_OK;
}
// ... and `s` for everything issued on the side stream so far
static int side_join(ocl_net* n, hipStream_t s) {
    hipEvent_t e = n->ev_ready[n->ev_next++ % n->ev_ready.size()];
    OCL_HIP(hipEventRecord(e, n->s2));
    OCL_HIP(hipStreamWaitEvent(s, e, 0));
    return OCL_OK;
}

// The one stream predicate: a pass of `pixels` (images x input pixels) gives work to the side stream from min_batch x 32 x 32 on.  Debug
// stops and measurement runs (ocl_prof_enable, OCL_SINGLE_STREAM=1: per-kernel durations of the kernel alone) stay on one stream.
static bool side_stream_at(int64_t pixels, int min_batch, int dbg_stop) {
    static const bool env_single = env_on("OCL_SINGLE_STREAM");
    return dbg_stop < 0 && pixels >= (int64_t)min_batch * 1024 && !prof_on() && !env_single;
}
// kTwoStreamMinBatch: the smallest pass whose weight gradients leave the caller's stream
static bool two_streams_at(int64_t pixels, int dbg_stop) { return side_stream_at(pixels, kTwoStreamMinBatch, dbg_stop); }
// ... kSideExtraMinBatch: the smallest whose head dW / db go there as well (and, in the forward, the projection shortcuts)
static bool head_side_at(int64_t pixels, bool two_streams) { return two_streams && pixels >= (int64_t)kSideExtraMinBatch * 1024; }

// The tensors of the head's backward: the tape of head_forward, the incoming gradient, and where the stage gradients go.
struct HeadBwd {
    const float *feat, *h1, *out, *norms, *dout;
    float *dfeat, *dh1, *dh2;
};
// Head half of the backward (ocl_net_backward; ocl_test_head runs it on caller-supplied tensors): dL/dfeat from dL/dout, and the head's
// weight and bias gradients into the flat gradient array Gr (accumulate = 0: overwritten, encoder.linear of a SupConResNet zeroed).
// two_streams: the pass has a side stream (ensure_side_stream has run); the head's dW / db go there from kSideExtraMinBatch on.
static int head_backward(ocl_net* n, const float* P, float* Gr, const HeadBwd& t, int N, int accumulate, hipStream_t s, bool two_streams) {
    auto T = [&](int i) { return P + n->tensors[i].off; };
    auto GT = [&](int i) { return Gr + n->tensors[i].off; };
    const int FD = n->feat_dim, OD = n->out_dim;
    auto lin_bwd = [&](const float* dy, int ncol, const float* xin, int kin, int tw, int tb, float* dx) -> int {
        // y = x W^T + b, W [ncol, kin]
        const bool hs = head_side_at(in_pixels(n, N), two_streams);
        hipStream_t sw = hs ? n->s2 : s;
        int r = hs ? side_wait(n, s) : OCL_OK;   // dy is complete
        if (r) return r;
        if ((r = ocl_gemm_small(dy, 1, ncol, xin, kin, 1, GT(tw), kin, ncol, kin, N, nullptr, 0, accumulate, sw))) return r;  // dW = dy^T x
        if ((r = launch_colsum(dy, N, ncol, GT(tb), accumulate, sw))) return r;
        if (dx) r = ocl_gemm_small(dy, ncol, 1, T(tw), kin, 1, dx, kin, N, kin, ncol, nullptr, 0, 0, s);  // dx = dy W
        return r;
    };
    int rc = OCL_OK;
    if (n->d.head == 0) return lin_bwd(t.dout, OD, t.feat, FD, n->t_linear_w, n->t_linear_b, t.dfeat);
    if (!accumulate) {  // encoder.linear takes no part in SupConResNet.forward: its gradient is zero
        // (weight and bias are neighbours in the flat array: one fill)
        if ((rc = launch_fill(GT(n->t_linear_w), n->tensors[n->t_linear_w].numel + n->tensors[n->t_linear_b].numel, 0.f, s))) return rc;
    }
    if (n->d.head == 1) {
        if ((rc = launch_l2norm_bwd(t.out, t.norms, t.dout, t.dh2, N, OD, s))) return rc;
        if ((rc = lin_bwd(t.dh2, OD, t.h1, FD, n->t_h2_w, n->t_h2_b, t.dh1))) return rc;
        if ((rc = launch_relu_bwd(t.dh1, t.h1, t.dh1, (int64_t)N * FD, s))) return rc;
        return lin_bwd(t.dh1, FD, t.feat, FD, n->t_h0_w, n->t_h0_b, t.dfeat);
    }
    if (n->d.head == 2) {
        if ((rc = launch_l2norm_bwd(t.out, t.norms, t.dout, t.dh2, N, OD, s))) return rc;
        return lin_bwd(t.dh2, OD, t.feat, FD, n->t_h2_w, n->t_h2_b, t.dfeat);
    }
    return launch_l2norm_bwd(t.out, t.norms, t.dout, t.dfeat, N, FD, s);
}

// -----------------------------------------------------------------------------------------------------
// Launch-sequence replay.  `body` issues launches that depend only on `key` (every pointer it uses lies in the workspace or the bound
// parameter / gradient / statistics arrays) and touches no host state.  First sight of a key: ordinary launches (plans get their
// device tables, one-time queries run).  Second sight: the same launches under stream capture -> hipGraph -> instantiate -> launch.
// From then on: one hipGraphLaunch.  Any failure falls back to ordinary launches for that key.  Off unless OCL_GRAPH=1; never
// while profiling (per-kernel events) or under a debug stop.
// -----------------------------------------------------------------------------------------------------
static bool graph_enabled(const ocl_net* n) {
    static const bool env_graph = env_on("OCL_GRAPH");
    return env_graph && !prof_on() && n->dbg_stop < 0;
}
template <class F>
static int run_replayed(ocl_net* n, ocl_net::GraphKey key, hipStream_t s, F&& body) {
    if (!graph_enabled(n)) return body();
    static const bool verbose = env_on("OCL_GRAPH_VERBOSE");
    ocl_net::GraphSlot& g = n->graphs[key];
    if (g.exec) {
        OCL_HIP(hipGraphLaunch(g.exec, s));
        return OCL_OK;
    }
    if (g.failed || g.seen++ < 1) return body();
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) {
        if (verbose) fprintf(stderr, "ocl graph: begin-capture failed (kind %d N %d)\n", key.kind, key.N);
        (void)hipGetLastError();
        g.failed = true;
        return body();
    }
    n->capturing = true;
    const int rc = body();
    n->capturing = false;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (rc != OCL_OK || e != hipSuccess || !graph) {
        if (verbose) fprintf(stderr, "ocl graph: capture failed (kind %d N %d): body rc %d, end-capture %d (%s)\n", key.kind, key.N, rc, (int)e, hipGetErrorString(e));
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        g.failed = true;
        return rc != OCL_OK ? rc : body();
    }
    size_t n_nodes = 0;
    (void)hipGraphGetNodes(graph, nullptr, &n_nodes);
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
        if (verbose) fprintf(stderr, "ocl graph: instantiate failed (kind %d N %d): %s\n", key.kind, key.N, hipGetErrorString(ei));
        (void)hipGetLastError();
        g.exec = nullptr;
        g.failed = true;
        return body();
    }
    if (verbose) fprintf(stderr, "ocl graph: captured kind %d N %d G %d slot %d: %zu nodes\n", key.kind, key.N, key.G, key.slot, n_nodes);
    OCL_HIP(hipGraphLaunch(g.exec, s));
    return OCL_OK;
}

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

int ocl_net_create(const ocl_net_desc* desc, ocl_net** out) {
    OCL_REQUIRE(desc && out, "net_create: null pointer");
    OCL_REQUIRE(desc->in_h >= 32 && desc->in_w >= 32 && desc->nf > 0 && desc->nf % 4 == 0, "net_create: bad input size / nf");
    OCL_REQUIRE(desc->head >= 0 && desc->head <= 3, "net_create: head=%d", desc->head);
    OCL_REQUIRE(desc->n_classes > 0 && desc->max_batch > 0 && desc->n_slots >= 1, "net_create: n_classes/max_batch/n_slots");
    OCL_REQUIRE(desc->head == 0 || desc->head == 3 || desc->feat_dim > 0, "net_create: feat_dim");
    ocl_net* n = new ocl_net();
    n->d = *desc;
    int rc = build_layout(n);
    if (rc != OCL_OK) {
        delete n;
        return rc;
    }
    *out = n;
    return OCL_OK;
}

void ocl_net_destroy(ocl_net* net) {
    if (!net) return;
    for (auto& kv : net->graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    for (auto e : net->ev_ready) (void)hipEventDestroy(e);
    for (int i = 0; i < ocl_net::kDyRing; ++i)
        if (net->ev_done[i]) (void)hipEventDestroy(net->ev_done[i]);
    if (net->ev_join) (void)hipEventDestroy(net->ev_join);
    if (net->ev_fork) (void)hipEventDestroy(net->ev_fork);
    if (net->s2) (void)hipStreamDestroy(net->s2);
    plan_arena_release(&net->plan_arena);   // the plans' device tables
    for (auto& kv : net->wgrad_tables)
        for (auto& t : kv.second) wgrad_multi_release(&t);
    delete net;
}

int64_t ocl_net_param_count(const ocl_net* net) { return net ? net->n_params : -1; }
int32_t ocl_net_num_tensors(const ocl_net* net) { return net ? (int32_t)net->tensors.size() : -1; }
int ocl_net_tensor_info(const ocl_net* net, int i, char* name64, int64_t* offset, int32_t* ndim, int64_t* shape4) {
    OCL_REQUIRE(net && i >= 0 && i < (int)net->tensors.size(), "tensor_info: index %d", i);
    const TensorInfo& t = net->tensors[i];
    if (name64) {
        strncpy(name64, t.name.c_str(), 63);
        name64[63] = 0;
    }
    if (offset) *offset = t.off;
    if (ndim) *ndim = t.ndim;
    if (shape4)
        for (int k = 0; k < 4; ++k) shape4[k] = t.shape[k];
    return OCL_OK;
}
int32_t ocl_net_num_bn(const ocl_net* net) { return net ? (int32_t)net->bns.size() : -1; }
int64_t ocl_net_bn_stat_count(const ocl_net* net) { return net ? net->n_stats : -1; }
int ocl_net_bn_info(const ocl_net* net, int i, char* name64, int64_t* offset, int32_t* channels) {
    OCL_REQUIRE(net && i >= 0 && i < (int)net->bns.size(), "bn_info: index %d", i);
    if (name64) {
        strncpy(name64, net->bns[i].name.c_str(), 63);
        name64[63] = 0;
    }
    if (offset) *offset = net->bns[i].stat_off;
    if (channels) *channels = net->bns[i].C;
    return OCL_OK;
}
int32_t ocl_net_feature_dim(const ocl_net* net) { return net ? net->feat_dim : -1; }
int32_t ocl_net_out_dim(const ocl_net* net) { return net ? net->out_dim : -1; }
int64_t ocl_net_workspace_bytes(const ocl_net* net) { return net ? net->ws_bytes : -1; }

int ocl_net_bind(ocl_net* net, float* params, float* grads, float* running, int64_t* nbt, void* workspace, int64_t workspace_bytes) {
    OCL_REQUIRE(net && params && grads && running && nbt && workspace, "net_bind: null pointer");
    OCL_REQUIRE(workspace_bytes >= net->ws_bytes, "net_bind: workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)net->ws_bytes);
    OCL_REQUIRE(((uintptr_t)workspace % 256) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)grads % 16) == 0,
                "net_bind: alignment (workspace 256 B, params/grads 16 B)");
    int rc = conv_kernels_init();
    if (rc != OCL_OK) return rc;
    net->params = params;
    net->grads = grads;
    net->running = running;
    net->nbt = nbt;
    net->ws = (unsigned char*)workspace;
    net->bound = true;
    net->descs_uploaded = false;
    net->pack_src = nullptr;
    for (size_t i = 0; i < net->slot_valid.size(); ++i) net->slot_valid[i] = false;
    // captured launch sequences hold the previous binding's workspace / gradient / statistics pointers
    for (auto& kv : net->graphs)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    net->graphs.clear();
    return OCL_OK;
}

}  // extern "C"

// the unbound one-slot net of the test hooks (layout, plans and head only; the caller destroys it)
static int make_test_net(int hw, int nf, int n_classes, int head, int feat_dim, int max_batch, ocl_net** out) {
    ocl_net_desc d;
    memset(&d, 0, sizeof(d));
    d.in_h = d.in_w = hw; d.nf = nf; d.n_classes = n_classes; d.head = head; d.feat_dim = feat_dim; d.max_batch = max_batch; d.n_slots = 1;
    return ocl_net_create(&d, out);
}

// -----------------------------------------------------------------------------------------------------
// Train-mode trunk: images [0, Nc) of the batch as G BatchNorm groups, every launch on `st`.  upd: update the running statistics
// inside the BatchNorm kernels (once per group, in group order = the reference's separate forward calls).  side: the projection
// shortcuts run on the engine's second stream.  frozen: BatchNorm normalises with the running statistics (eval-mode tape).
// -----------------------------------------------------------------------------------------------------
// Measurement only, like OCL_DEBUG_SKIP_WGRAD (results are WRONG with either set; scripts/gpu_r6bb.sh): upper bounds of what two launch
// folds the reviews asked for could return -- OCL_DEBUG_SKIP_BN2FWD=1: no bn_fwd_kernel launch behind conv2 of the seven non-final blocks
// (the fold of bn2 + residual + ReLU into the next conv1's staging would still have to read y2 and the residual and write z there);
// OCL_DEBUG_SKIP_SHORTCUT=1: no projection-shortcut convolution, data gradient or weight gradient (the fold into the block's 3x3
// stride-2 convolution keeps their arithmetic).
static bool dbg_skip_bn2fwd() {
    static const bool v = env_on("OCL_DEBUG_SKIP_BN2FWD");
    return v;
}
static bool dbg_skip_shortcut() {
    static const bool v = env_on("OCL_DEBUG_SKIP_SHORTCUT");
    return v;
}

static int trunk_forward_train(ocl_net* n, PlanSet* ps, const float* P, float* S, int Nc, int G, bool upd, float* feat, hipStream_t st,
                               bool side = false, bool frozen = false, bool fuse = false) {
    float* pack = (float*)(n->ws + n->off_pack);
    int rc = OCL_OK;
    auto view = [&](int conv_i) { return bn_view(n, P, nullptr, S, n->convs[conv_i].bn); };
    // side: the projection shortcut's 1x1 convolution (3 blocks) runs on the engine's second stream next to conv1 / bn1 / conv2 of its
    // block, which do not depend on it
    // conv_b >= 0: the projection shortcut whose BatchNorm output is this BatchNorm's residual, normalised in the same launch
    auto bn_fwd = [&](int conv_i, const float* y, float* z, const float* res, int relu, hipStream_t st, int conv_b = -1) -> int {
        const ConvInfo& c = n->convs[conv_i];
        const BnView v = view(conv_i);
        BnFwdArgs a;
        memset(&a, 0, sizeof(a));
        a.y = y; a.z = z; a.res = res;
        a.stats = v.stats;   // (cleared by the forward's weight-pack launch)
        a.stat_rep_stride = n->stats_rep_stride;
        a.gamma = v.gamma; a.beta = v.beta;
        a.running_mean = upd ? v.running_mean : nullptr;
        a.running_var = upd ? v.running_var : nullptr;
        a.nbt = upd ? v.nbt : nullptr;
        a.save_mean = v.save_mean; a.save_invstd = v.save_invstd;
        a.m_per_group = (int64_t)(Nc / G) * c.Ho * c.Wo;
        a.G = G; a.C = v.C; a.relu = relu;
        a.momentum = 0.1f; a.eps = 1e-5f;
        if (frozen) { a.frozen_mean = v.running_mean; a.frozen_var = v.running_var; }
        if (conv_b >= 0) {
            const BnView w = view(conv_b);
            a.yb = S + n->convs[conv_b].y_off;
            a.stats_b = w.stats;
            a.gamma_b = w.gamma; a.beta_b = w.beta;
            a.running_mean_b = upd ? w.running_mean : nullptr;
            a.running_var_b = upd ? w.running_var : nullptr;
            a.nbt_b = upd ? w.nbt : nullptr;
            a.save_mean_b = w.save_mean; a.save_invstd_b = w.save_invstd;
            if (frozen) { a.frozen_mean_b = w.running_mean; a.frozen_var_b = w.running_var; }
        }
        return launch_bn_fwd(a, st);
    };
    auto conv_stats = [&](int conv_i, const float* in, hipStream_t st, const XfBn* xf = nullptr) -> int {
        const ConvInfo& c = n->convs[conv_i];
        return run_conv(n, ps->fwd[conv_i], in, pack + c.tf_off, S + c.y_off, EPI_STATS, view(conv_i).stats, nullptr, nullptr, nullptr, nullptr, st, xf);
    };
    const ConvInfo& c0 = n->convs[0];
    if ((rc = conv_stats(0, S + n->x4_off, st))) return rc;
    float* cur = S + n->zstem_off;
    if ((rc = bn_fwd(0, S + c0.y_off, cur, nullptr, 1, st))) return rc;
    for (auto& b : n->blocks) {
        const ConvInfo& c1 = n->convs[b.conv1];
        const ConvInfo& c2 = n->convs[b.conv2];
        float* a1 = S + b.a1_off;
        float* z = S + b.z_off;
        const float* res = cur;
        if (b.convs >= 0) {
            hipStream_t ss = side ? n->s2 : st;
            if (side && (rc = side_wait(n, st))) return rc;       // `cur` (and the zeroed statistics) are ready
            // (its BatchNorm is applied by the block's last BatchNorm launch below: z = relu(bn2(y2) + bn_s(ys)), one launch for both)
            if (!dbg_skip_shortcut() && (rc = conv_stats(b.convs, cur, ss))) return rc;
            res = nullptr;
        }
        if ((rc = conv_stats(b.conv1, cur, st))) return rc;
        if (fuse) {
            // relu(bn1(.)) is applied by conv2 while it stages its patches: no BatchNorm launch, a1 is never written (the backward
            // recomputes it where it needs it: weight gradient of conv2, ReLU mask of bn1's backward)
            const BnView v = view(b.conv1);
            XfBn xf;
            xf.stats = v.stats;
            xf.gamma = v.gamma; xf.beta = v.beta;
            xf.save_mean = v.save_mean; xf.save_invstd = v.save_invstd;
            xf.running_mean = upd ? v.running_mean : nullptr;
            xf.running_var = upd ? v.running_var : nullptr;
            xf.nbt = upd ? v.nbt : nullptr;
            xf.m_per_group = (int64_t)(Nc / G) * c1.Ho * c1.Wo;
            if ((rc = conv_stats(b.conv2, S + c1.y_off, st, &xf))) return rc;
        } else {
            if ((rc = bn_fwd(b.conv1, S + c1.y_off, a1, nullptr, 1, st))) return rc;
            if ((rc = conv_stats(b.conv2, a1, st))) return rc;
        }
        if (b.convs >= 0 && side && (rc = side_join(n, st))) return rc;
        if (!(dbg_skip_bn2fwd() && &b != &n->blocks.back()) && (rc = bn_fwd(b.conv2, S + c2.y_off, z, res, 1, st, b.convs))) return rc;
        cur = z;
    }
    if (!feat) return OCL_OK;   // (a pass run for its running-statistic updates alone)
    return launch_avgpool_fwd(cur, feat, Nc, n->Hf, n->Wf, n->convs[n->blocks.back().conv2].Cout, st);
}

// Eval-mode trunk: every BatchNorm folded to a scale and a shift (from the running statistics) that its convolution's epilogue applies; no
// tape, the activations rotate through four scratch buffers.  `ps` may be planned for more than N images (ocl_net_forward_segments).
static int trunk_forward_eval(ocl_net* n, PlanSet* ps, const float* P, const float* x4, int N, float* feat, hipStream_t s) {
    float* pack = (float*)(n->ws + n->off_pack);
    float* fold = (float*)(n->ws + n->off_fold);   // scale[C], shift[C] per BatchNorm, laid out like the running statistics
    int rc = launch_bn_fold(P, n->running, fold, fold_descs(n), (int)n->bns.size(), 1e-5f, s);
    if (rc) return rc;
    auto conv_eval = [&](int conv_i, const float* in, float* o, const float* res, int relu) -> int {
        const ConvInfo& c = n->convs[conv_i];
        const BnInfo& b = n->bns[c.bn];
        int fl = EPI_AFFINE | (res ? EPI_RES : 0) | (relu ? EPI_RELU : 0);
        return run_conv(n, ps->fwd[conv_i], in, pack + c.tf_off, o, fl, nullptr, fold + b.stat_off, fold + b.stat_off + b.C, res, nullptr, s);
    };
    float* bufs[4] = {n->gbuf(0), n->gbuf(1), n->gbuf(2), n->gbuf(3)};
    float* cur = bufs[0];
    if ((rc = conv_eval(0, x4, cur, nullptr, 1))) return rc;
    int ci = 0;
    for (auto& b : n->blocks) {
        float* a1 = bufs[(ci + 1) & 3];
        float* sc = bufs[(ci + 2) & 3];
        float* z = bufs[(ci + 3) & 3];
        if ((rc = conv_eval(b.conv1, cur, a1, nullptr, 1))) return rc;
        const float* res = cur;
        if (b.convs >= 0) {
            if ((rc = conv_eval(b.convs, cur, sc, nullptr, 0))) return rc;
            res = sc;
        }
        if ((rc = conv_eval(b.conv2, a1, z, res, 1))) return rc;
        cur = z;
        ci = (ci + 3) & 3;
    }
    return launch_avgpool_fwd(cur, feat, N, n->Hf, n->Wf, n->convs[n->blocks.back().conv2].Cout, s);
}

extern "C" {

int ocl_net_forward(ocl_net* n, const float* x, int N, int groups, uint32_t flags, const float* params_override, float* feat_out,
                    float* out, int slot, void* stream) {
    OCL_REQUIRE(x, "net_forward: null input");
    const float* xs[1] = {x};
    const int32_t ns[1] = {N};
    return ocl_net_forward_segments(n, xs, ns, 1, groups, flags, params_override, feat_out, out, slot, stream);
}

int ocl_net_forward_segments(ocl_net* n, const float* const* xs, const int32_t* ns, int nseg, int groups, uint32_t flags,
                             const float* params_override, float* feat_out, float* out, int slot, void* stream) {
    OCL_REQUIRE(n && n->bound, "net_forward: net not bound");
    if (int arc = check_async_error("net_forward")) return arc;
    OCL_REQUIRE(xs && ns && nseg >= 1 && nseg <= kMaxInputSegments, "net_forward: %d input segments (1 .. %d)", nseg, kMaxInputSegments);
    InputSegments sg;
    memset(&sg, 0, sizeof(sg));
    int N = 0;
    for (int i = 0; i < nseg; ++i) {
        OCL_REQUIRE(xs[i] && ns[i] > 0, "net_forward: segment %d is empty", i);
        sg.x[i] = xs[i];
        sg.first[i] = N;
        N += ns[i];
    }
    sg.n = nseg;
    OCL_REQUIRE(N > 0 && N <= n->d.max_batch, "net_forward: n=%d (max_batch %d)", N, n->d.max_batch);
    OCL_REQUIRE(groups >= 1 && groups <= kGmax && N % groups == 0, "net_forward: groups=%d must divide n=%d (<= %d)", groups, N, kGmax);
    OCL_REQUIRE(slot >= 0 && slot < n->d.n_slots, "net_forward: slot %d", slot);
    hipStream_t s = (hipStream_t)stream;
    const bool frozen = (flags & OCL_FWD_FROZEN_BN) != 0;   // eval-mode BatchNorm, activations kept for ocl_net_backward
    OCL_REQUIRE(!frozen || ((flags & OCL_FWD_SAVE_TAPE) && !(flags & (OCL_FWD_TRAIN | OCL_FWD_UPDATE_RUNNING)) && groups == 1),
                "net_forward: OCL_FWD_FROZEN_BN goes with OCL_FWD_SAVE_TAPE only, one group");
    const bool train = (flags & OCL_FWD_TRAIN) != 0 || frozen;   // frozen: the train-mode kernel sequence with constant statistics
    OCL_REQUIRE(train || groups == 1, "net_forward: groups only apply to train-mode BatchNorm");
    if (!n->descs_uploaded) {
        int rc = upload_descs(n, s);
        if (rc != OCL_OK) return rc;
    }
    const float* P = params_override ? params_override : n->params;
    PlanSet* ps = nullptr;
    // Eval-mode passes have no cross-image terms (folded BatchNorm): their plans are made for the batch rounded up to 16 images (the
    // extra images are whatever the activation buffers hold; nothing reads their outputs), so the evaluation sets of the ASER update,
    // whose size changes from step to step, share a handful of plan sets instead of planning a new one almost every step.
    // (buckets of 4 up to 16 images: a 1 - 4 image pass is not padded to 16x its work)
    const int Nplan = train ? N : std::min(n->d.max_batch, N <= 16 ? (N + 3) / 4 * 4 : (N + 15) / 16 * 16);
    int rc = get_plans(n, Nplan, train ? groups : 1, &ps);
    if (rc != OCL_OK) return rc;
    float* pack = (float*)(n->ws + n->off_pack);
    const int max_elems = pack_max_elems(n);
    // every forward packs (the caller may have stepped the weights), but only the layouts the pass reads: the forward packs, and the
    // data-gradient packs when a backward will follow this tape
    // (OCL_FWD_PACK_ALL: the caller will run more passes on these weights, a taped one among them: pack for the backward now as well)
    // (a refused OCL_FWD_SAME_WEIGHTS counts as the same hint: the caller is inside a block of passes on one set of weights)
    const int pack_mask = n->pack_need_fwd | ((flags & (OCL_FWD_SAVE_TAPE | OCL_FWD_PACK_ALL | OCL_FWD_SAME_WEIGHTS)) ? n->pack_need_bwd : 0);
    // OCL_FWD_SAME_WEIGHTS: the packs of the previous forward are still those of this array -- no pack launch; a train-mode pass
    // clears its statistics arenas (the pack launch's other job) with one memset over both, an eval-mode pass needs nothing
    const bool same_weights = (flags & OCL_FWD_SAME_WEIGHTS) && n->pack_src == P && (n->pack_have & pack_mask) == pack_mask && n->pack_stream == s;

    float* S = n->slotf(slot);
    float* x4 = S + n->x4_off;
    // (the only launch that reads caller memory: in front of the replayable sequence)
    rc = launch_nchw3_to_nhwc4_segments(sg, x4, N, n->d.in_h, n->d.in_w, s);
    if (rc != OCL_OK) return rc;
    n->slot_valid[slot] = false;

    const bool replay = graph_enabled(n);
    // features only (ASER scoring, NCM): straight into the caller's array, no copy (a replayed sequence writes the slot's own array)
    const bool feat_direct = feat_out && !out && !(flags & OCL_FWD_SAVE_TAPE) && !replay;
    float* feat = feat_direct ? feat_out : S + n->feat_off;
    const bool upd = (flags & OCL_FWD_UPDATE_RUNNING) != 0;
    // (threshold in images x input pixels: MIR's 50-image 84 x 84 passes qualify, 5.05 -> 4.99 ms per step)
    const bool side = train && side_stream_at(in_pixels(n, N), kSideExtraMinBatch, n->dbg_stop);
    if (side && (rc = ensure_side_stream(n))) return rc;
    const bool fused = train && !frozen;
    const bool want_head = out || (flags & OCL_FWD_SAVE_TAPE);
    float* head_out2 = replay ? nullptr : out;   // the head's last kernel writes the caller's array as well (not when replayed)
    bool wrote = false;

    // ---- the launch sequence (everything below depends only on the key: shapes, slot, flags, parameter array) -----------------------
    auto body = [&]() -> int {
        int rc = OCL_OK;
        if (!same_weights) {
            rc = launch_pack_weights(P, pack, pack_descs(n), (int)n->convs.size(), max_elems, s, pack_mask, n->statsbuf(), n->stats_doubles,
                                     n->bsumsbuf(), n->bsums_doubles);   // (also clears the statistics arenas of the pass and of its backward)
            if (rc != OCL_OK) return rc;
        } else if (train) {   // the two arenas are neighbours in the workspace: one clear from the first cell of one to the last of the other
            unsigned char* lo = n->ws + std::min(n->off_stats, n->off_bsums);
            unsigned char* hi = n->ws + std::max(n->off_stats + n->stats_doubles * (int64_t)sizeof(StatCell),
                                                 n->off_bsums + n->bsums_doubles * (int64_t)sizeof(StatCell));
            OCL_HIP(hipMemsetAsync(lo, 0, (size_t)(hi - lo), s));
        }
        rc = train ? trunk_forward_train(n, ps, P, S, N, groups, upd && !frozen, (feat_out || want_head) ? feat : nullptr, s, side, frozen, fused)
                   : trunk_forward_eval(n, ps, P, x4, N, feat, s);
        if (rc != OCL_OK) return rc;
        if (want_head && (rc = head_forward(n, P, feat, S + n->h1_off, S + n->h2_off, S + n->norms_off, S + n->out_off, N, s, head_out2, &wrote)))
            return rc;
        return OCL_OK;
    };
    ocl_net::GraphKey key;
    memset(&key, 0, sizeof(key));
    key.kind = 0; key.N = N; key.G = groups; key.slot = slot; key.a = (int)flags; key.b = pack_mask;
    key.c = (want_head ? 1 : 0) | (feat == S + n->feat_off ? 2 : 0) | (same_weights ? 4 : 0) | ((feat_out || want_head) ? 8 : 0);
    key.p = (uint64_t)(uintptr_t)P;
    // (sequences that fork to the side stream are not replayed: as a graph the SCR pass ran at 4.2 ms per step against 2.35 with
    // stream launches -- profiles/r4_graph_replay.txt -- while a single-stream ER pass keeps its GPU time and halves the host's)
    rc = side ? body() : run_replayed(n, key, s, body);
    // host state of the pass (also when the launches were replayed)
    if (!same_weights || train) n->bsums_clean = true;
    // A pack launch wrote exactly `pack_mask` from the array's CURRENT contents; whatever else the arena held for the same pointer may be
    // from before an optimiser step and counts as gone (round 5: with OCL_FWD_SAME_WEIGHTS a stale data-gradient pack would otherwise
    // be trusted by the next taped forward -- the bug tests/test_gpu_net.py::test_same_weights_... now pins)
    if (!same_weights) note_packed(n, P, pack_mask, s);
    if (rc != OCL_OK) return rc;
    if (train) {
        n->slot_fused[slot] = fused;
        n->slot_n[slot] = N;
        n->slot_groups[slot] = groups;
    }
    if (feat_out && !feat_direct) OCL_HIP(hipMemcpyAsync(feat_out, feat, (size_t)N * n->feat_dim * 4, hipMemcpyDeviceToDevice, s));
    if (out && want_head && !(wrote && head_out2))
        OCL_HIP(hipMemcpyAsync(out, S + n->out_off, (size_t)N * n->out_dim * 4, hipMemcpyDeviceToDevice, s));
    if (train && (flags & OCL_FWD_SAVE_TAPE) && !params_override) {
        n->slot_valid[slot] = true;
        n->slot_frozen[slot] = frozen;
        n->slot_n[slot] = N;
        n->slot_groups[slot] = groups;
    }
    return OCL_OK;
}

}  // extern "C"

// -----------------------------------------------------------------------------------------------------
// Backward of the trunk: from dL/dfeat to the parameter gradients in Gr (overwritten or accumulated).  side != null: the weight
// gradients go to that stream behind events (large batches); null: everything on `s`, in order (small batches, measurements).
// -----------------------------------------------------------------------------------------------------
static int trunk_backward(ocl_net* n, PlanSet* ps, const float* P, float* Gr, float* S, int Nc, int G, int accumulate, const float* dfeat,
                          hipStream_t s, hipStream_t side, bool frozen = false, bool fused = false) {
    float* pack = (float*)(n->ws + n->off_pack);
    float* partial = n->partialbuf();
    int rc = OCL_OK;
    if (!n->bsums_clean) OCL_HIP(hipMemsetAsync(n->bsumsbuf(), 0, n->bsums_doubles * sizeof(StatCell), s));   // a second backward since the last forward
    n->bsums_clean = false;
    auto GT = [&](int t) { return Gr + n->tensors[t].off; };
    auto view = [&](int conv_i) { return bn_view(n, P, Gr, S, n->convs[conv_i].bn); };
    const float* x4 = S + n->x4_off;
    float* gA = n->gbuf(0);  // grad wrt current block output
    float* gD = n->gbuf(3);
    float* gE = n->gbuf(4);
    float* gB = nullptr;         // dL/dy of the main-path BatchNorm being processed (ring slot)
    float* gC = nullptr;         // dL/dy of the projection-shortcut BatchNorm
    const int Clast = n->convs[n->blocks.back().conv2].Cout;
    if ((rc = launch_avgpool_bwd(dfeat, gA, Nc, n->Hf, n->Wf, Clast, s))) return rc;

    const bool two_streams = side != nullptr;
    hipStream_t sw = two_streams ? side : s;   // stream of the weight gradients
    n->dy_next = 0;
    for (int i = 0; i < ocl_net::kDyRing; ++i) n->ev_done_pending[i] = false;
    // one stream (replay-sized batches: bound by the number of dependent launches): every layer writes its slabs into its own region
    // and ONE launch at the end of the backward reduces them all
    // (with a side stream too: the small launches of a replay-sized backward leave most of the machine idle, so the weight gradients
    // run BESIDE the dependent chain there, each layer into its own slab region, and one launch at the end reduces them all)
    const bool batched = Nc < kTwoStreamMinBatch && ps->batched_reduce && n->dbg_stop < 0;
    // ... and on one stream the weight gradients themselves wait for the end: every dL/dy stays in its own buffer, and the layers leave in
    // one launch per form set (conv_wgrad_multi_kernel) in front of the one reduction: 20 launches of the dependent chain -> 1 or 2
    static const bool env_multi = env_not_off("OCL_WGRAD_MULTI");
    int n_dy = 1;
    for (auto& b : n->blocks) n_dy += b.convs >= 0 ? 3 : 2;
    const bool defer = env_multi && batched && !two_streams && !n->capturing && n_dy <= ocl_net::kDyKeep;
    // Two streams: with one dL/dy buffer per layer as well, the dependent chain never waits for the weight-gradient stream to hand a ring
    // slot back (and records no event per layer for it) -- OCL_DY_KEEP=0: the ring of kDyRing buffers
    static const bool env_keep = env_not_off("OCL_DY_KEEP");
    const bool keep = defer || (env_keep && two_streams && n_dy <= ocl_net::kDyKeep);
    // ... and the weight-gradient stream is told about new dL/dy buffers every OCL_WGRAD_FLUSH layers (an event record on the chain's stream +
    // a wait on the other per hand-over): it lags behind the chain anyway
    // (SCR's 220 views: ring 2.025 ms, per-layer buffers 2.005, + hand-over every 2 / 3 / 5 / 10 / 21 layers 2.000 / 1.990 / 2.054 / 2.109 /
    // 2.256 -- the sooner the other stream has work, the more of it hides; MIR's 50 - 60-image passes: 4.614 / 4.545 / 4.603 at 3:
    // profiles/r6_dy_keep_flush_ab.txt.  Three layers per hand-over from 128 images on.)
    static const int env_flush = env_int("OCL_WGRAD_FLUSH", INT_MIN);   // (INT_MIN: unset)
    const int flush_every = env_flush != INT_MIN ? std::max(1, env_flush) : (Nc >= 128 ? 3 : 1);
    const bool coarse = two_streams && keep && flush_every > 1;
    // ... except at the end of the backward, where the chain is short of what the other stream still has to do: the last
    // OCL_WGRAD_FLUSH_TAIL layers (in backward order; the stem, which stays on the caller's stream, is the last of them) are handed over
    // one by one, each as soon as its dL/dy exists, and the last hand-over is issued in front of the stem's BatchNorm backward instead
    // of behind it.  0: groups of flush_every to the end, the last one behind the stem's BatchNorm backward.
    static const int env_tail = std::max(0, env_int("OCL_WGRAD_FLUSH_TAIL", kWgradFlushTail));
    const int tail_from = coarse ? n_dy - env_tail : n_dy;   // first layer, in backward order, that is handed over on its own
    int n_handed = 0;
    std::vector<WgradPlan> deferred;
    // next dL/dy buffer: the layer's own, or the next ring slot (*slot_out, for release; the main stream waits for its previous readers)
    auto take_dy = [&](int* slot_out = nullptr) -> float* {
        if (keep) return n->dykeep(n->dy_next++);
        const int r = n->dy_next;
        n->dy_next = (r + 1) % ocl_net::kDyRing;
        if (two_streams && n->ev_done_pending[r]) {
            (void)hipStreamWaitEvent(s, n->ev_done[r], 0);
            n->ev_done_pending[r] = false;
        }
        if (slot_out) *slot_out = r;
        return n->dybuf(r);
    };
    auto publish = [&]() -> int {   // everything the main stream has written so far is visible to the wgrad stream
        return two_streams && !coarse ? side_wait(n, s) : OCL_OK;
    };
    auto release = [&](int r) -> int {   // the wgrad stream is done reading ring slot r
        if (!two_streams || keep) return OCL_OK;
        OCL_HIP(hipEventRecord(n->ev_done[r], sw));
        n->ev_done_pending[r] = true;
        return OCL_OK;
    };

    // zmask == nullptr with from_y: the activation behind this BatchNorm was never written (fused forward): mask from the raw output
    auto bn_bwd = [&](const float* dz, const float* zmask, int conv_a, float* dya, int conv_b, float* dyb, bool from_y = false) -> int {
        BnBwdArgs a;
        memset(&a, 0, sizeof(a));
        const ConvInfo& ca = n->convs[conv_a];
        a.dz = dz; a.z = zmask;
        a.mask_from_y = from_y ? 1 : 0;
        a.m_per_group = (int64_t)(Nc / G) * ca.Ho * ca.Wo;
        a.G = G; a.C = ca.Cout;
        a.nsets = conv_b >= 0 ? 2 : 1;
        const int cs[2] = {conv_a, conv_b};
        float* dys[2] = {dya, dyb};
        for (int k = 0; k < a.nsets; ++k) {
            const BnView v = view(cs[k]);
            a.y[k] = S + n->convs[cs[k]].y_off;
            a.mean[k] = v.save_mean; a.invstd[k] = v.save_invstd;
            a.gamma[k] = v.gamma; a.beta[k] = v.beta;
            a.dy[k] = dys[k];
            a.dgamma[k] = v.dgamma; a.dbeta[k] = v.dbeta;
        }
        // sums are addressed [set][G][2][C] inside conv_a's arena of 2*kGmax*2*C cells: two sets fit at every G <= kGmax
        const BnView va = view(conv_a);
        a.sums = va.bsums;
        // one-pass kernel (<= 2 groups; two BatchNorms sharing dz each bring their own accumulator arena)
        if (G <= 2) {
            a.fsums = va.fsums;
            a.barrier = va.barrier;
            if (conv_b >= 0) a.fsums_b = view(conv_b).fsums;
        }
        a.accumulate = accumulate;
        a.frozen = frozen ? 1 : 0;
        return launch_bn_bwd(a, s);
    };
    WgradReduceMulti rm;
    rm.partial = partial; rm.grads = Gr; rm.accumulate = accumulate; rm.n = 0;
    // Large passes: four layers write their slabs into regions of 12 MB side by side -- plan_wgrad caps a layer's split at that -- and ONE
    // launch reduces them (20 reductions of 4 - 6 us on the weight-gradient stream -> 5; same reduction body: same bits; the 220-view
    // pass 1978 -> 1953 us, groups of two 1965: profiles/r5_wgrad_switches.txt); the stem's region (see below) lies behind them.
    constexpr int64_t kGroupRegion = 12ll << 20;
    constexpr int group_k = 4;
    const bool grouped = !batched && n->dbg_stop < 0 && (int64_t)(group_k + 1) * kGroupRegion <= n->partial_floats * 4;
    const int64_t stem_region = grouped ? (int64_t)group_k * kGroupRegion : (16ll << 20);   // bytes from `partial`
    // xf_conv >= 0: xin is the RAW output of that convolution; its BatchNorm + ReLU is applied while the kernel stages its patches
    // measurement only (OCL_DEBUG_SKIP_WGRAD=1: the gradients of the convolution weights are NOT computed): the wall time of the dependent
    // chain alone; step time - that = the weight-gradient time the second stream does not hide (bench.py --exposed-wgrad)
    static const bool env_skip_wgrad = env_on("OCL_DEBUG_SKIP_WGRAD");
    auto flush_reduce = [&](hipStream_t st) -> int {   // one launch reduces the slabs of the layers gathered in `rm`
        const int r = rm.n > 0 ? launch_wgrad_reduce_multi(rm, st) : OCL_OK;
        if (!r) rm.n = 0;
        return r;
    };
    struct PendingWgrad { int conv_i; const float* xin; const float* dy; int xf_conv; };
    std::vector<PendingWgrad> pending;
    auto wgrad_now = [&](int conv_i, const float* xin, const float* dy, int xf_conv = -1) -> int {   // on the weight-gradient stream
        if (env_skip_wgrad) return OCL_OK;
        WgradPlan wp = ps->wgrad[conv_i];
        wp.a.x = xin;
        wp.a.dy = dy;
        if (xf_conv >= 0) {
            const BnView v = view(xf_conv);
            wp.a.xf = 1;
            wp.a.xf_groups = G;
            wp.a.xf_group_size = Nc / G;
            wp.a.xf_mean = v.save_mean; wp.a.xf_invstd = v.save_invstd;
            wp.a.xf_gamma = v.gamma; wp.a.xf_beta = v.beta;
        }
        if (grouped) {   // slab regions of kGroupRegion bytes side by side, one reduction launch per group_k layers
            if ((int64_t)wp.partial_floats * 4 > kGroupRegion || rm.n >= group_k) {
                if ((rc = flush_reduce(sw))) return rc;
            }
            if ((int64_t)wp.partial_floats * 4 <= kGroupRegion) {
                const int64_t off = (int64_t)rm.n * (kGroupRegion / 4);
                wp.a.partial = partial + off;
                int r = launch_wgrad(wp, sw);
                if (r) return r;
                wgrad_reduce_layer(wp, off, n->tensors[n->convs[conv_i].w_t].off, &rm.L[rm.n++]);
                return OCL_OK;
            }
        }
        wp.a.partial = batched ? partial + ps->partial_off[conv_i] : partial;
        if (defer) {
            deferred.push_back(wp);
            wgrad_reduce_layer(wp, ps->partial_off[conv_i], n->tensors[n->convs[conv_i].w_t].off, &rm.L[rm.n++]);
            return OCL_OK;
        }
        int r = launch_wgrad(wp, sw);
        if (r) return r;
        if (batched) {
            wgrad_reduce_layer(wp, ps->partial_off[conv_i], n->tensors[n->convs[conv_i].w_t].off, &rm.L[rm.n++]);
            return OCL_OK;
        }
        return launch_wgrad_reduce(wp, GT(n->convs[conv_i].w_t), accumulate, sw);
    };
    auto flush_pending = [&]() -> int {
        if (pending.empty()) return OCL_OK;
        int r = side_wait(n, s);
        for (size_t i = 0; i < pending.size() && !r; ++i) r = wgrad_now(pending[i].conv_i, pending[i].xin, pending[i].dy, pending[i].xf_conv);
        pending.clear();
        return r;
    };
    auto wgrad = [&](int conv_i, const float* xin, const float* dy, int xf_conv = -1) -> int {
        if (!coarse) return wgrad_now(conv_i, xin, dy, xf_conv);
        pending.push_back({conv_i, xin, dy, xf_conv});
        return (n_handed++ >= tail_from || (int)pending.size() >= flush_every) ? flush_pending() : OCL_OK;
    };
    auto dgrad = [&](int conv_i, const float* dy, float* dx, const float* res, const float* resmask, int extra_flags,
                     const BnbEpi* be = nullptr) -> int {
        const ConvInfo& c = n->convs[conv_i];
        for (auto& p : ps->dgrad[conv_i]) {
            int fl = extra_flags | (res ? (resmask ? EPI_RESMASK : EPI_RES) : 0);
            int r = run_conv(n, p, dy, pack + c.td_off, dx, fl, nullptr, nullptr, nullptr, res, resmask, s, nullptr, be);
            if (r) return r;
        }
        return OCL_OK;
    };
    // BatchNorm `bn_conv`'s backward with the reduction half in the epilogue of the data gradient that produces d (EPI_BNB): the
    // descriptor for that launch, and the apply launch that follows it
    auto bnb_desc = [&](int bn_conv, const float* zmask) -> BnbEpi {
        const BnView v = view(bn_conv);
        BnbEpi e;
        e.y = S + n->convs[bn_conv].y_off;
        e.z = zmask;
        e.mean = v.save_mean; e.invstd = v.save_invstd;
        e.gamma = v.gamma; e.beta = v.beta;
        e.sums = v.fsums;
        e.rep_stride = (int64_t)G * 2 * v.C;
        return e;
    };
    auto bn_apply_e = [&](int bn_conv, const float* d, float* dy) -> int {
        const ConvInfo& c = n->convs[bn_conv];
        const BnView v = view(bn_conv);
        BnApplyEArgs a;
        memset(&a, 0, sizeof(a));
        a.d = d; a.y = S + c.y_off; a.dy = dy;
        a.mean = v.save_mean; a.invstd = v.save_invstd;
        a.gamma = v.gamma;
        a.dgamma = v.dgamma; a.dbeta = v.dbeta;
        a.esums = v.fsums;
        a.esums_rep_stride = (int64_t)G * 2 * v.C;
        a.m_per_group = (int64_t)(Nc / G) * c.Ho * c.Wo;
        a.G = G; a.C = v.C; a.accumulate = accumulate;
        return launch_bn_apply_e(a, s);
    };

    auto stop_here = [&](int bi, int step) -> bool {
        if (n->dbg_stop != bi * 10 + step) return false;
        n->dbg_role[0] = gA; n->dbg_role[1] = gB; n->dbg_role[2] = gC; n->dbg_role[3] = gD; n->dbg_role[4] = gE;
        return true;
    };
    if (stop_here(99, 0)) return OCL_OK;   // right after the head: gA = dL/dz of the last block
    bool prev_epi = false;   // gA is already ReLU-masked and the batch sums of the BatchNorm it enters are in that BatchNorm's arena
    for (int bi = (int)n->blocks.size() - 1; bi >= 0; --bi) {
        const BlockInfo& b = n->blocks[bi];
        const ConvInfo& c1 = n->convs[b.conv1];
        const float* xin = S + (bi == 0 ? n->zstem_off : n->blocks[bi - 1].z_off);
        const float* a1 = S + b.a1_off;
        const float* z = S + b.z_off;
        // gA = dL/dz.  bn2 (and the projection BN) share the ReLU-masked gradient.
        int rB = -1, rC = -1;
        gB = take_dy(&rB);
        if (b.convs >= 0) gC = take_dy(&rC);
        if (prev_epi) {   // gA arrived masked, bn2's batch sums with it (epilogue of the block behind): the streaming apply kernel
            if ((rc = bn_apply_e(b.conv2, gA, gB))) return rc;
        } else if ((rc = bn_bwd(gA, z, b.conv2, gB, b.convs, gC))) return rc;
        prev_epi = false;
        if (stop_here(bi, 1)) return OCL_OK;                                 // gB = dL/dy2, gC = dL/dys
        if ((rc = publish())) return rc;
        if (b.convs >= 0) {
            if (!dbg_skip_shortcut() && (rc = wgrad(b.convs, xin, gC))) return rc;
            if ((rc = release(rC))) return rc;                               // (the shortcut's dgrad below reads gC on `s`)
        }
        if ((rc = fused ? wgrad(b.conv2, S + c1.y_off, gB, b.conv1) : wgrad(b.conv2, a1, gB))) return rc;
        if ((rc = release(rB))) return rc;
        // bn1's backward: its batch sums come out of conv2's data gradient (gD = the MASKED dL/da1), a streaming kernel applies them;
        // otherwise (plan without the epilogue table, eval-mode tape, > 2 groups) the one-pass kernel on the unmasked gD
        const bool epi1 = ps->dgrad_bnb[b.conv2] && !frozen && G <= 2 && n->dbg_stop < 0;
        BnbEpi be1;
        if (epi1) be1 = bnb_desc(b.conv1, fused ? nullptr : a1);
        if ((rc = dgrad(b.conv2, gB, gD, nullptr, nullptr, 0, epi1 ? &be1 : nullptr))) return rc;   // gD = dL/da1 (pre-mask; masked with EPI_BNB)
        if (stop_here(bi, 2)) return OCL_OK;
        int rB1 = -1;
        float* gB1 = take_dy(&rB1);
        if (epi1) {
            if ((rc = bn_apply_e(b.conv1, gD, gB1))) return rc;                                       // gB1 = dL/dy1
        } else if ((rc = bn_bwd(gD, fused ? nullptr : a1, b.conv1, gB1, -1, nullptr, fused))) return rc;
        gB = gB1;
        if (stop_here(bi, 3)) return OCL_OK;
        if ((rc = publish())) return rc;
        if ((rc = wgrad(b.conv1, xin, gB1))) return rc;
        if ((rc = release(rB1))) return rc;
        if (b.convs >= 0) {
            if ((rc = dgrad(b.conv1, gB1, gE, nullptr, nullptr, 0))) return rc;
            if (stop_here(bi, 4)) return OCL_OK;
            if (!dbg_skip_shortcut() && (rc = dgrad(b.convs, gC, gE, nullptr, nullptr, EPI_ACCUM))) return rc;
        } else {
            // + identity shortcut: dz * (z>0).  Stage 2 (small passes, get_plans): this launch completes dL/dz of the block in front (of the stem for
            // block 0), so its epilogue also masks that gradient with (xin > 0) and sums it for the BatchNorm behind xin
            const bool single_target = bi == 0 || n->blocks[bi - 1].convs < 0;
            const bool epi2 = ps->dgrad_bnb[b.conv1] && single_target && !frozen && G <= 2 && n->dbg_stop < 0;
            BnbEpi be2;
            if (epi2) be2 = bnb_desc(bi == 0 ? 0 : n->blocks[bi - 1].conv2, xin);
            if ((rc = dgrad(b.conv1, gB1, gE, gA, z, 0, epi2 ? &be2 : nullptr))) return rc;
            prev_epi = epi2;
        }
        if (stop_here(bi, 5)) return OCL_OK;                                 // gE = dL/dx of the block
        std::swap(gA, gE);
    }
    // stem
    if (env_tail > 0 && (rc = flush_pending())) return rc;   // (layer1.0.conv1's dL/dy exists: the stem's BatchNorm backward is not waited for)
    float* gS = take_dy();
    if (prev_epi) {
        if ((rc = bn_apply_e(0, gA, gS))) return rc;
    } else if ((rc = bn_bwd(gA, S + n->zstem_off, 0, gS, -1, nullptr))) return rc;
    if ((rc = flush_pending())) return rc;
    bool joined = !two_streams;   // nothing is left on the side stream
    auto join_side = [&]() -> int {   // the caller's stream waits for all of the side stream, and has whatever weight gradient still follows
        OCL_HIP(hipEventRecord(n->ev_join, sw));
        OCL_HIP(hipStreamWaitEvent(s, n->ev_join, 0));
        for (int i = 0; i < ocl_net::kDyRing; ++i) n->ev_done_pending[i] = false;   // covered by the join
        sw = s;
        joined = true;
        return OCL_OK;
    };
    // The stem's weight gradient is the tail of the backward: it runs on the caller's stream (no two more cross-stream hand-offs, ~30 us
    // of event latency in the trace) BESIDE the side stream's last kernels -- layer 1's weight gradients, the largest of the step, are
    // still running there when the chain ends -- with its own slab region (the slabs of one layer stay under 12 MB; the stem's start
    // 16 MB into the buffer), and the join follows it.
    if (two_streams && !batched) {
        if ((rc = flush_reduce(sw))) return rc;   // the layers still waiting for their reduction
        WgradPlan wp = ps->wgrad[0];
        wp.a.x = x4;
        wp.a.dy = gS;
        wp.a.partial = partial + stem_region / 4;
        if (stem_region / 4 + (int64_t)wp.partial_floats > n->partial_floats) wp.a.partial = nullptr;   // (workspace too small: after the join)
        // the side stream's slabs start at `partial`: the stem's region is only free beside them while every other layer's slabs end
        // below it (plan_wgrad caps a split at 12 MB, but a single slab of a wider net may exceed that)
        for (size_t i = 1; i < ps->wgrad.size(); ++i)
            if ((int64_t)ps->wgrad[i].partial_floats * 4 > (grouped ? kGroupRegion : (16ll << 20))) wp.a.partial = nullptr;
        if (wp.a.partial && !env_skip_wgrad) {
            if ((rc = launch_wgrad(wp, s))) return rc;
            if ((rc = launch_wgrad_reduce(wp, GT(n->convs[0].w_t), accumulate, s))) return rc;
        }
        if ((rc = join_side())) return rc;
        if (wp.a.partial) return OCL_OK;
    }
    // Every other pass: the stem's weight gradient goes where the other layers' went -- the caller's stream, or the side stream of a replay-sized
    // pass (the one reduction of all layers there too, then the join) -- followed by what waited for the end of the backward
    if (!joined && (rc = publish())) return rc;
    if ((rc = wgrad(0, x4, gS))) return rc;
    if (!joined && (rc = flush_pending())) return rc;
    if (defer) {   // every layer's weight gradient: one launch per form set, the layers without a form in the merged kernel on their own
        auto& tabs = n->wgrad_tables[std::make_tuple(Nc, G, (const float*)S)];
        for (int set = 0; set < 2; ++set) {
            std::vector<WgradPlan> grp;
            for (auto& wp : deferred)
                if (wgrad_multi_variant(wp) >= 0 && wgrad_multi_variant(wp) / 4 == set) grp.push_back(wp);
            if (grp.size() == 1) rc = launch_wgrad(grp[0], s);
            else if (!grp.empty()) rc = launch_wgrad_multi(grp.data(), (int)grp.size(), &tabs[set], s);
            if (rc) return rc;
        }
        for (auto& wp : deferred)
            if (wgrad_multi_variant(wp) < 0 && (rc = launch_wgrad(wp, s))) return rc;
    }
    if ((rc = flush_reduce(sw))) return rc;
    return joined ? OCL_OK : join_side();
}

extern "C" {

int ocl_net_backward(ocl_net* n, int slot, const float* dout, int accumulate, void* stream) {
    OCL_REQUIRE(n && n->bound, "net_backward: net not bound");
    if (int arc = check_async_error("net_backward")) return arc;
    OCL_REQUIRE(slot >= 0 && slot < n->d.n_slots && n->slot_valid[slot],
                "net_backward: slot %d holds no train-mode forward tape (forward with OCL_FWD_TRAIN|OCL_FWD_SAVE_TAPE first)", slot);
    OCL_REQUIRE(dout, "net_backward: null dout");
    hipStream_t s = (hipStream_t)stream;
    const int N = n->slot_n[slot], G = n->slot_groups[slot];
    const bool frozen = n->slot_frozen[slot];
    PlanSet* ps = nullptr;
    int rc = get_plans(n, N, G, &ps);
    if (rc != OCL_OK) return rc;
    n->slot_valid[slot] = false;  // a tape is consumed once (activation buffers are not preserved past this point)
    float* S = n->slotf(slot);
    const float* P = n->params;
    float* Gr = n->grads;
    float* pack = (float*)(n->ws + n->off_pack);
    // the arena was rewritten by a forward of MIR's virtual model since the taped forward (or plans made since need another layout)
    const bool repack = n->pack_src != P || (n->pack_have & n->pack_need_bwd) != n->pack_need_bwd;
    const int repack_mask = n->pack_need_fwd | n->pack_need_bwd;
    const bool bsums_dirty = !n->bsums_clean;   // a second backward since the last forward: trunk_backward clears the arena itself
    const bool replay = graph_enabled(n);
    const int FD = n->feat_dim, OD = n->out_dim;
    float* hb = (float*)(n->ws + n->off_head);
    float* dfeat = hb;
    float* dh1 = hb + (int64_t)N * FD;
    float* dh2 = dh1 + (int64_t)N * FD;
    if (replay) {   // the only read of caller memory: dout is staged inside the workspace, in front of the replayable sequence
        float* stage = hb + (int64_t)N * (3 * FD + 2 * OD);
        OCL_HIP(hipMemcpyAsync(stage, dout, (size_t)N * OD * 4, hipMemcpyDeviceToDevice, s));
        dout = stage;
    }
    float* feat = S + n->feat_off;
    float* h1 = S + n->h1_off;
    float* o = S + n->out_off;
    float* norms = S + n->norms_off;

    // ---- head -------------------------------------------------------------------------------------
    // Single chain, two HIP streams for the large batches: the caller's stream carries the dependent chain (head dx -> BatchNorm
    // backward -> data gradient -> ...); the weight gradients (head dW / db, conv_wgrad_kernel + reduce: a third of the step's MFMA
    // work, needed by nobody until the optimiser step) run on a second stream as soon as their dL/dy exists.  dL/dy buffers of the
    // trunk come from a ring, a slot is rewritten only after the event behind its last weight-gradient reader.  Replay batches of
    // 10-20 images are latency-bound: the event traffic costs more than the overlap returns there.  Debug stops and measurement
    // runs (ocl_prof_enable, OCL_SINGLE_STREAM=1: per-kernel durations of the kernel alone) stay on one stream as well.
    const bool two_streams = two_streams_at(in_pixels(n, N), n->dbg_stop);
    if (two_streams && (rc = ensure_side_stream(n))) return rc;
    HeadBwd hd;
    hd.feat = feat; hd.h1 = h1; hd.out = o; hd.norms = norms; hd.dout = dout;
    hd.dfeat = dfeat; hd.dh1 = dh1; hd.dh2 = dh2;
    const bool fused_tape = n->slot_fused[slot];
    auto body = [&]() -> int {
        int rc = OCL_OK;
        if (repack) {
            if ((rc = launch_pack_weights(P, pack, pack_descs(n), (int)n->convs.size(), pack_max_elems(n), s, repack_mask))) return rc;
        }
        if ((rc = head_backward(n, P, Gr, hd, N, accumulate, s, two_streams))) return rc;
        // ---- trunk ------------------------------------------------------------------------------------
        n->bsums_clean = !bsums_dirty;   // (trunk_backward reads the flag: the same decision whenever the sequence is issued)
        return trunk_backward(n, ps, P, Gr, S, N, G, accumulate, dfeat, s, two_streams ? n->s2 : nullptr, frozen, fused_tape);
    };
    ocl_net::GraphKey key;
    memset(&key, 0, sizeof(key));
    key.kind = 1; key.N = N; key.G = G; key.slot = slot;
    key.a = (accumulate ? 1 : 0) | (frozen ? 2 : 0) | (fused_tape ? 4 : 0) | (two_streams ? 8 : 0);
    key.b = (repack ? 1 : 0) | (bsums_dirty ? 2 : 0);
    key.c = repack_mask;
    key.p = (uint64_t)(uintptr_t)P;
    rc = two_streams ? body() : run_replayed(n, key, s, body);   // (single-stream sequences only: see ocl_net_forward_segments)
    if (repack) note_packed(n, P, repack_mask, s);
    n->bsums_clean = false;
    return rc;
}

int ocl_test_net_forms(int hw, int nf, int N, int groups, int train, ocl_test_net_form* out, int cap) {
    OCL_REQUIRE(N > 0 && groups > 0 && N % groups == 0 && (train || groups == 1), "test_net_forms: N=%d groups=%d train=%d", N, groups, train);
    ocl_net* n = nullptr;
    int rc = make_test_net(hw, nf, 10, 0, 0, N, &n);
    if (rc != OCL_OK) return rc;
    PlanSet ps;
    rc = make_plan_set(n, N, groups, &ps);
    int cnt = 0;
    auto put = [&](int layer, int dir) -> ocl_test_net_form* {
        ocl_test_net_form* e = cnt < cap && out ? &out[cnt] : nullptr;
        ++cnt;
        if (e) {
            memset(e, 0, sizeof(*e));
            e->layer = layer; e->dir = dir;
        }
        return e;
    };
    for (size_t i = 0; rc == OCL_OK && i < n->convs.size(); ++i) {
        const ConvInfo& c = n->convs[i];
        ocl_test_conv_desc cd;
        memset(&cd, 0, sizeof(cd));
        cd.cin = c.Cin; cd.cout = c.Cout; cd.k = c.k; cd.stride = c.stride; cd.hin = c.Hin; cd.win = c.Win; cd.n = N; cd.groups = groups;
        cd.xf = c.xf_src >= 0 ? 1 : 0;
        if (ocl_test_net_form* e = put((int)i, 0)) {
            e->desc = cd;
            test_conv_form(ps.fwd[i], &e->form);
        }
        if (!train) continue;
        cd.xf = 0;
        cd.dir = 1;
        cd.merge = 1;
        cd.bnb = ps.dgrad_bnb[i];
        for (auto& p : ps.dgrad[i])
            if (ocl_test_net_form* e = put((int)i, 1)) {
                e->desc = cd;
                test_conv_form(p, &e->form);
            }
        if (ocl_test_net_form* e = put((int)i, 2)) {
            e->wg_merged = ps.wgrad_target[i] > 0;
            e->wdesc.cin = c.Cin; e->wdesc.cout = c.Cout; e->wdesc.k = c.k; e->wdesc.stride = c.stride; e->wdesc.hin = c.Hin; e->wdesc.win = c.Win;
            e->wdesc.n = N; e->wdesc.xf_groups = c.xf_src >= 0 ? groups : 0; e->wdesc.wg_target = ps.wgrad_target[i];
            test_wgrad_form(ps.wgrad[i], &e->wform);
        }
    }
    ocl_net_destroy(n);
    return rc == OCL_OK ? cnt : rc;
}

int ocl_test_head_side_min_batch(int hw) {
    OCL_REQUIRE(hw >= 32, "test_head_side_min_batch: hw=%d", hw);
    const int64_t px = (int64_t)hw * hw;
    const int64_t need = (int64_t)std::max(kTwoStreamMinBatch, kSideExtraMinBatch) * 1024;
    const int N = (int)std::max<int64_t>(1, (need + px - 1) / px);
    return head_side_at(N * px, two_streams_at(N * px, -1)) ? N : 0;   // (0: measurement modes keep every pass on one stream)
}

int ocl_test_head(ocl_test_head_args* a, void* stream) {
    OCL_REQUIRE(a && a->params && a->grads && a->feat && a->dout && a->out && a->dfeat, "test_head: null pointer");
    OCL_REQUIRE(a->head >= 0 && a->head <= 3 && a->n > 0 && a->hw >= 32 && a->nf > 0, "test_head: head=%d n=%d hw=%d nf=%d", a->head, a->n, a->hw, a->nf);
    OCL_REQUIRE(a->head == 0 || a->norms, "test_head: norms");
    OCL_REQUIRE((a->head != 1 && a->head != 2) || (a->h2 && a->dh2), "test_head: h2 / dh2");
    OCL_REQUIRE(a->head != 1 || (a->h1 && a->dh1), "test_head: h1 / dh1");
    ocl_net* n = nullptr;
    int rc = make_test_net(a->hw, a->nf, a->n_classes, a->head, a->feat_dim, a->n, &n);
    if (rc != OCL_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int N = a->n;
    if (a->n_params != n->n_params) {
        set_error("test_head: the flat arrays hold %lld floats, the net's %lld", (long long)a->n_params, (long long)n->n_params);
        rc = OCL_ERR_ARG;
    }
    bool wrote = false;
    if (rc == OCL_OK)
        rc = head_forward(n, a->params, (float*)a->feat, a->h1, a->h2, a->norms, a->out, N, s, nullptr, &wrote);
    const bool two_streams = two_streams_at(in_pixels(n, N), n->dbg_stop);
    if (rc == OCL_OK && two_streams) rc = ensure_side_stream(n);
    if (rc == OCL_OK) {
        HeadBwd hd;
        hd.feat = a->feat; hd.h1 = a->h1; hd.out = a->out; hd.norms = a->norms; hd.dout = a->dout;
        hd.dfeat = a->dfeat; hd.dh1 = a->dh1; hd.dh2 = a->dh2;
        rc = head_backward(n, a->params, a->grads, hd, N, a->accumulate, s, two_streams);
        a->side_stream = head_side_at(in_pixels(n, N), two_streams) ? 1 : 0;
    }
    if (n->s2) (void)hipStreamSynchronize(n->s2);
    if (hipStreamSynchronize(s) != hipSuccess && rc == OCL_OK) {
        set_error("test_head: %s", hipGetErrorString(hipGetLastError()));
        rc = OCL_ERR_HIP;
    }
    ocl_net_destroy(n);
    return rc;
}

int ocl_net_debug_stop(ocl_net* n, int stage) {
    OCL_REQUIRE(n, "debug_stop: null net");
    n->dbg_stop = stage;
    return OCL_OK;
}

int ocl_net_debug_copy(ocl_net* n, int slot, int what, int index, float* dst, int64_t max_floats, int64_t* n_written, void* stream) {
    OCL_REQUIRE(n && n->bound && slot >= 0 && slot < n->d.n_slots && dst, "debug_copy: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int N = n->slot_n[slot] > 0 ? n->slot_n[slot] : n->d.max_batch;
    const float* src = nullptr;
    int64_t cnt = 0;
    float* S = n->slotf(slot);
    if (what == 0) {  // raw conv output
        OCL_REQUIRE(index >= 0 && index < (int)n->convs.size(), "debug_copy: conv index");
        const ConvInfo& c = n->convs[index];
        src = S + c.y_off;
        cnt = (int64_t)N * c.Ho * c.Wo * c.Cout;
    } else if (what == 1) {  // block output
        OCL_REQUIRE(index >= 0 && index < (int)n->blocks.size(), "debug_copy: block index");
        const ConvInfo& c = n->convs[n->blocks[index].conv1];
        src = S + n->blocks[index].z_off;
        cnt = (int64_t)N * c.Ho * c.Wo * c.Cout;
    } else if (what == 2) {  // gradient scratch buffer
        OCL_REQUIRE(index >= 0 && index < 5, "debug_copy: gbuf index");
        src = n->gbuf(index);
        cnt = n->gbuf_floats;
    } else if (what == 3) {  // gradient buffer by role (gA..gE) at the last debug stop
        OCL_REQUIRE(index >= 0 && index < 5 && n->dbg_role[index], "debug_copy: no debug stop recorded");
        src = n->dbg_role[index];
        cnt = n->gbuf_floats;
    } else if (what == 5) {  // stem output
        const ConvInfo& c = n->convs[0];
        src = S + n->zstem_off;
        cnt = (int64_t)N * c.Ho * c.Wo * c.Cout;
    } else if (what == 4) {  // post-ReLU activation a1 of block `index`
        OCL_REQUIRE(index >= 0 && index < (int)n->blocks.size(), "debug_copy: block index");
        const ConvInfo& c = n->convs[n->blocks[index].conv1];
        src = S + n->blocks[index].a1_off;
        cnt = (int64_t)N * c.Ho * c.Wo * c.Cout;
        if (n->slot_fused[slot]) {   // the pass never wrote a1: materialise it from the raw output and the saved statistics
            const BnView v = bn_view(n, n->params, nullptr, S, c.bn);
            const int G = std::max(1, n->slot_groups[slot]);
            int rc = launch_bn_apply_saved(S + c.y_off, v.save_mean, v.save_invstd, v.gamma, v.beta, S + n->blocks[index].a1_off, (int64_t)(N / G) * c.Ho * c.Wo, G, v.C, s);
            if (rc != OCL_OK) return rc;
        }
    } else {
        set_error("debug_copy: what=%d", what);
        return OCL_ERR_ARG;
    }
    cnt = std::min(cnt, max_floats);
    OCL_HIP(hipMemcpyAsync(dst, src, (size_t)cnt * 4, hipMemcpyDeviceToDevice, s));
    if (n_written) *n_written = cnt;
    return OCL_OK;
}

}  // extern "C"

namespace ocl {

int net_test_tables(int hw, int nf, NetTestTables* out) {
    ocl_net* n = nullptr;
    int rc = make_test_net(hw, nf, 10, 0, 0, 1, &n);
    if (rc != OCL_OK) return rc;
    make_descs(n, &out->pack, &out->fold);
    out->n_params = n->n_params;
    out->n_stats = n->n_stats;
    out->pack_floats = n->pack_floats;
    out->max_elems = pack_max_elems(n);
    ocl_net_destroy(n);
    return OCL_OK;
}

}  // namespace ocl
