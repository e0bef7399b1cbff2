// Host side of the Reduced-ResNet18 convolution engine for gfx950: the planners and plan tables of the three kernel families, the launch,
// the batch-sum mode switch and the per-device set-up.  No kernel lives here:
//
//  conv_t_kernel.h    conv_t_kernel, implicit-GEMM 3x3 / 1x1 convolution on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32); instantiated by
//                     conv_t.hip (plain forms) and conv_t_bnb.hip (EPI_BNB forms)
//  conv_q.hip         conv_q_kernel, <= 20 output channels on v_mfma_f32_4x4x1_16b_f32
//  conv_s.hip         conv_s_kernel, few output pixels behind a deep K
//  convw.hip          conv_w_kernel, wave-autonomous tiles (with its own planner)
//  wgrad.hip          conv_wgrad_kernel, the weight gradient (with its own planner)
//  bn.hip             train-mode BatchNorm forward and backward
//  conv_aux.hip       weight packing, input layout conversion, pooling, L2 norm and the other small kernels
//
// Replaces the ATen sequences behind models/resnet.py:10-12,32-37,90-99 and their autograd.
#include "conv_dev.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <cmath>

namespace ocl {

// The host's copy of g_det_sums, PER DEVICE (conv_s_kernel's instantiation is chosen by it; the __constant__ lives per device, so a
// process-wide host flag could disagree with it as soon as a second device is touched: cells written as fixed point and read as doubles)
static const int kMaxDevices = 64;
static int g_det_dev[kMaxDevices] = {0};
static int det_host() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    return g_det_dev[dev];
}
std::vector<det_flag_setter_t>& det_flag_setters() {
    static std::vector<det_flag_setter_t> v;   // function-local: complete before the first unit's registration, whatever the load order
    return v;
}
int set_deterministic_sums(int on) {
    const int v = on ? 1 : 0;
    int dev = 0;
    OCL_HIP(hipGetDevice(&dev));
    OCL_REQUIRE(dev >= 0 && dev < kMaxDevices, "set_deterministic: device %d", dev);
    OCL_HIP(hipDeviceSynchronize());   // (no launch may straddle the switch: the cells are interpreted by the flag)
    for (det_flag_setter_t set : det_flag_setters()) OCL_HIP(set(v));   // every translation unit's copy of the flag (conv_stats_dev.h)
    g_det_dev[dev] = v;                // the current device only: the mode is a per-device state, like the symbol
    return OCL_OK;
}

static conv_fn_t convt_fn(int MT, int NT, int PF, int res, int cls = 0, int pipe = 0, int bnb = 0) {
    return bnb ? convt_bnb_fn(MT, NT, PF, res, cls, pipe) : convt_plain_fn(MT, NT, PF, res, cls, pipe);
}
static int convt_pf_for(int units) { return units <= 1024 ? 4 : 8; }
// the prefetch depth of the conv_t_kernel instantiation launch_conv picks for a plan (also what the test hooks report)
int convt_plan_pf(const ConvPlan& p) { return convt_pf_for(p.a.imgs * p.a.PR * p.a.PC * (p.a.KC / 4)); }

// ---- conv_t_kernel layout: fills the tile-dependent fields for (MT channel tiles, NT pixel tiles); returns LDS bytes (0: no fit)
static size_t convt_layout(const ConvGeomDesc& g, ConvArgs& a, int MT, int NT, bool pipe = false) {
    const int nt16 = cdiv(g.Cout, 16);
    const int splits = cdiv(nt16, MT);
    const int COPW = 16 * MT;
    a.n_splits = splits;
    a.CoutP = splits * COPW;
    a.group_size = g.N / g.groups;
    const int LP = g.LH * g.LW;
    const int BM = 64 * NT;
    if (LP >= BM) {
        a.imgs = 1; a.ppi = BM; a.tiles_per_img = cdiv(LP, BM);
    } else {
        a.imgs = std::min(BM / LP, a.group_size); a.ppi = LP; a.tiles_per_img = 1;
    }
    a.PC = (g.LW - 1) * g.is + (a.max_dx - a.min_dx) + 1;
    const int rows_l = (a.imgs == 1 && LP >= BM) ? std::min(g.LH, (BM + g.LW - 2) / g.LW + 1) : g.LH;
    a.PR = (rows_l - 1) * g.is + (a.max_dy - a.min_dy) + 1;
    a.C4tot = g.Cin / 4;
    size_t bytes = 0;
    for (;;) {
        for (int KC = g.Cin; KC >= 4; KC -= 4) {
            if (g.Cin % KC) continue;
            a.KC = KC;
            a.CP = ((KC / 4) & 1) ? KC : KC + 4;     // 16-byte pixel slots, an odd number of them per pixel: b128 reads of 16 pixels spread over all banks
            a.Qc = g.ntaps * (KC / 4);
            a.Qpad = 0;   // every class's groups are padded to whole rounds of 4
            for (int c = 0; c < std::max(1, g.ncls); ++c) a.Qpad += (int)round_up((g.ncls > 1 ? g.cls_ntaps[c] : g.ntaps) * (KC / 4), 4);
            const size_t w_all = (size_t)a.Qpad * COPW * 16;
            a.wres = (KC == g.Cin && w_all <= kResidentBytes) ? 1 : 0;
            a.pipe = (pipe && !a.wres && NT == 1) ? 1 : 0;   // ring of three stage buffers of pipe_qs(MT) groups (conv_t_kernel<..., PIPE>)
            a.QS = a.wres ? a.Qpad : a.pipe ? pipe_qs(MT) : std::min(a.Qpad, ((256 * kWPF) / COPW) & ~3);
            a.nstage = cdiv(a.Qpad, a.QS);
            const size_t patch_b = (size_t)round_up(std::max((size_t)a.imgs * a.PR * a.PC * a.CP * 4, (size_t)8 * COPW * 8), 16);
            a.patch_floats = (int)(patch_b / 4);
            const size_t xf_b = g.xf ? (size_t)g.groups * g.Cin * 8 : 0;   // input transform: scale / shift per (group, channel)
            const size_t bnb_b = g.bnb ? (size_t)g.groups * g.Cout * 12 : 0;   // EPI_BNB: scale / shift / mean per (group, output channel)
            a.bnb_lds = g.bnb ? (int)(xf_b / 4) : -1;
            bytes = (size_t)kMaxWgTiles * 32 + 64 + (size_t)2 * a.Qpad * 4 + (a.wres ? w_all : (size_t)(a.pipe ? 3 : 2) * a.QS * COPW * 16) + patch_b + xf_b + bnb_b;
            const bool units_ok = a.imgs * a.PR * a.PC * (KC / 4) <= 256 * kConvPatchPF;
            if (units_ok && bytes <= kLdsLimit - 2048 && (bytes <= 100 * 1024 || KC <= 20)) goto found;
        }
        if (a.imgs > 1) {   // shrink the tile (fewer images per workgroup) and retry
            a.imgs -= 1;
            continue;
        }
        return 0;
    }
found:
    if (a.imgs > 127 || a.PR >= 256 || a.PC >= 256 || a.KC / 4 >= 256) return 0;
    a.tiles_per_group = cdiv(a.group_size, a.imgs) * a.tiles_per_img;
    return bytes;
}

// ---- conv_q_kernel plan: 5 blocks of 4 channels, NTQ 64-pixel sets per wave (tile = 256 * NTQ pixels), weights resident, one chunk
static int plan_conv_q_ntq(const ConvGeomDesc& g, ConvPlan* p, const int NTQ, bool* too_wide = nullptr) {
    ConvArgs& a = p->a;
    constexpr int COPW = 4 * kQBlocks;
    if (g.Cout > COPW || g.Cout % 4 || g.ncls > 1) return OCL_ERR_ARG;
    a.n_splits = 1;
    a.CoutP = COPW;
    a.group_size = g.N / g.groups;
    const int LP = g.LH * g.LW, BM = 256 * NTQ;
    if (LP >= BM) {
        a.imgs = 1; a.ppi = BM; a.tiles_per_img = cdiv(LP, BM);
    } else {
        a.imgs = std::min(BM / LP, a.group_size); a.ppi = LP; a.tiles_per_img = 1;
    }
    a.PC = (g.LW - 1) * g.is + (a.max_dx - a.min_dx) + 1;
    // lattice rows a tile can touch: exactly BM / LW when tiles start at row boundaries, one more when they straddle
    const bool whole_rows = BM % g.LW == 0 && LP % BM == 0;
    const int rows_l = (a.imgs == 1 && LP >= BM) ? (whole_rows ? BM / g.LW : std::min(g.LH, (BM + g.LW - 2) / g.LW + 1)) : g.LH;
    a.PR = (rows_l - 1) * g.is + (a.max_dy - a.min_dy) + 1;
    a.C4tot = g.Cin / 4;
    a.KC = g.Cin;
    a.CP = ((a.KC / 4) & 1) ? a.KC : a.KC + 4;
    a.Qc = g.ntaps * (a.KC / 4);
    a.Qpad = (int)round_up(a.Qc, 4);
    a.wres = 1; a.pipe = 0; a.QS = a.Qpad; a.nstage = 1;
    const int units = a.imgs * a.PR * a.PC * (a.KC / 4);
    if (too_wide) *too_wide = units > 256 * 12;
    if (units > 256 * 12 || a.imgs > 127 || a.PR >= 256 || a.PC >= 256 || a.KC / 4 >= 64) return OCL_ERR_ARG;
    const int PF = (units <= 1024 && NTQ == 2) ? 4 : 12;
    const size_t patch_b = (size_t)round_up(std::max((size_t)a.imgs * a.PR * a.PC * a.CP * 4, (size_t)8 * COPW * 8), 16);
    a.patch_floats = (int)(patch_b / 4);
    size_t lds = (size_t)kMaxWgTiles * 32 + 64 + (size_t)2 * a.Qpad * 4 + (size_t)a.Qpad * COPW * 16 + patch_b + (g.xf ? (size_t)g.groups * g.Cin * 8 : 0) +
                 (g.bnb ? (size_t)g.groups * g.Cout * 12 : 0);
    a.bnb_lds = g.bnb ? (g.xf ? g.groups * g.Cin * 2 : 0) : -1;
    a.qstat_off = (int)round_up(lds, 16);
    lds = (size_t)a.qstat_off + (size_t)(4 * 4 + 4) * 2 * COPW * 4;   // statistics scratch: row sums + per-wave accumulators
    if (lds > kLdsLimit - 2048) return OCL_ERR_ARG;
    a.tiles_per_group = cdiv(a.group_size, a.imgs) * a.tiles_per_img;
    const int ntiles = g.groups * a.tiles_per_group;
    // the form wants the machine full of whole tiles: below ~half a tile per CU the 64-pixel tiles of conv_t_kernel spread better
    if (ntiles < 128 && g.force_q4 <= 0) return OCL_ERR_ARG;
    a.cls_pack = 1 | (g.ntaps << 4);
    a.cls_oyx = 0;
    p->q4 = NTQ; p->MT = kQBlocks; p->NT = NTQ;
    p->lds_bytes = lds;
    a.WPT = g.WPT > 0 ? g.WPT : (int)round_up(g.Cout, 16);
    for (int t = 0; t < 9; ++t) a.tpo[t] = t < a.ntaps ? ((a.tdy[t] - a.min_dy) * a.PC + (a.tdx[t] - a.min_dx)) * a.CP : 0;
    {
        const int kc4 = a.KC / 4;
        a.d_c4 = 256 % kc4;
        const int d_pix = 256 / kc4;
        a.d_pc = d_pix % a.PC;
        a.d_row = d_pix / a.PC;
    }
    a.groups = g.groups;
    a.aligned = a.imgs > 1 ? 1 : ((BM % g.LW == 0 && LP % BM == 0) ? 1 : 0);
    {
        auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); };
        a.m_tpg = magic(a.tiles_per_group); a.m_tpi = magic(a.tiles_per_img); a.m_lw = magic(a.LW); a.m_ppi = magic(a.ppi);
        a.m_kc4 = magic(a.KC / 4); a.m_pc = magic(a.PC); a.m_pr = magic(a.PR);
        const int64_t xmax = std::max<int64_t>(std::max<int64_t>(ntiles, (int64_t)LP + BM), 4096);
        const int64_t dmax = std::max(std::max(a.tiles_per_group, a.tiles_per_img), std::max(std::max(a.LW, a.ppi), std::max(a.PC, a.PR)));
        if (xmax * dmax >= (1ll << 32)) return OCL_ERR_ARG;
    }
    {   // two workgroups per CU where the LDS allows it: the second wave per SIMD covers the other's operand reads
        int bpc = (int)std::min<size_t>(2, kLdsLimit / (lds + 512));
        if (g.force_bpc) bpc = g.force_bpc;
        p->grid_x = std::max(1, std::min(ntiles, 256 * std::max(1, bpc)));
    }
    p->grid_x = std::max(p->grid_x, cdiv(ntiles, kMaxWgTiles));
    p->grid_y = 1;
    a.off_tdesc = (int)round_up(16 + 2 * a.Qpad, 4);
    a.off_pu = a.off_tdesc + ntiles * 8;
    a.off_loc = a.off_pu + 3 * PF * 256;
    a.blob_ints = a.off_loc + 3 * NTQ * 256;
    a.blob = nullptr;
    return OCL_OK;
}

static int plan_conv_q(const ConvGeomDesc& g, ConvPlan* p) {
    // 512-pixel tiles; 256-pixel tiles where the patch of 512 pixels has more units than a workgroup stages (84-pixel-wide rows)
    ConvPlan q = *p;
    bool too_wide = false;
    int r = plan_conv_q_ntq(g, &q, 2, &too_wide);
    if (r != OCL_OK && too_wide) {   // (not where 512-pixel tiles are merely too few: there conv_t_kernel's 64-pixel tiles spread better)
        q = *p;
        r = plan_conv_q_ntq(g, &q, 1);
    }
    if (r == OCL_OK) *p = q;
    return r;
}

// ---- conv_s_kernel plan: (16 NT)-pixel x 16-channel workgroups, input channels split over the four waves --------------------------
static int plan_conv_s_nt(const ConvGeomDesc& g, ConvPlan* p, int NT) {
    ConvArgs& a = p->a;
    if (g.ncls > 1 || g.Cin % 16 || g.Cout % 4) return OCL_ERR_ARG;
    const int LP = g.LH * g.LW, TP = 16 * NT;
    // a tile = TP consecutive lattice pixels of one image (whole rows where the lattice allows: the lane -> pixel map is then the same
    // for every tile and comes from the plan's table), or whole images
    a.n_splits = cdiv(g.Cout, 16);
    a.CoutP = a.n_splits * 16;
    a.group_size = g.N / g.groups;
    if (LP >= TP) {
        a.imgs = 1; a.ppi = TP; a.tiles_per_img = cdiv(LP, TP);
    } else {
        a.imgs = std::min(TP / LP, a.group_size); a.ppi = LP; a.tiles_per_img = 1;
    }
    a.PC = (g.LW - 1) * g.is + (a.max_dx - a.min_dx) + 1;
    const bool whole_rows = TP % g.LW == 0 && LP % TP == 0;
    const int rows_l = LP >= TP ? (whole_rows ? TP / g.LW : std::min(g.LH, (TP + g.LW - 2) / g.LW + 1)) : g.LH;
    a.PR = (rows_l - 1) * g.is + (a.max_dy - a.min_dy) + 1;
    a.C4tot = g.Cin / 4;
    a.KC = g.Cin / 4;                                   // one wave's channel slice
    a.CP = ((a.KC / 4) & 1) ? a.KC : a.KC + 4;
    a.Qc = g.ntaps * (a.KC / 4);
    a.Qpad = (int)round_up(a.Qc, 16);                   // whole loop bodies of four rounds (the padding groups carry zero weights)
    if (16 + 2 * a.Qpad > 512) return OCL_ERR_ARG;
    a.wres = 0; a.pipe = 0; a.QS = a.Qpad;
    const int units = a.imgs * a.PR * a.PC * (a.KC / 4);
    a.nstage = cdiv(units, 64 * kPFS);                  // staging passes of 64 kPFS units per wave
    if (a.nstage > 3 || a.imgs > 127 || a.PR >= 256 || a.PC >= 256 || a.KC / 4 >= 64) return OCL_ERR_ARG;
    a.patch_floats = std::max((int)round_up((int64_t)a.imgs * a.PR * a.PC * a.CP, 4), NT * 64 * 4);   // (>= the partial tiles it holds at the end)
    a.bnb_lds = g.bnb ? 0 : -1;   // (conv_s_kernel reads the BatchNorm's parameters straight from memory: no table)
    a.tiles_per_group = cdiv(a.group_size, a.imgs) * a.tiles_per_img;
    const int ntiles = g.groups * a.tiles_per_group;
    const size_t lds = 64 + (size_t)(2 * a.Qpad + 16) * 4 + (size_t)4 * a.patch_floats * 4 + (g.xf ? (size_t)g.groups * g.Cin * 8 : 0);
    if (lds > 64 * 1024) return OCL_ERR_ARG;
    // Worth it (profiles/r3_conv_s_ab.md) where conv_t_kernel's 64-pixel tiles leave most of the machine idle behind a long K chain:
    // lattices of <= 16 pixels per image (layer 4: a 64-pixel tile is four images, each with its own halo, and K = 720 - 1440 behind
    // every wave) at any batch size; larger lattices (layer 3) below 1000 units of conv_t_kernel work (< 200 images), where that
    // kernel's resident-weight plan takes over (26.9 vs 30.2 us at 220 images).
    const int64_t tiles64 = (int64_t)g.groups * (LP >= 64 ? (int64_t)a.group_size * cdiv(LP, 64) : cdiv(a.group_size, std::max(1, 64 / LP)));
    if (g.force_cs <= 0 && ((LP > 16 && tiles64 * cdiv(g.Cout, 16) >= 1000) || a.Qc <= 36)) return OCL_ERR_ARG;
    a.cls_pack = 1 | (g.ntaps << 4);
    a.cls_oyx = 0;
    p->cs = 1; p->q4 = 0; p->MT = 1; p->NT = NT;
    p->lds_bytes = lds;
    a.WPT = g.WPT > 0 ? g.WPT : a.CoutP;
    for (int t = 0; t < 9; ++t) a.tpo[t] = t < a.ntaps ? ((a.tdy[t] - a.min_dy) * a.PC + (a.tdx[t] - a.min_dx)) * a.CP : 0;
    {   // a wave's 64 lanes walk the patch units
        const int kc4 = a.KC / 4;
        a.d_c4 = 64 % kc4;
        const int d_pix = 64 / kc4;
        a.d_pc = d_pix % a.PC;
        a.d_row = d_pix / a.PC;
    }
    a.groups = g.groups;
    a.aligned = (LP < TP || whole_rows) ? 1 : 0;
    {
        auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); };
        a.m_tpg = a.m_tpi = a.m_kc4 = a.m_pc = a.m_pr = 0;
        a.m_lw = magic(a.LW); a.m_ppi = magic(a.ppi);
        if ((int64_t)(LP + TP) * std::max(a.LW, a.ppi) >= (1ll << 32)) return OCL_ERR_ARG;
    }
    p->grid_x = ntiles;
    p->grid_y = a.n_splits;
    a.off_tdesc = (int)round_up(16 + 2 * a.Qpad, 4);
    a.off_pu = a.off_tdesc + ntiles * 8;
    a.off_loc = a.off_pu + 3 * kPFS * a.nstage * 256;
    a.blob_ints = a.off_loc + 3 * NT * 256;
    a.blob = nullptr;
    return OCL_OK;
}

static int plan_conv_s(const ConvGeomDesc& g, ConvPlan* p) {
    // One pixel tile per workgroup; two (every weight quad feeds two MFMAs: half the weight and table bytes per MFMA, twice the patch per
    // wave) on the 8x8 lattices of layer 3 once the one-tile grid has >= 800 workgroups -- 100 images: 14.6 vs 17.4 us, 150: 21.8 vs
    // 24.1; on layer 4 (two whole images per workgroup) it only pays around 150 images (profiles/r3_conv_s_ab.md).
    static const int env_nt = env_int("OCL_CONV_S_NT", 0);   // measurement knob: 1 / 2 = always
    ConvPlan q1 = *p;
    const int r1 = plan_conv_s_nt(g, &q1, 1);
    const bool want2 = env_nt ? env_nt == 2 : (r1 == OCL_OK && g.LH * g.LW > 16 && (int64_t)q1.grid_x * q1.grid_y >= 800);
    if (want2) {
        ConvPlan q2 = *p;
        if (plan_conv_s_nt(g, &q2, 2) == OCL_OK) {
            *p = q2;
            return OCL_OK;
        }
    }
    if (r1 == OCL_OK) *p = q1;
    return r1;
}

static int plan_conv_t(const ConvGeomDesc& g, ConvPlan* p) {
    ConvArgs& a = p->a;
    p->cs = 0;
    p->cw = 0;
    {   // wave-autonomous tiles over resident weights (convw.hip): no workgroup barrier between the prologue and the statistics flush
        // OCL_CONV_W: 0 = never, 1 (default) = where its specialised form exists and measured faster (profiles/r6_convw_vs_planner.txt: the 3x3
        // stride-1 convolutions of 40 and 80 channels from ~100 images on), 2 = wherever it fits (A/B reference of tests/test_gpu_ring.py)
        static const int env_cw = env_int("OCL_CONV_W", 1);
        if (g.force_cw > 0 || (g.force_cw == 0 && env_cw > 0 && !g.force_MT && !g.force_NT && g.force_cs <= 0 && g.force_q4 <= 0)) {
            ConvPlan q = *p;
            if (plan_conv_w(g, &q) == OCL_OK) {
                const int64_t units = (int64_t)(g.N / q.a.imgs) * q.a.tiles_per_img * q.a.n_splits;   // (pixel tile, channel split) units of the launch
                // (not with the input transform: conv_wx_kernel's register pipeline for it is slower than conv_t_kernel's staging -- 33.7 vs 33.3 us
                // on layer 2, 196 us on layer 3: profiles/r6_convw_in_network.txt)
                const bool hot = q.cw == 2 && !g.xf && g.ntaps == 9 && g.is == 1 && (g.Cout == 40 || g.Cout == 80) && g.Cin == g.Cout && units >= 2048;
                if (g.force_cw > 0 || env_cw >= 2 || hot) {
                    *p = q;
                    return OCL_OK;
                }
            }
        }
    }
    {   // few output pixels behind a deep K (layers 3 - 4 of a replay-sized pass): K split over the waves
        static const bool env_cs = env_int("OCL_CONV_S", 1) != 0;
        if (g.force_cs > 0 || (g.force_cs == 0 && env_cs && !g.force_MT && !g.force_NT)) {
            ConvPlan q = *p;
            if (plan_conv_s(g, &q) == OCL_OK) {
                *p = q;
                return OCL_OK;
            }
        }
    }
    {   // <= 20 output channels: the 4x4x1 form (no channel / K padding) where it fits and the launch is large enough
        static const bool env_q4 = env_int("OCL_CONV_Q4", 1) != 0;
        if (g.force_q4 > 0 || (g.force_q4 == 0 && env_q4 && !g.force_MT && !g.force_NT)) {
            ConvPlan q = *p;
            if (plan_conv_q(g, &q) == OCL_OK) {
                *p = q;
                return OCL_OK;
            }
        }
    }
    p->q4 = 0;
    const int nt16 = cdiv(g.Cout, 16);
    const int LPx = g.LH * g.LW;
    const int64_t tiles64 = (int64_t)g.groups * (LPx >= 64 ? (int64_t)(g.N / g.groups) * cdiv(LPx, 64)
                                                            : cdiv(g.N / g.groups, std::max(1, 64 / LPx)));
    // channel tiles per workgroup: all of them up to 5 (a lane's A reads are reused NT times, its B reads MT times); fewer when
    // the layer has too few pixel tiles to give every CU a workgroup
    int MT = std::min(5, nt16);
    if (nt16 > 5) MT = cdiv(nt16, cdiv(nt16, 5));                    // balanced splits (10 tiles -> 2 x 5)
    while (MT > 1 && tiles64 * cdiv(nt16, MT) < 200) --MT;   // kbench sweep: 4x55 workgroups of 3 channel tiles beat 5x55 of 2 on layer 4
    if (nt16 > MT) MT = cdiv(nt16, cdiv(nt16, MT));
    // 160 output channels behind a deep K that conv_s_kernel does not take (layer 4 of a 50-image 84x84 pass: 100 pixel tiles): two
    // splits of five channel tiles are 200 workgroups with a 360-round chain each; five splits of two fill the machine twice
    // (kbench sweep, profiles/r3_kbench_sweep_84.txt: 37.7 vs 48.6 us; three or four tiles per workgroup pad 10 tiles to 12)
    if (nt16 == 10 && g.ntaps * g.Cin >= 1280 && tiles64 * 2 < 400) MT = 2;
    int NT = tiles64 * cdiv(nt16, MT) >= 2048 ? 2 : 1;
    if (g.ncls > 1) NT = 1;
    if (g.force_MT) MT = g.force_MT;
    if (g.force_NT) NT = g.force_NT;
    if (MT < 1 || MT > 5 || NT < 1 || NT > 2 || MT > nt16) return OCL_ERR_ARG;
    if (g.ncls > 1 && NT != 1) return OCL_ERR_ARG;   // (a forced NT = 2: conv_t_kernel has output classes with one pixel tile per wave only)
    // staged-weight schedule: the three-buffer ring unless OCL_CONV_PIPE=0 asks for the two-buffer one (plan constant: read once)
    static const bool env_pipe = env_int("OCL_CONV_PIPE", 1) != 0;
    const bool pipe = g.force_pipe > 0 || (g.force_pipe == 0 && env_pipe);
    size_t lds = convt_layout(g, a, MT, NT, pipe);
    if (!lds && NT == 2 && !g.force_NT) { NT = 1; lds = convt_layout(g, a, MT, NT, pipe); }
    if (!lds && pipe) lds = convt_layout(g, a, MT, NT, false);
    if (!lds) return OCL_ERR_ARG;
    if (a.pipe) {
        // the ring's third buffer can cost the second workgroup per CU; when the launch has more workgroups than CUs that matters more
        // than the schedule (layer 4's merged data gradient at 220 images: 275 workgroups, 36.7 us with two buffers and two workgroups
        // per CU, 40.6 us with the ring and one: profiles/r2_kbench_ring_v2.txt) -- keep the two-buffer plan there
        ConvArgs b = a;
        const size_t lds2 = convt_layout(g, b, MT, NT, false);
        const int bpc_ring = (int)std::min<size_t>(2, kLdsLimit / (lds + 512));
        const int bpc_two = lds2 ? (int)std::min<size_t>(2, kLdsLimit / (lds2 + 512)) : 0;
        const int64_t wgs = (int64_t)g.groups * (cdiv(a.group_size, a.imgs) * a.tiles_per_img) * a.n_splits;
        if (bpc_two > bpc_ring && wgs > 256 * bpc_ring) {
            a = b;
            lds = lds2;
        }
    }
    a.cls_pack = std::max(1, g.ncls);
    a.cls_oyx = 0;
    for (int c = 0; c < std::max(1, g.ncls); ++c) {
        a.cls_pack |= (g.ncls > 1 ? g.cls_ntaps[c] : g.ntaps) << (4 + 4 * c);
        if (g.ncls > 1) a.cls_oyx |= (g.cls_oy[c] << (2 * c)) | (g.cls_ox[c] << (2 * c + 1));
    }
    p->MT = MT; p->NT = NT;
    p->lds_bytes = lds;
    a.WPT = g.WPT > 0 ? g.WPT : a.CoutP;
    for (int t = 0; t < 9; ++t) a.tpo[t] = t < a.ntaps ? ((a.tdy[t] - a.min_dy) * a.PC + (a.tdx[t] - a.min_dx)) * a.CP : 0;
    {
        const int kc4 = a.KC / 4;
        a.d_c4 = 256 % kc4;
        const int d_pix = 256 / kc4;
        a.d_pc = d_pix % a.PC;
        a.d_row = d_pix / a.PC;
    }
    a.groups = g.groups;
    {
        const int BMp = 64 * NT, LPp = g.LH * g.LW;
        a.aligned = a.imgs > 1 ? 1 : ((BMp % g.LW == 0 && LPp % BMp == 0) ? 1 : 0);
    }
    const int ntiles = g.groups * a.tiles_per_group;
    {
        auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); };
        a.m_tpg = magic(a.tiles_per_group); a.m_tpi = magic(a.tiles_per_img); a.m_lw = magic(a.LW); a.m_ppi = magic(a.ppi);
        a.m_kc4 = magic(a.KC / 4); a.m_pc = magic(a.PC); a.m_pr = magic(a.PR);
        // exactness of x / d by one multiply-high needs x * d < 2^32: the largest dividends are tile and pixel indices
        const int64_t xmax = std::max<int64_t>(std::max<int64_t>(ntiles, (int64_t)g.LH * g.LW + 64 * NT), 4096);
        const int64_t dmax = std::max(std::max(a.tiles_per_group, a.tiles_per_img), std::max(std::max(a.LW, a.ppi), std::max(a.PC, a.PR)));
        if (xmax * dmax >= (1ll << 32)) return OCL_ERR_ARG;
    }
    int bpc = (int)std::min<size_t>(2, kLdsLimit / (lds + 512));
    if (g.force_bpc) bpc = g.force_bpc;
    p->grid_x = std::max(1, std::min(ntiles, (256 * std::max(1, bpc)) / a.n_splits));
    p->grid_x = std::max(p->grid_x, cdiv(ntiles, kMaxWgTiles));   // a workgroup keeps at most kMaxWgTiles tile descriptors
    p->grid_y = a.n_splits;
    // layout of the plan's device tables (conv_plan_tables)
    if (16 + 2 * a.Qpad > 768) return OCL_ERR_ARG;   // the prologue copies the group tables with three predicated loads per thread
    const int PF = convt_pf_for(a.imgs * a.PR * a.PC * (a.KC / 4));
    a.off_tdesc = (int)round_up(16 + 2 * a.Qpad, 4);
    a.off_pu = a.off_tdesc + ntiles * 8;
    a.off_loc = a.off_pu + 3 * PF * 256;
    a.blob_ints = a.off_loc + 3 * NT * 256;
    a.blob = nullptr;
    return OCL_OK;
}

// ---- the plan's tables: every value the kernel's prologue used to compute per workgroup and per launch -------------------------
void conv_plan_tables(const ConvPlan& p, std::vector<int>* out) {
    if (p.cw) {
        conv_w_tables(p, out);
        return;
    }
    const ConvArgs& a = p.a;
    const int NT = p.NT, MT = p.MT;
    (void)MT;
    const int kc4 = a.KC / 4;
    const int ncls = a.cls_pack & 15;
    const bool pipe = a.pipe != 0, res = a.wres != 0;
    std::vector<int>& b = *out;
    b.assign((size_t)a.blob_ints, 0);
    int* ctab = b.data();
    int* qoff = ctab + 16;
    int* qrow = qoff + a.Qpad;
    // K groups: class by class, each class padded to whole rounds of 4 groups
    {
        int q0 = 0, t0 = 0;
        for (int c = 0; c < ncls; ++c) {
            const int ntc = (a.cls_pack >> (4 + 4 * c)) & 15, nq = (ntc * kc4 + 3) & ~3;
            for (int ql = 0; ql < nq; ++ql) {
                const int q = q0 + ql;
                const bool ok = ql < ntc * kc4;
                const int t = t0 + ql / kc4, c4 = ql % kc4;
                qoff[q] = ok ? a.tpo[t] + 4 * c4 : 0;
                // ring: the BYTE offset of the pack row (bit 31 = past every buffer descriptor: such a load returns zeros)
                qrow[q] = ok ? (a.tw[t] * a.C4tot + c4) * (pipe ? a.WPT * 16 : 1) : (pipe ? (int)0x80000000 : -1);
            }
            if (ncls > 1) {
                const int oy = (a.cls_oyx >> (2 * c)) & 1, ox = (a.cls_oyx >> (2 * c + 1)) & 1;
                ctab[c * 4 + 0] = q0;
                ctab[c * 4 + 1] = nq;
                ctab[c * 4 + 2] = (oy * a.Wout + ox) * a.Cout;
                ctab[c * 4 + 3] = res ? 1 : (nq + a.QS - 1) / a.QS;
            }
            q0 += nq; t0 += ntc;
        }
        for (int q = q0; q < a.Qpad; ++q) {   // (conv_s_kernel pads to whole loop bodies: groups that load no weights)
            qoff[q] = 0;
            qrow[q] = pipe ? (int)0x80000000 : -1;
        }
        if (ncls > 1)
            for (int c = ncls; c < 4; ++c) ctab[c * 4 + 0] = q0;   // (classes past the last: first group = end, no groups)
    }
    // tile descriptors
    const int LP = a.LH * a.LW;
    const int ntiles = a.groups * a.tiles_per_group;
    int* td = b.data() + a.off_tdesc;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int grp = tile / a.tiles_per_group, tg_ = tile % a.tiles_per_group;
        const int ti = tg_ / a.tiles_per_img, tp = tg_ % a.tiles_per_img;
        const int img0 = grp * a.group_size + ti * a.imgs;
        const int p0 = tp * a.ppi;
        const int grp_end = std::min(a.N, (grp + 1) * a.group_size);
        const int ly0 = p0 / a.LW;
        const int pend = std::min(p0 + a.ppi, LP);
        const int ly1 = (pend - 1) / a.LW;
        const int nimg = std::min(a.imgs, grp_end - img0);
        const int nrows = a.imgs > 1 ? nimg * a.PR : (ly1 - ly0) * a.is + (a.max_dy - a.min_dy) + 1;
        const int iy0 = ly0 * a.is + a.min_dy;
        int* d = td + (size_t)tile * 8;
        d[0] = (((img0 * a.Hin + iy0) * a.Win + a.min_dx) * a.Cin) * 4;                // input byte offset of the patch origin
        d[1] = iy0;
        d[2] = nrows;
        d[3] = ((img0 * a.Hout + ly0 * a.os + a.oy0) * a.Wout + a.ox0) * a.Cout;         // output element offset of the tile origin
        d[4] = nimg;
        d[5] = grp;
        d[6] = p0;
        d[7] = img0 | (ly0 << 20);
    }
    // per-thread patch units: unit u = tid + i * 256 of the flat [row][pc][c4] patch
    const int PF = (a.off_loc - a.off_pu) / (3 * 256);
    int* pu = b.data() + a.off_pu;
    for (int tid = 0; tid < (p.cs ? 64 : 256); ++tid) {   // (conv_s_kernel: a wave's 64 lanes walk the units, stride 64)
        const int pix = tid / kc4;
        int c4 = tid % kc4, row = pix / a.PC, pc = pix % a.PC;
        for (int i = 0; i < PF; ++i) {
            int il = 0, pr = row;
            if (a.imgs > 1) { il = row / a.PR; pr = row % a.PR; }
            const int ix = a.min_dx + pc;
            const bool xok = ix >= 0 && ix < a.Win;               // columns of the halo outside the image: zeros (never loaded, still stored)
            pu[(3 * i + 0) * 256 + tid] = xok ? (((il * a.Hin + pr) * a.Win + pc) * a.Cin + c4 * 4) * 4 : -1;
            pu[(3 * i + 1) * 256 + tid] = (row * a.PC + pc) * a.CP + c4 * 4;
            pu[(3 * i + 2) * 256 + tid] = (il < 128 && pr < 256) ? (row | (pr << 16) | (c4 << 24)) : 0x7fff;   // row 0x7fff: past every tile's last row; bits 24+: channel quad
            c4 += a.d_c4;
            pc += a.d_pc;
            if (c4 >= kc4) { c4 -= kc4; pc += 1; }
            row += a.d_row;
            if (pc >= a.PC) { pc -= a.PC; row += 1; }
        }
    }
    // per-lane output pixels relative to the tile origin
    int* lc = b.data() + a.off_loc;
    for (int tid = 0; tid < 256; ++tid) {
        const int wave = tid >> 6, r16 = tid & 15, lane = tid & 63;
        for (int nt = 0; nt < NT; ++nt) {
            // conv_t_kernel: 16-pixel tiles, the lane's pixel = its r16; conv_q_kernel: 64-pixel sets, one pixel per lane
            // conv_s_kernel: every wave holds the same 16 NT pixels
            const int r = p.cs ? nt * 16 + r16 : p.q4 ? wave * 64 * NT + nt * 64 + lane : wave * 16 * NT + nt * 16 + r16;
            const int il = r / a.ppi, pl = r % a.ppi;
            const int ly = pl / a.LW, lx = pl % a.LW;
            lc[(3 * nt + 0) * 256 + tid] = ((il * a.PR + ly * a.is) * a.PC + lx * a.is) * a.CP;
            lc[(3 * nt + 1) * 256 + tid] = ((il * a.Hout + ly * a.os) * a.Wout + lx * a.os) * a.Cout;
            lc[(3 * nt + 2) * 256 + tid] = il;
        }
    }
}

int conv_plan_finalize(ConvPlan* p, PlanArena* arena, hipStream_t s) {
    if (p->a.blob) return OCL_OK;
    if (!arena) {
        std::vector<int> t;
        conv_plan_tables(*p, &t);
        int* d = nullptr;
        OCL_HIP(hipMalloc((void**)&d, t.size() * sizeof(int)));
        OCL_HIP(hipMemcpy(d, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
        p->a.blob = d;
        return OCL_OK;
    }
    std::vector<int>* t = new std::vector<int>();
    arena->host_keep.push_back(t);
    conv_plan_tables(*p, t);
    const size_t bytes = (size_t)round_up((int64_t)t->size() * sizeof(int), 256);
    if (arena->chunks.empty() || arena->used + bytes > arena->cap) {
        const size_t cap = std::max<size_t>(8u << 20, bytes);
        void* c = nullptr;
        OCL_HIP(hipMalloc(&c, cap));
        {
            if (log_plans()) fprintf(stderr, "[ocl] plan-table arena: chunk %zu allocated (%zu bytes)\n", arena->chunks.size() + 1, cap);
        }
        arena->chunks.push_back(c);
        arena->used = 0;
        arena->cap = cap;
    }
    int* d = (int*)((char*)arena->chunks.back() + arena->used);
    arena->used += bytes;
    OCL_HIP(hipMemcpyAsync(d, t->data(), t->size() * sizeof(int), hipMemcpyHostToDevice, s));
    hipEvent_t e;
    OCL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    arena->events.push_back(e);
    OCL_HIP(hipEventRecord(e, s));
    p->ready = e;
    p->ready_stream = s;
    p->a.blob = d;
    return OCL_OK;
}
void plan_arena_release(PlanArena* a) {
    for (hipEvent_t e : a->events) (void)hipEventDestroy(e);
    a->events.clear();
    for (void* c : a->chunks) (void)hipFree(c);
    for (auto* v : a->host_keep) delete v;
    a->chunks.clear();
    a->host_keep.clear();
    a->used = a->cap = 0;
}
void conv_plan_release(ConvPlan* p) {
    if (p->a.blob) (void)hipFree((void*)p->a.blob);
    p->a.blob = nullptr;
}

int plan_conv(const ConvGeomDesc& g, ConvPlan* p) {
    memset(p, 0, sizeof(*p));
    ConvArgs& a = p->a;
    OCL_REQUIRE(g.N > 0 && g.groups > 0 && g.N % g.groups == 0, "plan_conv: N=%d not divisible into %d groups", g.N, g.groups);
    OCL_REQUIRE(g.Cin % 4 == 0 && g.Cout % 4 == 0 && g.ntaps >= 1 && g.ntaps <= 9, "plan_conv: Cin=%d Cout=%d ntaps=%d", g.Cin,
                g.Cout, g.ntaps);
    OCL_REQUIRE(g.LH > 0 && g.LW > 0, "plan_conv: empty lattice");
    a.N = g.N; a.Hin = g.Hin; a.Win = g.Win; a.Cin = g.Cin;
    a.Hout = g.Hout; a.Wout = g.Wout; a.Cout = g.Cout;
    a.LH = g.LH; a.LW = g.LW; a.os = g.os; a.oy0 = g.oy0; a.ox0 = g.ox0; a.is = g.is;
    a.ntaps = g.ntaps;
    a.min_dy = a.min_dx = 1 << 20;
    a.max_dy = a.max_dx = -(1 << 20);
    for (int t = 0; t < g.ntaps; ++t) {
        a.tdy[t] = g.tdy[t]; a.tdx[t] = g.tdx[t]; a.tw[t] = g.tw[t];
        a.min_dy = std::min(a.min_dy, g.tdy[t]); a.max_dy = std::max(a.max_dy, g.tdy[t]);
        a.min_dx = std::min(a.min_dx, g.tdx[t]); a.max_dx = std::max(a.max_dx, g.tdx[t]);
    }
    if (plan_conv_t(g, p) != OCL_OK) {
        set_error("plan_conv: no tiling fits (Hin=%d Win=%d Cin=%d Cout=%d taps=%d classes=%d, forced MT=%d NT=%d)", g.Hin, g.Win, g.Cin, g.Cout,
                  g.ntaps, g.ncls, g.force_MT, g.force_NT);
        return OCL_ERR_ARG;
    }
    return OCL_OK;
}

int pack_width(int channels) { return (int)round_up(channels, 16); }

void geom_fwd(const ConvShape& c, int N, int groups, ConvGeomDesc* g) {
    memset(g, 0, sizeof(*g));
    g->N = N; g->groups = groups;
    g->Hin = c.Hin; g->Win = c.Win; g->Cin = c.CinT;
    g->Hout = c.Ho; g->Wout = c.Wo; g->Cout = c.Cout;
    g->LH = c.Ho; g->LW = c.Wo; g->os = 1; g->oy0 = 0; g->ox0 = 0; g->is = c.stride;
    g->WPT = c.CoutP;
    const int pad = c.k == 3 ? 1 : 0;
    g->ntaps = c.k * c.k;
    for (int t = 0; t < g->ntaps; ++t) {
        g->tdy[t] = t / c.k - pad;
        g->tdx[t] = t % c.k - pad;
        g->tw[t] = t;
    }
}

void geom_dgrad(const ConvShape& c, int N, std::vector<ConvGeomDesc>* out, bool merge_classes, int groups) {
    out->clear();
    ConvGeomDesc g;
    memset(&g, 0, sizeof(g));
    g.N = N; g.groups = groups;
    g.Hin = c.Ho; g.Win = c.Wo; g.Cin = c.Cout;
    g.Hout = c.Hin; g.Wout = c.Win; g.Cout = c.Cin;
    g.is = 1;
    g.WPT = c.CiP;
    if (c.stride == 1) {
        g.LH = c.Hin; g.LW = c.Win; g.os = 1;
        const int pad = c.k == 3 ? 1 : 0;
        g.ntaps = c.k * c.k;
        for (int t = 0; t < g.ntaps; ++t) {
            g.tdy[t] = pad - t / c.k;
            g.tdx[t] = pad - t % c.k;
            g.tw[t] = t;
        }
        out->push_back(g);
    } else if (c.k == 1) {  // 1x1 stride 2, pad 0: only even pixels receive gradient
        g.os = 2; g.oy0 = 0; g.ox0 = 0;
        g.LH = (c.Hin + 1) / 2; g.LW = (c.Win + 1) / 2;
        g.ntaps = 1;
        g.tdy[0] = 0; g.tdx[0] = 0; g.tw[0] = 0;
        out->push_back(g);
    } else if (merge_classes && c.Hin % 2 == 0 && c.Win % 2 == 0) {
        // the four parity classes as output classes of one launch: they read the same dy window (rows / columns +0, +1), use
        // disjoint taps (1, 2, 2 and 4 of the 9) and write the four interleaved lattices of dx
        g.os = 2; g.oy0 = 0; g.ox0 = 0;
        g.LH = c.Hin / 2; g.LW = c.Win / 2;
        g.ncls = 4;
        int nt = 0;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const int cls = py * 2 + px;
                g.cls_oy[cls] = py; g.cls_ox[cls] = px;
                const int first = nt;
                for (int ky = 0; ky < 3; ++ky) {
                    if (((py + 1 - ky) & 1) != 0) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        if (((px + 1 - kx) & 1) != 0) continue;
                        g.tdy[nt] = (py + 1 - ky) / 2;
                        g.tdx[nt] = (px + 1 - kx) / 2;
                        g.tw[nt] = ky * 3 + kx;
                        ++nt;
                    }
                }
                g.cls_ntaps[cls] = nt - first;
            }
        g.ntaps = nt;
        out->push_back(g);
    } else {  // 3x3 stride 2 pad 1: four dense parity classes of the dx lattice
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                ConvGeomDesc q = g;
                q.os = 2; q.oy0 = py; q.ox0 = px;
                q.LH = (c.Hin - py + 1) / 2; q.LW = (c.Win - px + 1) / 2;
                if (q.LH <= 0 || q.LW <= 0) continue;
                int nt = 0;
                for (int ky = 0; ky < 3; ++ky) {
                    if (((py + 1 - ky) & 1) != 0) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        if (((px + 1 - kx) & 1) != 0) continue;
                        q.tdy[nt] = (py + 1 - ky) / 2;  // exact: even numerator
                        q.tdx[nt] = (px + 1 - kx) / 2;
                        q.tw[nt] = ky * 3 + kx;
                        ++nt;
                    }
                }
                q.ntaps = nt;
                out->push_back(q);
            }
    }
}

int launch_conv(const ConvPlan& p, hipStream_t s) {
    if (p.cw) return launch_conv_w(p, s);
    if (p.cs) {
        if (!p.a.blob) {
            set_error("launch_conv: plan without device tables (conv_plan_finalize)");
            return OCL_ERR_STATE;
        }
        ProfScope ps(PROF_CONV, s);
        const int det = det_host();
        hipLaunchKernelGGL(convs_fn(p.NT, p.a.trace != nullptr && !det, (p.a.flags & EPI_BNB) != 0, det != 0), dim3(p.grid_x, p.grid_y), dim3(256),
                           p.lds_bytes, s, p.a);
        OCL_LAUNCH_CHECK();
        return OCL_OK;
    }
    if (p.q4) {
        conv_fn_t fq = convq_fn(p.q4, (p.a.off_loc - p.a.off_pu) / (3 * 256), (p.a.flags & EPI_BNB) ? 2 : (p.a.flags & EPI_STATS) ? 1 : 0);
        if (p.a.trace)
            if (conv_fn_t ft = convq_trace_fn(p.q4, (p.a.off_loc - p.a.off_pu) / (3 * 256), (p.a.flags & EPI_BNB) ? 2 : (p.a.flags & EPI_STATS) ? 1 : 0)) {
                fq = ft;
                OCL_HIP(hipFuncSetAttribute((const void*)fq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
            }
        if (!fq || !p.a.blob) {
            set_error("launch_conv: no conv_q_kernel for q4=%d / plan without device tables", p.q4);
            return OCL_ERR_STATE;
        }
        ProfScope ps(PROF_CONV, s);
        hipLaunchKernelGGL(fq, dim3(p.grid_x, p.grid_y), dim3(256), p.lds_bytes, s, p.a);
        OCL_LAUNCH_CHECK();
        return OCL_OK;
    }
    conv_fn_t fn = convt_fn(p.MT, p.NT, convt_plan_pf(p), p.a.wres, (p.a.cls_pack & 15) > 1, p.a.pipe,
                            (p.a.flags & EPI_BNB) ? 1 : 0);
    if (!fn) {
        set_error("launch_conv: no kernel for MT=%d NT=%d", p.MT, p.NT);
        return OCL_ERR_STATE;
    }
    if (!p.a.blob) {
        set_error("launch_conv: plan without device tables (conv_plan_finalize)");
        return OCL_ERR_STATE;
    }
    ProfScope ps(PROF_CONV, s);
    hipLaunchKernelGGL(fn, dim3(p.grid_x, p.grid_y), dim3(256), p.lds_bytes, s, p.a);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// Allow every instantiation to use the full 160 KiB of dynamic LDS.
int conv_kernels_init() {
    static bool done_dev[kMaxDevices] = {false};   // function attributes and the mode symbol are per device
    int dev = 0;
    OCL_HIP(hipGetDevice(&dev));
    OCL_REQUIRE(dev >= 0 && dev < kMaxDevices, "conv_kernels_init: device %d", dev);
    bool& done = done_dev[dev];
    if (done) return OCL_OK;
    if (env_on("OCL_DETERMINISTIC")) {
        int rc = set_deterministic_sums(1);
        if (rc != OCL_OK) return rc;
    }
    if (int rc = wgrad_kernels_init()) return rc;
    if (int rc = convw_kernels_init()) return rc;
    for (int m = 1; m <= 5; ++m)
        for (int n = 1; n <= 2; ++n)
            for (int pf = 4; pf <= 8; pf += 4)
                for (int res = 0; res < 2; ++res)
                    OCL_HIP(hipFuncSetAttribute((const void*)convt_fn(m, n, pf, res), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    for (int m = 1; m <= 5; ++m)
        for (int pf = 4; pf <= 8; pf += 4)
            for (int res = 0; res < 2; ++res)
                OCL_HIP(hipFuncSetAttribute((const void*)convt_fn(m, 1, pf, res, 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    for (int m = 1; m <= 5; ++m)
        for (int pf = 4; pf <= 8; pf += 4)
            for (int cls = 0; cls < 2; ++cls)
                OCL_HIP(hipFuncSetAttribute((const void*)convt_fn(m, 1, pf, 0, cls, 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    for (int nt = 1; nt <= 2; ++nt)
        for (int tr = 0; tr < 2; ++tr)
            OCL_HIP(hipFuncSetAttribute((const void*)convs_fn(nt, tr != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    // the EPI_BNB instantiations
    for (int m = 1; m <= 5; ++m)
        for (int pf = 4; pf <= 8; pf += 4) {
            for (int n = 1; n <= 2; ++n)
                for (int res = 0; res < 2; ++res)
                    OCL_HIP(hipFuncSetAttribute((const void*)convt_fn(m, n, pf, res, 0, 0, 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
            OCL_HIP(hipFuncSetAttribute((const void*)convt_fn(m, 1, pf, 0, 0, 1, 1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
        }
    for (int nt = 1; nt <= 2; ++nt)
        for (int det = 0; det < 2; ++det)
            for (int bnb = det ? 0 : 1; bnb < 2; ++bnb)
                OCL_HIP(hipFuncSetAttribute((const void*)convs_fn(nt, false, bnb != 0, det != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    for (int st = 0; st < 3; ++st) {
        OCL_HIP(hipFuncSetAttribute((const void*)convq_fn(2, 4, st), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
        OCL_HIP(hipFuncSetAttribute((const void*)convq_fn(2, 12, st), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
        OCL_HIP(hipFuncSetAttribute((const void*)convq_fn(1, 12, st), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
    }
    done = true;
    return OCL_OK;
}

}  // namespace ocl
