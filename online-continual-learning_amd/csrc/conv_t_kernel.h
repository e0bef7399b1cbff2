// K1: the Reduced-ResNet18 convolution kernel for gfx950.
//
//  conv_t_kernel      implicit-GEMM 3x3 / 1x1 convolution on exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), D[channel][pixel] tiles with
//                     K-grouped operands.  One generic "tap list + output lattice" geometry covers forward (stride 1/2), data
//                     gradient (stride 1; stride 2 as four parity classes, in one launch where the lattices coincide) and the
//                     1x1 shortcut.  The input patch (with halo) of a 64/128-pixel tile is staged ONCE in LDS and reused by
//                     all taps; weights are resident in LDS or stream through a double-buffered stage.  Epilogues from
//                     registers: BN batch statistics (fp64 atomics), folded eval-mode BN, residual, ReLU, masked residual.
//
// The kernel template only: conv_t.hip instantiates the plain forms, conv_t_bnb.hip the EPI_BNB forms (two translation units that compile
// side by side); the planner and the launch are in conv.hip.
#pragma once
#include "conv_stats_dev.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <cmath>

namespace ocl {

// =====================================================================================================
// conv_t_kernel: channels x pixels orientation with K-grouped operands
// =====================================================================================================
// D[channel][pixel] tiles: the MFMA's A operand is the weight (row = output channel), B the input patch (column = output pixel).
//  * K runs over (tap, channel quad) GROUPS q; a round of 4 MFMAs covers 4 groups, one per lane quarter g = lane >> 4, and MFMA
//    j of the round multiplies channel 4*c4(q_g) + j.  Any one-to-one assignment of k slots works as long as A and B agree, and
//    this one makes the 4 operands a lane needs for a round ONE 16-byte LDS read each: B from the pixel-major patch (channels
//    contiguous), A from the K-grouped pack [q][channel][4].  Per round a wave issues 1 + NT + MT LDS reads for 4*MT*NT MFMAs
//    (the round-1 kernel, pixels x channels tiles: 4*(MT+NT) 4-byte reads and their address arithmetic).
//  * A lane's 4 accumulator registers are 4 CONSECUTIVE output channels of one pixel: the epilogue (statistics, folded BatchNorm,
//    residual, mask, ReLU, accumulate) works on registers and stores 16-byte vectors straight to the NHWC tensor: no LDS
//    transpose, no barriers after the MFMAs.
//  * Weights of the small layers (<= kResidentBytes per channel split) are copied to LDS ONCE per persistent workgroup; the others
//    stream through a double-buffered stage of QS groups, fetched one stage ahead into registers.
//  * BatchNorm statistics: fp32 per-lane partials over the workgroup's tiles, fp64 from the cross-lane reduction on, flushed with
//    one fp64 atomic per channel per workgroup (8 replicas, as above).

// PIPE variant of the staged-weight path (the default since round 3; OCL_CONV_PIPE=0 / ConvGeomDesc::force_pipe = -1 select the
// two-buffer schedule).  Bit-identical to it on the whole network (tests/test_gpu_ring.py), 18 - 21 % faster per staged launch.  The two-buffer
// schedule pays, per stage and with one workgroup per CU, a serial section nothing overlaps: the table look-ups and loads of the
// next stage (4 dependent LDS round trips), the commit, a barrier and the first operand reads (~1900 of ~3800 cycles around 60
// MFMAs, profiles/r2_kbench_conv_staged_trace.txt).  Here the stages of a (tile, class, chunk) form ONE software-pipelined round
// sequence: weights go through a ring of three stage buffers, the registers hold the stage after next, and the stage's single
// barrier sits in the middle of its first round (after the commit of the next stage), so operand reads run across stage boundaries:
//    first round of stage t:  operand reads of round 1 | commit regs -> buffer (t+1)%3, look up the rows of stage t+2 |
//                             MFMAs of round 0 | loads of stage t+2 -> regs, barrier | ...
//  * buffer (t+1)%3 was last read in stage t-2, which every wave left before the barrier of stage t-1;
//  * stage t+1 is read after the barrier of stage t, which follows every wave's commit.
// (Stage geometry by MT: pipe_qs / pipe_wpf, conv_dev.h.)

// BNB: instantiated with the EPI_BNB epilogue (its registers must not weigh on the other launches: the forward instantiations sit at the
// edge of their occupancy step)
template <int MT, int NT, int PF, bool RES, bool CLS = false, bool PIPE = false, bool BNB = false>   // CLS: several output classes per tile (merged parity classes of a stride-2 data gradient)
__global__ void __launch_bounds__(256, PIPE ? 1 : 2) conv_t_kernel(const ConvArgs a) {   // PIPE plans run one workgroup per CU (three stage buffers): all 512 registers
    static_assert(!(PIPE && RES), "the ring is a schedule of the staged-weight path");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int COPW = 16 * MT;              // channels per workgroup (one channel split)
    constexpr int WPF = RES ? 1 : (PIPE ? pipe_wpf(MT) : kWPF);   // float4 weight-prefetch registers per thread
    constexpr int QSP = pipe_qs(MT);           // PIPE: groups per stage (== a.QS)
    int* tdesc = (int*)lds_raw;                // [kMaxWgTiles][8] per-tile geometry of this workgroup's tile range
    int* ctab = tdesc + kMaxWgTiles * 8;       // [4][4] per output class: first group, groups (padded to rounds), output offset, weight stages
    int* qoff = ctab + 16;                     // [Qpad] patch offset (floats) of group q relative to a pixel's origin
    int* qrow = qoff + a.Qpad;                 // [Qpad] row of the K-grouped pack (tap * C4tot + channel quad), -1: padding group
    float* wl = (float*)(qrow + a.Qpad);       // resident: [Qpad][COPW][4]; staged: [2][QS][COPW][4]; PIPE: [3][QS][COPW][4]
    float* patch = wl + (size_t)(RES ? a.Qpad : (PIPE ? 3 : 2) * a.QS) * COPW * 4;   // [imgs][PR][PC][CP]
    float* xft = patch + a.patch_floats;       // input transform: [groups][Cin/4][2][4] scale quads / shift quads
    const float* bnt = xft + (a.bnb_lds > 0 ? a.bnb_lds : 0);   // EPI_BNB: [groups][Cout/4][3][4] scale, shift, mean quads of the BatchNorm being differentiated

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.y * COPW;
    const int LP = a.LH * a.LW;
    const int ntiles_all = a.groups * a.tiles_per_group;
    // contiguous tile range of this workgroup: neighbouring tiles share halo rows (L2) and one BatchNorm group
    const int t_begin = (int)(((int64_t)blockIdx.x * ntiles_all) / gridDim.x), t_end = (int)(((int64_t)(blockIdx.x + 1) * ntiles_all) / gridDim.x);
    const int nwt = t_end - t_begin;
    if (nwt <= 0) return;
    const int flags = BNB ? a.flags : (a.flags & ~EPI_BNB);
    int tr_n = 0;
    auto stamp = [&]() __attribute__((always_inline)) {
        if (a.trace && tid == 0 && tr_n < 64) a.trace[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 + tr_n++] = __builtin_amdgcn_s_memtime();
    };
    stamp();   // 0: start
    // ---- tables ------------------------------------------------------------------------------------------------------------------
    // Everything that depends only on the plan -- the K-group tables, the geometry of every tile, every thread's patch units and
    // output pixels -- is computed ONCE on the host when the plan is made (conv_plan_tables) and sits in device memory next to the
    // plan: the prologue is a handful of independent loads instead of ~8 k cycles of integer arithmetic, dependent LDS round trips
    // and kernel-argument fetches per launch (profiles/r3_kbench_conv_220_trace.txt; rounds 1 - 2 built them here, per workgroup).
    const int ncls = CLS ? (a.cls_pack & 15) : 1;
    const int* __restrict__ blob = a.blob;
    int pu_goff[PF], pu_lds[PF], pu_rp[PF];   // per-thread patch units (float4 along the channels): global byte offset from the patch origin; LDS float offset; row | pr << 16
    {
        const int* pu = blob + a.off_pu + tid;
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            pu_goff[i] = pu[(3 * i + 0) * 256];
            pu_lds[i] = pu[(3 * i + 1) * 256];
            pu_rp[i] = pu[(3 * i + 2) * 256];
        }
    }
    // the lane's NT pixels relative to the tile origin (aligned plans: tile-invariant)
    int loc_p[NT], loc_o[NT], loc_il[NT];
    {
        const int* lc = blob + a.off_loc + tid;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            loc_p[nt] = lc[(3 * nt + 0) * 256];
            loc_o[nt] = lc[(3 * nt + 1) * 256];
            loc_il[nt] = lc[(3 * nt + 2) * 256];
        }
    }
    const int4 tile0 = *(const int4*)(blob + a.off_tdesc + (size_t)t_begin * 8);   // first tile: in_base, iy0, nrows, obase (block-uniform)
    // class table + group tables (contiguous in the blob and in LDS: 16 + 2 * Qpad <= 768 ints, checked by the planner) and this
    // workgroup's tile descriptors (<= kMaxWgTiles * 8 = 512 ints): predicated loads, requested BEFORE the first patch (loads return in order: the stores
    // below then wait for the tables only, not for the patch)
    const int ntab = 16 + 2 * a.Qpad, ntd = nwt * 8;
    const int* td = blob + a.off_tdesc + (size_t)t_begin * 8;
    const int tab0 = tid < ntab ? blob[tid] : 0, tab1 = tid + 256 < ntab ? blob[tid + 256] : 0, tab2 = tid + 512 < ntab ? blob[tid + 512] : 0;
    const int td0 = tid < ntd ? td[tid] : 0, td1 = tid + 256 < ntd ? td[tid + 256] : 0;
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(a.in), rs_w = make_rsrc(a.wT);
    float4 pv[PF];
    unsigned okm = 0;   // bit i: unit i of the patch in flight lies inside the image (input transform: the others stay zero)
    auto load_patch_d = [&](const int4 d, int c0) __attribute__((always_inline)) {   // d: in_base, iy0, nrows, obase
        const int base = d.x + c0 * 4;
        okm = 0;
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int row = pu_rp[i] & 0xffff, pr = (pu_rp[i] >> 16) & 0xff;
            const bool ok = (row < d.z) & ((unsigned)(d.y + pr) < (unsigned)a.Hin) & (pu_goff[i] >= 0);
            pv[i] = buf_load16(rs_in, ok ? base + pu_goff[i] : kOob);
            okm |= ok ? (1u << i) : 0u;
        }
    };
    // grp / c0: BatchNorm group of the tile and channel origin of the chunk being stored (input transform only)
    auto store_patch = [&](int nrows, int grp, int c0) __attribute__((always_inline)) {
        if (a.xf) {   // block-uniform
            const float* tb = xft + (size_t)(grp * a.C4tot + (c0 >> 2)) * 8;
#pragma unroll
            for (int i = 0; i < PF; ++i)
                if ((pu_rp[i] & 0xffff) < nrows) {
                    const float* t = tb + (pu_rp[i] >> 24) * 8;
                    const float4 sc = *(const float4*)t, sh = *(const float4*)(t + 4);
                    float4 v = pv[i];
                    v.x = fmaxf(__fmaf_rn(v.x, sc.x, sh.x), 0.f); v.y = fmaxf(__fmaf_rn(v.y, sc.y, sh.y), 0.f);
                    v.z = fmaxf(__fmaf_rn(v.z, sc.z, sh.z), 0.f); v.w = fmaxf(__fmaf_rn(v.w, sc.w, sh.w), 0.f);
                    if (!((okm >> i) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4*)(patch + pu_lds[i]) = v;
                }
            return;
        }
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if ((pu_rp[i] & 0xffff) < nrows) {   // CP % 4 == 0: 16-byte aligned
                *(float4*)(patch + pu_lds[i]) = pv[i];
            }
    };
    auto load_patch = [&](int k, int c0) __attribute__((always_inline)) { load_patch_d(*(const int4*)(tdesc + k * 8), c0); };
    load_patch_d(tile0, 0);
    if (a.xf) {   // the producer's BatchNorm folded into scale / shift per (group, channel); see ConvArgs::xf
        const int C = a.Cin;
        const double M = (double)a.xf_m_per_group;
        const bool lead = blockIdx.x == 0 && blockIdx.y == 0;
        for (int j = tid; j < a.groups * C; j += 256) {
            const int gq = j / C, c = j - gq * C;
            double mean, var;
            bn_batch_moments(a.xf_stats, a.xf_rep_stride, gq, c, C, M, mean, var);
            // 1 / sqrt(var + eps) without the fp64 divide / square-root sequences (every workgroup of the launch runs this prologue):
            // fp32 rsqrt seed + two Newton steps in fp64 (relative error < 1e-15: the float it is rounded to is the exact one)
            const double xv = var + (double)a.xf_eps;
            double invstd = (double)rsqrtf((float)xv);
            invstd = invstd * (1.5 - 0.5 * xv * invstd * invstd);
            invstd = invstd * (1.5 - 0.5 * xv * invstd * invstd);
            float sc, sh;
            bn_scale_shift(a.xf_gamma[c], a.xf_beta[c], (float)mean, (float)invstd, sc, sh);
            float* t = xft + (size_t)(gq * (C >> 2) + (c >> 2)) * 8 + (c & 3);
            t[0] = sc;
            t[4] = sh;
            if (lead) {
                a.xf_save_mean[j] = (float)mean;
                a.xf_save_invstd[j] = (float)invstd;
            }
        }
        if (lead && a.xf_running_mean)
            bn_running_update(a.xf_stats, a.xf_rep_stride, a.groups, C, M, a.xf_momentum, a.xf_running_mean, a.xf_running_var, a.xf_nbt, tid, 256);
    }
    if (BNB && (flags & EPI_BNB)) bnb_table(a, const_cast<float*>(bnt), tid, 256);
    if (tid < ntab) ctab[tid] = tab0;
    if (tid + 256 < ntab) ctab[tid + 256] = tab1;
    if (tid + 512 < ntab) ctab[tid + 512] = tab2;
    if (tid < ntd) tdesc[tid] = td0;
    if (tid + 256 < ntd) tdesc[tid + 256] = td1;

    stamp();   // P1: tables written, first patch requested
    __syncthreads();   // tables visible
    stamp();   // P2: barrier
    // ---- weights ----------------------------------------------------------------------------------------------------------
    const int wcol_ok = a.WPT - n0;   // columns of this split that exist in the pack
    if (RES) {
        // global -> LDS without registers (buffer_load ... lds): a wave instruction fills 64 consecutive 16-byte units (LDS address =
        // wave-uniform base + lane * 16, global address per lane); everything is in flight at once, one wait at the end.  Padding
        // groups / channels past the pack address the descriptor's out-of-range area, which reads as zeros.
        const int units = a.Qpad * COPW;
#pragma unroll 4
        for (int u0 = wave * 64; u0 < units; u0 += 256) {
            const int u = u0 + lane;
            const int q = min(u, units - 1) / COPW, c = min(u, units - 1) - q * COPW;
            const int row = qrow[q];
            const int off = (u < units && row >= 0 && c < wcol_ok) ? ((row * a.WPT + n0 + c) * 4) * 4 : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(wl + (size_t)u0 * 4), 16, off, 0, 0, 0);
        }
    }
    stamp();   // P3: weight DMA issued
    // staged: stage s of chunk c0 covers groups [s*QS, s*QS + QS); unit u = tid + i*256 -> (group in stage, channel)
    float4 wv[WPF];
    auto w_prefetch = [&](int s_, int c0_, int cls) __attribute__((always_inline)) {
        const int q0 = (CLS ? ctab[cls * 4] : 0) + s_ * a.QS, qend = CLS ? ctab[cls * 4] + ctab[cls * 4 + 1] : a.Qpad;
        const int c4base = c0_ >> 2;
#pragma unroll
        for (int i = 0; i < WPF; ++i) {
            const int u = tid + i * 256;
            const int qq = u / COPW, c = u - qq * COPW;
            const int q = q0 + qq;
            const int row = (qq < a.QS && q < qend) ? qrow[q] : -1;
            wv[i] = buf_load16(rs_w, (row >= 0 && c < wcol_ok) ? (((row + c4base) * a.WPT + n0 + c) * 4) * 4 : kOob);
        }
    };
    auto w_commit = [&](int buf) __attribute__((always_inline)) {
        float* dst = wl + (size_t)buf * a.QS * COPW * 4;
#pragma unroll
        for (int i = 0; i < WPF; ++i) {
            const int u = tid + i * 256;
            if (u < a.QS * COPW) *(float4*)(dst + (size_t)u * 4) = wv[i];
        }
    };
    // ---- PIPE: the prefetch cursor runs two stages ahead of the MFMAs (stage in class-chunk, chunk origin, class, tile; the class's
    // first group / group count / stage count); the look-up, the loads and the commit are separate steps so that each sits where its
    // latency is covered (see the schedule above).  Past the workgroup's last stage the cursor simply wraps to the first tile's stages
    // (two stages of loads nobody reads).
    int pf_s = 0, pf_c0 = 0, pf_cls = 0, pf_q0 = 0, pf_nq = a.Qpad, pf_nst = a.nstage;
    int xb = 0;                                // ring buffer of the stage whose MFMAs issue
    // The look-up only READS the table (its consumers come after a round of MFMAs: no wait in between).  No bounds beyond the table's:
    // groups past the class's last one (partial last stage) or past the workgroup's last stage fetch rows no MFMA reads.
    int prow[PIPE ? WPF : 1];
    auto pf_lookup = [&]() __attribute__((always_inline)) {
        const int qs0 = pf_q0 + pf_s * QSP;
#pragma unroll
        for (int i = 0; i < (PIPE ? WPF : 1); ++i) prow[i] = qrow[min(qs0 + (tid + i * 256) / COPW, a.Qpad - 1)];
    };
    auto pf_issue = [&]() __attribute__((always_inline)) {
        const int cb = (pf_c0 >> 2) * a.WPT * 16;   // chunk origin in the pack, bytes
#pragma unroll
        for (int i = 0; i < (PIPE ? WPF : 1); ++i) {
            const int u = tid + i * 256;
            const int c = u - (u / COPW) * COPW;
            wv[i] = buf_load16(rs_w, (prow[i] + cb + (n0 + c) * 16) | (c < wcol_ok ? 0 : (int)0x80000000));
        }
        if (++pf_s >= pf_nst) {   // block-uniform
            pf_s = 0;
            pf_c0 += a.KC;
            if (pf_c0 >= a.Cin) {
                pf_c0 = 0;
                if (CLS) {   // next class, or the first class of the next tile
                    if (++pf_cls >= ncls) pf_cls = 0;
                    pf_q0 = __builtin_amdgcn_readfirstlane(ctab[pf_cls * 4]);
                    pf_nq = __builtin_amdgcn_readfirstlane(ctab[pf_cls * 4 + 1]);
                    pf_nst = (pf_nq + QSP - 1) / QSP;
                }
            }
        }
    };
    auto pf_commit = [&](int buf) __attribute__((always_inline)) {   // 256 * WPF == QSP * COPW: every unit exists
        float* dst = wl + (size_t)buf * QSP * COPW * 4;
#pragma unroll
        for (int i = 0; i < (PIPE ? WPF : 1); ++i) *(float4*)(dst + (size_t)(tid + i * 256) * 4) = wv[i];
    };
    if (PIPE) {   // stage 0 is requested here: its latency runs under the per-lane set-up below
        if (CLS) {
            pf_q0 = __builtin_amdgcn_readfirstlane(ctab[0]);
            pf_nq = __builtin_amdgcn_readfirstlane(ctab[1]);
            pf_nst = (pf_nq + QSP - 1) / QSP;
        }
        pf_lookup();
        pf_issue();
    }

    const int nchunks = a.Cin / a.KC;
    float s1[MT][4], s2[MT][4];   // BatchNorm partial sums of this lane's channels over this workgroup's tiles
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[mt][e] = s2[mt][e] = 0.f;
    // PIPE (one workgroup per CU: the AccVGPR half of the register file is free): the statistics partials sit in AccVGPRs while a
    // tile's MFMA sequence runs -- 8*MT ArchVGPRs fewer live across the loop, which is what lets the register allocator keep the two
    // operand sets in place instead of squeezing temporaries into them (copies + early waits: profiles/r2_kbench_ring_trace.txt)
    constexpr bool PARK = PIPE && !CLS;
    float park[PARK ? 8 * MT : 1];
    auto park_stats = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[PARK ? (mt * 4 + e) * 2 : 0]) : "v"(s1[mt][e]));
                asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(park[PARK ? (mt * 4 + e) * 2 + 1 : 0]) : "v"(s2[mt][e]));
            }
    };
    auto unpark_stats = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(s1[mt][e]) : "a"(park[PARK ? (mt * 4 + e) * 2 : 0]));
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(s2[mt][e]) : "a"(park[PARK ? (mt * 4 + e) * 2 + 1 : 0]));
            }
    };
    int run_grp = -1;
    auto flush_stats = [&]() __attribute__((always_inline)) {
        // lanes with the same g hold the same channels for 16 different pixels: fp32 butterfly over them (a lane's partial covers at
        // most a few dozen values), then fp64: the 4 waves through LDS (`patch` is free here: a barrier precedes), one atomic per channel
        double* red = (double*)patch;   // [4 waves][2][COPW]
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = row16_sum(s1[mt][e]), y = row16_sum(s2[mt][e]);
                if (r16 == 0) {
                    red[(wave * 2 + 0) * COPW + mt * 16 + 4 * g + e] = (double)x;
                    red[(wave * 2 + 1) * COPW + mt * 16 + 4 * g + e] = (double)y;
                }
                s1[mt][e] = s2[mt][e] = 0.f;
            }
        __syncthreads();
        if (tid < 2 * COPW && run_grp >= 0) {
            const int which = tid / COPW, c = tid - which * COPW;
            const int co = n0 + c;
            if (co < a.Cout) {
                const double v = (red[(0 * 2 + which) * COPW + c] + red[(1 * 2 + which) * COPW + c]) +
                                 (red[(2 * 2 + which) * COPW + c] + red[(3 * 2 + which) * COPW + c]);
                StatCell* st_ = a.stats + (int64_t)(blockIdx.x % kStatReps) * a.stat_rep_stride;
                fx_add(&st_[((int64_t)run_grp * 2 + which) * a.Cout + co], v);
            }
        }
        __syncthreads();
    };

    int st = 0;
    if (PIPE) {   // stage 0 into buffer 0 (published by the barriers of the first tile), stage 1 into the registers
        pf_commit(0);
        pf_lookup();
        pf_issue();
    } else if (!RES) {
        w_prefetch(0, 0, 0);
    }
    // the resident weights (LDS-DMA) were in flight during the per-lane set-up above; every wave waits for ITS OWN DMA writes here
    // (a barrier does not wait for vector-memory operations), the barriers of the first tile publish them
    if (RES) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp();   // P5: set-up done
    for (int k = 0; k < nwt; ++k) {
        const int4 d0 = *(const int4*)(tdesc + k * 8);       // in_base, iy0, nrows, obase
        const int4 d1 = *(const int4*)(tdesc + k * 8 + 4);   // nimg, grp, p0, img0 | ly0 << 20
        if ((flags & (EPI_STATS | EPI_BNB)) && d1.y != run_grp) {   // block-uniform; the tile range is in ascending group order
            if (run_grp >= 0) flush_stats();
            run_grp = d1.y;
        }
        // this lane's NT output pixels: LDS patch offset of the pixel's origin, output element offset (-1: not a pixel)
        int pbase[NT], ooff[NT];
        if (a.aligned) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const bool v = loc_il[nt] < d1.x;
                pbase[nt] = v ? loc_p[nt] : 0;
                ooff[nt] = v ? d0.w + loc_o[nt] : -1;
            }
        } else {
            const int img0 = d1.w & 0xfffff, ly0 = d1.w >> 20;
            const int grp_end = min(a.N, (d1.y + 1) * a.group_size);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int r = wave * 16 * NT + nt * 16 + r16;
                int pl, lx;
                const int il = mdiv(r, a.m_ppi, a.ppi, pl);
                const int p = d1.z + pl;
                const int n = img0 + il;
                const bool v = (il < a.imgs) & (n < grp_end) & (p < LP);
                const int ly = mdiv(p, a.m_lw, a.LW, lx);
                pbase[nt] = v ? ((il * a.PR + (ly - ly0) * a.is) * a.PC + lx * a.is) * a.CP : 0;
                ooff[nt] = v ? ((n * a.Hout + ly * a.os + a.oy0) * a.Wout + lx * a.os + a.ox0) * a.Cout : -1;
            }
        }
        f32x4 acc[MT][NT];

        // operands of round rho+1 are read from LDS while the MFMAs of round rho issue (two register sets).  What the ring's loop taught
        //  applies here too: the patch-offset table entry of a fetch is read TWO fetches ahead (its wait never falls on
        // reads that have just been issued -- the round-2 loop waited for the entry right behind its ds_read, an exposed LDS round trip
        // per round pair), the operand reads are unconditional (past the last round they fetch registers nobody uses, from addresses
        // inside the weight / patch area) so that a round pair is ONE straight-line body, and sched_barriers keep every read in front
        // of the MFMAs whose register set it does not touch.
        auto rounds = [&](const float* wbase, int q0, int nq) __attribute__((always_inline)) {
            const float* wb = wbase + (size_t)(g * COPW + r16) * 4;
            const int nr = nq >> 2;
            float4 bv[2][NT], av[2][MT];
            int fR = 0;
            int po = qoff[q0 + g], po1 = qoff[q0 + 4 * min(1, nr - 1) + g];
            auto fetch = [&](int set) __attribute__((always_inline)) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bv[set][nt] = *(const float4*)(patch + pbase[nt] + po);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[set][mt] = *(const float4*)(wb + (size_t)fR * 4 * COPW * 4 + mt * 64);
                ++fR;
                po = po1;
                po1 = qoff[q0 + 4 * min(fR + 1, nr - 1) + g];
            };
            auto fma4 = [&](int set) __attribute__((always_inline)) {   // k component outermost: consecutive MFMAs accumulate into different tiles
#define OCL_KSTEP(E)                                                                                                              \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                           \
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[set][mt].E, bv[set][nt].E, acc[mt][nt], 0, 0, 0);
                OCL_KSTEP(x) OCL_KSTEP(y) OCL_KSTEP(z) OCL_KSTEP(w)
#undef OCL_KSTEP
            };
            fetch(0);
            int rho = 0;
            for (; rho + 2 <= nr; rho += 2) {
                fetch(1);
                __builtin_amdgcn_sched_barrier(0);
                fma4(0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(0);
                __builtin_amdgcn_sched_barrier(0);
                fma4(1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (rho < nr) fma4(0);
        };
        // PIPE: the nrs rounds of one (class, chunk) as ONE pipelined sequence over its weight stages (ring buffers xb, xb+1, ...)
        auto seq = [&](int q0, int nrs) __attribute__((always_inline)) {
            constexpr int RPS = QSP / 4;                 // rounds per stage (even)
            const float* wlane = wl + (size_t)(g * COPW + r16) * 4;
            float4 bv[2][NT], av[2][MT];
            int fR = 0, fr = 0, fb = xb;                 // fetch cursor: round of the sequence, round of its stage, ring buffer
            // patch offsets of the next two fetches: a table entry is consumed two fetches (one loop iteration, 2 x 4*MT*NT MFMAs) after it
            // is read, so the wait in front of its address arithmetic never falls on reads that have just been issued
            int po = qoff[q0 + g], po1 = qoff[q0 + 4 * min(1, nrs - 1) + g];
            auto fetch = [&](int set) __attribute__((always_inline)) {
                const float* wb = wlane + (size_t)fb * (QSP * COPW * 4) + fr * (16 * COPW);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bv[set][nt] = *(const float4*)(patch + pbase[nt] + po);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[set][mt] = *(const float4*)(wb + mt * 64);
                ++fR;
                po = po1;
                po1 = qoff[q0 + 4 * min(fR + 1, nrs - 1) + g];
                if (++fr == RPS) { fr = 0; fb = fb == 2 ? 0 : fb + 1; }
            };
            // k component outermost: consecutive MFMAs accumulate into different tiles
            auto fma4 = [&](int set) __attribute__((always_inline)) {
#define OCL_KSTEP(E, F)                                                                                                           \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                           \
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[set][mt].E, bv[set][nt].F, acc[mt][nt], 0, 0, 0);
                OCL_KSTEP(x, x) OCL_KSTEP(y, y) OCL_KSTEP(z, z) OCL_KSTEP(w, w)
#undef OCL_KSTEP
            };
            // (operand reads are unconditional: past the sequence's last round they fetch registers nobody uses, from addresses inside the
            // ring and the patch.  The sched_barriers keep every read where it is written: hoisted into MFMAs that still read the
            // register set it refills, a read gets other registers and a copy -- with an early wait -- behind it.)
            // One wave per SIMD: every instruction that is not an MFMA costs the MFMA stream an issue slot unless it falls into the
            // 32-cycle shadow of an MFMA (about four per gap, cdna guide: issue slots).  The stage's bookkeeping is ~45 instructions
            // (commit, table look-ups) plus ~40 (addresses, loads, cursor): left to the scheduler they form two bursts in front of the
            // first MFMAs of each round (ISA of round 2's build: 45 instructions inside the first k-step of round 0) and the MFMA pipe
            // starves for ~900 cycles per stage (profiles/r3_kbench_conv_220_trace.txt: 44.9 cycles per MFMA against 33.8).  The
            // group barriers below spread them: after every MFMA of the round at most kFill other instructions.
            constexpr int kFillMask = 0x002 | 0x004 | 0x010 | 0x080;   // VALU | SALU | VMEM | DS
            auto spread = [&](int fill) __attribute__((always_inline)) {
#pragma unroll
                for (int i = 0; i < 4 * MT * NT; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (fill == 2) __builtin_amdgcn_sched_group_barrier(kFillMask, 2, 0);
                    else __builtin_amdgcn_sched_group_barrier(kFillMask, 3, 0);
                }
            };
            auto first_pair = [&]() __attribute__((always_inline)) {   // rounds 0, 1 of a stage, with the stage's bookkeeping
                fetch(1);
                pf_commit(xb == 2 ? 0 : xb + 1);
                pf_lookup();
                fma4(0);
                if (OCL_RING_SPREAD) spread(3);
                __builtin_amdgcn_sched_barrier(0);       // the loads (and their table values) stay behind the first round's MFMAs
                fetch(0);
                __builtin_amdgcn_sched_barrier(0);       // operand reads first: they have the whole second round to land
                pf_issue();
                fma4(1);
                if (OCL_RING_SPREAD) spread(2);
                __builtin_amdgcn_sched_barrier(0);       // (the barrier is not hoisted into the MFMAs: its wait would cover the reads above)
                __syncthreads();                         // before the first read of stage t+1 (last round pair of this stage)
            };
            // (a variant with each round's reads split into three pieces between the k-steps of the round before -- at most three LDS
            // instructions per gap -- measured the same: profiles/r2_kbench_ring_v3.txt; the simpler form is kept)
            auto pair = [&]() __attribute__((always_inline)) {
                fetch(1);
                __builtin_amdgcn_sched_barrier(0);
                fma4(0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(0);
                __builtin_amdgcn_sched_barrier(0);
                fma4(1);
                __builtin_amdgcn_sched_barrier(0);
            };
            fetch(0);
            // whole stages: ONE straight-line loop body (RPS rounds), so the two operand sets keep their registers around the back edge
            const int nfull = nrs / RPS;
            for (int t = 0; t < nfull; ++t) {
                first_pair();
#pragma unroll
                for (int p = 1; p < RPS / 2; ++p) pair();
                xb = xb == 2 ? 0 : xb + 1;
            }
            // the class-chunk's last, partial stage (fewer than RPS rounds)
            const int rem = nrs - nfull * RPS;
            if (rem > 0) {
                int R = 0;
                if (rem >= 2) {
                    first_pair();
                    for (R = 2; R + 2 <= rem; R += 2) pair();
                }
                if (R < rem) {   // odd last round
                    if (R == 0) {
                        pf_commit(xb == 2 ? 0 : xb + 1);
                        pf_lookup();
                        fma4(0);
                        __builtin_amdgcn_sched_barrier(0);
                        pf_issue();
                        __syncthreads();
                    } else {
                        fma4(0);
                    }
                }
                xb = xb == 2 ? 0 : xb + 1;
            }
        };

        // output classes (one for an ordinary convolution): with a single channel chunk they share the tile's patch; with several
        // chunks every (class, chunk) stages its own
        if (PARK) park_stats();
        for (int cls = 0; cls < ncls; ++cls) {
        const int4 ct = CLS ? *(const int4*)(ctab + cls * 4) : make_int4(0, a.Qpad, 0, a.nstage);   // first group, groups, output offset, weight stages
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int chunk = 0; chunk < nchunks; ++chunk) {
            const int c0 = chunk * a.KC;
            const bool fresh = (nchunks > 1) | (cls == 0);   // block-uniform
            if (fresh) {
                stamp();   // tile + 0: tile set-up done
                __syncthreads();   // consumers of the previous patch are done
                stamp();   // tile + 1: barrier passed
                store_patch(d0.z, d1.y, c0);
                stamp();   // tile + 2: patch arrived and written to LDS
                if (chunk + 1 < nchunks) load_patch(k, c0 + a.KC);
                else if (nchunks > 1 && cls + 1 < ncls) load_patch(k, 0);
                else if (k + 1 < nwt) load_patch(k + 1, 0);
            }
            if (RES) {
                if (fresh) {
                    __syncthreads();   // patch (and, the first time, the resident weights) visible
                    stamp();   // tile + 3: second barrier passed
                }
                rounds(wl + (size_t)ct.x * COPW * 4, ct.x, ct.y);
                if (fresh) stamp();   // tile + 4: MFMAs issued
            } else if (PIPE) {
                if (fresh) {
                    __syncthreads();   // patch visible (a stage's weights: published by the barrier that follows their commit)
                    stamp();
                }
                seq(ct.x, ct.y >> 2);
                stamp();   // (ring) MFMAs of the class-chunk issued
            } else {
                for (int s_ = 0; s_ < ct.w; ++s_, ++st) {
                    w_commit(st & 1);
                    stamp();   // (staged) weights of the stage arrived and written
                    __syncthreads();   // stage st's weights (and the patch) visible; everyone is done with stage st-1
                    stamp();   // (staged) barrier passed
                    {   // the stage after this one: next stage of the class, next chunk, next class, next tile
                        int ns = s_ + 1, nc0 = c0, ncl = cls, nk = k;
                        if (ns >= ct.w) {
                            ns = 0; nc0 = c0 + a.KC;
                            if (nc0 >= a.Cin) {
                                nc0 = 0; ncl = cls + 1;
                                if (ncl >= ncls) { ncl = 0; nk = k + 1; }
                            }
                        }
                        if (nk < nwt) w_prefetch(ns, nc0, ncl);
                    }
                    const int q0 = ct.x + s_ * a.QS;
                    rounds(wl + (size_t)(st & 1) * a.QS * COPW * 4, q0, min(a.QS, ct.x + ct.y - q0));
                    stamp();   // (staged) MFMAs of the stage issued
                }
            }
        }

        if (PARK) unpark_stats();
        // ---- epilogue from registers: lane (r16 = pixel, g) holds channels n0 + mt*16 + 4g .. +3 of its NT pixels -----------------
        // the two flag sets of a training step (forward: statistics only; plain data gradient: nothing) run without per-store branches
        if (flags == EPI_STATS || flags == 0) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const bool pv_ok = ooff[nt] >= 0;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int co = n0 + mt * 16 + 4 * g;
                    if (pv_ok && co < a.Cout) {
                        const float4 v = make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]);
                        s1[mt][0] += v.x; s1[mt][1] += v.y; s1[mt][2] += v.z; s1[mt][3] += v.w;
                        s2[mt][0] = fmaf(v.x, v.x, s2[mt][0]); s2[mt][1] = fmaf(v.y, v.y, s2[mt][1]);
                        s2[mt][2] = fmaf(v.z, v.z, s2[mt][2]); s2[mt][3] = fmaf(v.w, v.w, s2[mt][3]);
                        *(float4*)(a.out + (int64_t)ooff[nt] + ct.z + co) = v;
                    }
                }
            }
        } else
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bool pv_ok = ooff[nt] >= 0;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int co = n0 + mt * 16 + 4 * g;
                if (!pv_ok || co >= a.Cout) continue;
                float4 v = make_float4(acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]);
                if (flags & EPI_STATS) {
                    s1[mt][0] += v.x; s1[mt][1] += v.y; s1[mt][2] += v.z; s1[mt][3] += v.w;
                    s2[mt][0] = fmaf(v.x, v.x, s2[mt][0]); s2[mt][1] = fmaf(v.y, v.y, s2[mt][1]);
                    s2[mt][2] = fmaf(v.z, v.z, s2[mt][2]); s2[mt][3] = fmaf(v.w, v.w, s2[mt][3]);
                }
                float* op = a.out + (int64_t)ooff[nt] + ct.z + co;
                if (flags & EPI_AFFINE) {
                    const float4 sc = *(const float4*)(a.scale + co), sh = *(const float4*)(a.shift + co);
                    v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
                }
                if (flags & EPI_RES) {
                    const float4 r = *(const float4*)(a.res + (int64_t)ooff[nt] + ct.z + co);
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                if (flags & EPI_RESMASK) {
                    const float4 r = *(const float4*)(a.res + (int64_t)ooff[nt] + ct.z + co);
                    const float4 m = *(const float4*)(a.resmask + (int64_t)ooff[nt] + ct.z + co);
                    v.x += m.x > 0.f ? r.x : 0.f; v.y += m.y > 0.f ? r.y : 0.f; v.z += m.z > 0.f ? r.z : 0.f; v.w += m.w > 0.f ? r.w : 0.f;
                }
                if (flags & EPI_ACCUM) {
                    const float4 o = *(const float4*)op;
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                }
                if (BNB && (flags & EPI_BNB)) {   // ReLU mask + the two batch sums of the BatchNorm this gradient enters (ConvArgs::bnb_*)
                    const int64_t eo = (int64_t)ooff[nt] + ct.z + co;
                    const float* t = bnt + (size_t)(d1.y * (a.Cout >> 2) + (co >> 2)) * 12;
                    bnb_apply(a, *(const float4*)t, *(const float4*)(t + 4), *(const float4*)(t + 8), eo, v, s1[mt], s2[mt]);
                }
                if (flags & EPI_RELU) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                *(float4*)op = v;
            }
        }
        }   // classes
        stamp();   // tile + 5: epilogue issued
    }
    if ((flags & (EPI_STATS | EPI_BNB)) && run_grp >= 0) flush_stats();
    stamp();
}

// the (MT, NT) tilings convt_plain_fn / convt_bnb_fn instantiate
#define OCL_CONVT_TILINGS(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(5, 2)

}  // namespace ocl
