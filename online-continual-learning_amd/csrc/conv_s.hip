// conv_s_kernel (few output pixels behind a deep K) and its selector; planner (plan_conv_s) and launch in conv.hip.
#include "conv_stats_dev.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <cmath>

namespace ocl {

// =====================================================================================================
// conv_s_kernel: few output pixels behind a deep K (layer 4 at every batch size, layer 3 below ~200 images)
// =====================================================================================================
// A 20-image pass has 320 output pixels on layer 4 and 1280 on layer 3: five / twenty 64-pixel tiles.  conv_t_kernel gives every
// wave 16 of a tile's pixels and the WHOLE K dimension -- 360 dependent-chain MFMAs per wave on layer 4, on 20 - 60 workgroups of
// the 256 CUs: 14 - 20 us for 0.15 GFLOP (profiles/r3_aser_kernel_stats_v2_single_stream.csv: 25 such launches per ASER step).
// Here a workgroup owns 16 NT pixels x 16 channels and its four waves split K by INPUT CHANNELS (wave w: channels [w, w + 1) * Cin / 4,
// all taps): 4x the workgroups, a quarter of the chain; each wave stages its own channel slice of the (shared-halo) patch, takes its
// weights straight from the pack in global memory / L2 into registers (16 bytes per lane and round, one loop body of four rounds
// ahead: nothing about them is shared between waves, so LDS would only add a copy), and the four partial tiles meet in LDS, where
// wave j adds those of pixel tile j in a fixed order and runs the usual register epilogue.  Tables, input transform and epilogue flags
// as in conv_t_kernel.  NT = 16-pixel tiles per workgroup: at NT = 2 every weight quad and every table entry feeds two MFMAs, for
// twice the patch per wave -- it pays on layer 3's 8x8 lattices from ~100 images on and on the 84x84 input's lattices, not on
// layer 4's 4x4 images (profiles/r3_conv_s_ab.md, which also has the per-wave phase traces and the counter passes).
// The kernel must stay free of scratch: a build with 10 spilled VGPRs was 1 - 4 us per launch slower than the one before it.
template <int NT, bool TRACE, bool BNB = false, bool DET = false>   // BNB: instantiated with the EPI_BNB epilogue; DET: for the deterministic batch sums
__global__ void __launch_bounds__(256, NT == 1 ? 5 : 4) conv_s_kernel(const ConvArgs a) {
    constexpr int FXM = DET ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int* ctab = (int*)lds_raw;
    int* qoff = ctab + 16;                           // [4][Qpad / 4] patch offset of group q = 4 rho + g, stored [g][rho] (one wave's channel slice)
    int* qrow = qoff + a.Qpad;                       // [4][Qpad / 4 + 4] pack row of group q relative to the slice's first channel quad, same order; each row ends in four -1 ("no load")
    float* patch0 = (float*)(qrow + a.Qpad + 16);    // [4 waves][patch_floats]; after the K loop each wave's slice holds its partial tiles [NT][64 lanes][4]
    float* xft = patch0 + (size_t)4 * a.patch_floats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.y * 16;
    const int flags = BNB ? a.flags : (a.flags & ~EPI_BNB);
    const int* __restrict__ blob = a.blob;
    const int tile = blockIdx.x;
    const int c0 = wave * a.KC;                      // this wave's channel slice
    float* patch = patch0 + (size_t)wave * a.patch_floats;
    // (TRACE, a measurement build launched when ConvArgs::trace is set: s_memtime stamps of lane 0 of every wave, 8 slots per wave -- kbench KBENCH_TRACE)
    unsigned long long* trp = TRACE ? a.trace + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 64 + wave * 8 : nullptr;
    auto stamp = [&](int i) __attribute__((always_inline)) { if (TRACE && lane == 0) trp[i] = __builtin_amdgcn_s_memtime(); };
    stamp(0);
    const int4 d0 = *(const int4*)(blob + a.off_tdesc + (size_t)tile * 8);       // in_base, iy0, nrows, obase
    const int4 d1 = *(const int4*)(blob + a.off_tdesc + (size_t)tile * 8 + 4);   // nimg, grp, p0, img0 | ly0 << 20
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(a.in), rs_w = make_rsrc(a.wT);
    const int c4base = c0 >> 2;
    // ---- the lane's patch units (64-lane walk), kPFS per staging pass: table entries -> loads -> (transform) -> the wave's LDS slice ------
    int pu_lds[kPFS], pu_rp[kPFS];
    float4 pv[kPFS];
    unsigned okm = 0;
    auto stage_load = [&](int pass) __attribute__((always_inline)) {
        const int* pu = blob + a.off_pu + pass * (3 * kPFS * 256) + lane;
        okm = 0;
#pragma unroll
        for (int i = 0; i < kPFS; ++i) {
            const int goff = pu[(3 * i + 0) * 256];
            pu_lds[i] = pu[(3 * i + 1) * 256];
            pu_rp[i] = pu[(3 * i + 2) * 256];
            const int row = pu_rp[i] & 0xffff, pr = (pu_rp[i] >> 16) & 0xff;
            const bool ok = (row < d0.z) & ((unsigned)(d0.y + pr) < (unsigned)a.Hin) & (goff >= 0);
            pv[i] = buf_load16(rs_in, ok ? d0.x + c0 * 4 + goff : kOob);
            okm |= ok ? (1u << i) : 0u;
        }
    };
    auto stage_store = [&]() __attribute__((always_inline)) {
        const float* tb = xft + (size_t)(d1.y * a.C4tot + c4base) * 8;
#pragma unroll
        for (int i = 0; i < kPFS; ++i)
            if ((pu_rp[i] & 0xffff) < d0.z) {
                float4 v = pv[i];
                if (a.xf) {
                    const float* t = tb + (pu_rp[i] >> 24) * 8;
                    const float4 sc = *(const float4*)t, sh = *(const float4*)(t + 4);
                    v.x = fmaxf(__fmaf_rn(v.x, sc.x, sh.x), 0.f); v.y = fmaxf(__fmaf_rn(v.y, sc.y, sh.y), 0.f);
                    v.z = fmaxf(__fmaf_rn(v.z, sc.z, sh.z), 0.f); v.w = fmaxf(__fmaf_rn(v.w, sc.w, sh.w), 0.f);
                    if (!((okm >> i) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                *(float4*)(patch + pu_lds[i]) = v;
            }
    };
    stage_load(0);
    // ---- the lane's output pixels, the group tables ------------------------------------------------------------------------------------------
    int loc_p[NT], loc_o[NT], loc_il[NT];
    {
        const int* lc = blob + a.off_loc + r16;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            loc_p[nt] = lc[(3 * nt + 0) * 256];
            loc_o[nt] = lc[(3 * nt + 1) * 256];
            loc_il[nt] = lc[(3 * nt + 2) * 256];
        }
    }
    const int ntab = 16 + 2 * a.Qpad;
    const int tab0 = tid < ntab ? blob[tid] : 0, tab1 = tid + 256 < ntab ? blob[tid + 256] : 0;
    if (a.xf) {
        const int C = a.Cin;
        const double M = (double)a.xf_m_per_group;
        const bool lead = blockIdx.x == 0 && blockIdx.y == 0;
        // A tile lies inside one BatchNorm group (d1.y) and stage_store reads that group's rows only: the ~2000 workgroups of a layer-4
        // launch each build ONE group's table, two replica loads in flight per thread (every group's with one load in flight was 16
        // dependent L2 round trips per entry and two entries per thread: 6.4 us of a 32 us launch, profiles/r6_convs_xf_prologue_ab.txt);
        // the lead workgroup builds every group's (it saves mean / invstd for the backward).
        const int j_end = lead ? a.groups * C : (d1.y + 1) * C;
        for (int j = (lead ? 0 : d1.y * C) + tid; j < j_end; j += 256) {
            const int gq = j / C, c = j - gq * C;
            double mean, var;
            bn_batch_moments<2, FXM>(a.xf_stats, a.xf_rep_stride, gq, c, C, M, mean, var);
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
            bn_running_update<FXM>(a.xf_stats, a.xf_rep_stride, a.groups, C, M, a.xf_momentum, a.xf_running_mean, a.xf_running_var, a.xf_nbt, tid, 256);
    }
    stamp(1);
    const int nr = a.Qpad >> 2;                      // rounds of 4 groups; a multiple of 4 (the planner pads with zero-weight groups)
    {   // the group tables transposed to [g][rho]: a lane fetches four rounds of its g with one 16-byte read
        auto tpos = [&](int t) __attribute__((always_inline)) -> int {
            if (t < 16) return t;
            int e = t - 16, base = 16;
            if (e >= a.Qpad) return 16 + a.Qpad + ((e - a.Qpad) & 3) * (nr + 4) + ((e - a.Qpad) >> 2);
            return base + (e & 3) * nr + (e >> 2);
        };
        if (tid < ntab) ctab[tpos(tid)] = tab0;
        if (tid + 256 < ntab) ctab[tpos(tid + 256)] = tab1;
        if (tid < 16) qrow[(tid >> 2) * (nr + 4) + nr + (tid & 3)] = -1;
    }
    __syncthreads();   // group tables (and the transform table) visible
    stamp(2);
    // ---- weights: round rho of this wave = groups 4 rho + g, one 16-byte load per lane, four rounds (one loop body) ahead -----------------
    const int wcol = n0 + r16;
    const int* qoffT = qoff + g * nr;
    const int* qrowT = qrow + g * (nr + 4);
    const bool wok = wcol < a.WPT;
    const int wbase = (c4base * a.WPT + wcol) * 16, wstride = a.WPT * 16;
    auto w_addr = [&](int row) __attribute__((always_inline)) -> int { return (row >= 0 && wok) ? row * wstride + wbase : kOob; };
    int4 qr = *(const int4*)qrowT;                   // pack rows of rounds 0 .. 3
    float4 aw[kDepthS];
    aw[0] = buf_load16(rs_w, w_addr(qr.x)); aw[1] = buf_load16(rs_w, w_addr(qr.y));
    aw[2] = buf_load16(rs_w, w_addr(qr.z)); aw[3] = buf_load16(rs_w, w_addr(qr.w));
    qr = *(const int4*)(qrowT + 4);                  // rounds 4 .. 7: the loads the first body issues (past the last round: -1, no load)
    int4 qo = *(const int4*)qoffT;                   // patch offsets of rounds 0 .. 3
    // ---- this wave's patch slice (private to the wave: no workgroup barrier, its own LDS writes are ordered before its reads) -------------
    stamp(3);
    stage_store();
    for (int pass = 1; pass < a.nstage; ++pass) {
        stage_load(pass);
        stage_store();
    }
    stamp(4);
    int pbase[NT], ooff[NT];
    if (a.aligned) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const bool pix_ok = loc_il[nt] < d1.x;
            pbase[nt] = pix_ok ? loc_p[nt] : 0;
            ooff[nt] = pix_ok ? d0.w + loc_o[nt] : -1;
        }
    } else {   // tiles that start inside a lattice row (11 x 11, 21 x 21 lattices of the 84 x 84 input): one image per tile
        const int img0 = d1.w & 0xfffff, ly0 = d1.w >> 20;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int p = d1.z + nt * 16 + r16;
            const bool v = p < a.LH * a.LW;
            int lx;
            const int ly = mdiv(p, a.m_lw, a.LW, lx);
            pbase[nt] = v ? (((ly - ly0) * a.is) * a.PC + lx * a.is) * a.CP : 0;
            ooff[nt] = v ? ((img0 * a.Hout + ly * a.os + a.oy0) * a.Wout + lx * a.os + a.ox0) * a.Cout : -1;
        }
    }
    f32x4 acc[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt][0] = acc[nt][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // One body = four rounds, no branches: the B operands of the body and the tables of the next are requested at its top, each
    // weight register is refilled (for the next body) right after it is read, and the MFMAs of two rounds alternate between two
    // accumulators per pixel tile.  With one wave per SIMD (a 20-image pass) the loop ran at 578 cycles per round of 4 MFMAs -- two
    // dependent LDS round trips (table, then operand) and a 4-MFMA chain per round; profiles/r3_conv_s_ab.md.
    for (int rho = 0; rho < nr; rho += 4) {
        float4 bv[NT][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            bv[nt][0] = *(const float4*)(patch + pbase[nt] + qo.x); bv[nt][1] = *(const float4*)(patch + pbase[nt] + qo.y);
            bv[nt][2] = *(const float4*)(patch + pbase[nt] + qo.z); bv[nt][3] = *(const float4*)(patch + pbase[nt] + qo.w);
        }
        const int4 qo_n = *(const int4*)(qoffT + min(rho + 4, nr - 4));
        const int4 qr_n = *(const int4*)(qrowT + min(rho + 8, nr));
        const int qrv[4] = {qr.x, qr.y, qr.z, qr.w};
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
            const float4 a0 = aw[i], a1 = aw[i + 1];
            aw[i] = buf_load16(rs_w, w_addr(qrv[i]));
            aw[i + 1] = buf_load16(rs_w, w_addr(qrv[i + 1]));
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bv[nt][i].x, acc[nt][0], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bv[nt][i + 1].x, acc[nt][1], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bv[nt][i].y, acc[nt][0], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bv[nt][i + 1].y, acc[nt][1], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bv[nt][i].z, acc[nt][0], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, bv[nt][i + 1].z, acc[nt][1], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bv[nt][i].w, acc[nt][0], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, bv[nt][i + 1].w, acc[nt][1], 0, 0, 0);
            }
        }
        qo = qo_n;
        qr = qr_n;
    }
    stamp(5);
    // (the wave's own patch slice is dead once its K loop is done: the partial tiles go there, no extra buffer and no extra barrier)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const f32x4 t = acc[nt][0] + acc[nt][1];
        *(float4*)(patch + (size_t)(nt * 64 + lane) * 4) = make_float4(t[0], t[1], t[2], t[3]);
    }
    __syncthreads();
    stamp(6);
    if (wave >= NT) return;   // wave j adds the four partial tiles of pixel tile j in a fixed order and runs its epilogue
    float4 v;
    {
        const float* rj = patch0 + (size_t)(wave * 64 + lane) * 4;
        const size_t ws = (size_t)a.patch_floats;
        const float4 p0 = *(const float4*)(rj), p1 = *(const float4*)(rj + ws);
        const float4 p2 = *(const float4*)(rj + 2 * ws), p3 = *(const float4*)(rj + 3 * ws);
        v = make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
    }
    // ---- epilogue: lane (r16 = pixel of tile `wave`, g) holds channels n0 + 4g .. + 3 -------------------------------------------------------
    int oo = ooff[0];
#pragma unroll
    for (int nt = 1; nt < NT; ++nt) oo = wave == nt ? ooff[nt] : oo;
    const int co = n0 + 4 * g;
    const bool live = oo >= 0 && co < a.Cout;
    if (flags & EPI_STATS) {   // sums over the tile's pixels (DPP row of 16 lanes), one fp64 atomic per channel
        const float4 z = live ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        const float s1x = row16_sum(z.x), s1y = row16_sum(z.y), s1z = row16_sum(z.z), s1w = row16_sum(z.w);
        const float s2x = row16_sum(z.x * z.x), s2y = row16_sum(z.y * z.y), s2z = row16_sum(z.z * z.z), s2w = row16_sum(z.w * z.w);
        if (r16 < 8 && co < a.Cout) {   // (every lane of the row holds the eight sums: lane j adds sum j -- one accumulation per lane)
            const int j = r16;
            const float v = j == 0 ? s1x : j == 1 ? s1y : j == 2 ? s1z : j == 3 ? s1w : j == 4 ? s2x : j == 5 ? s2y : j == 6 ? s2z : s2w;
            StatCell* st_ = a.stats + (int64_t)((blockIdx.x + blockIdx.y + wave) % kStatReps) * a.stat_rep_stride + ((int64_t)d1.y * 2) * a.Cout + co;
            fx_add<FXM>(st_ + (j >> 2) * a.Cout + (j & 3), (double)v);
        }
    }
    float* op = a.out + (int64_t)oo + co;
    if (live) {
        if (flags & EPI_AFFINE) {
            const float4 sc = *(const float4*)(a.scale + co), sh = *(const float4*)(a.shift + co);
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
        }
        if (flags & EPI_RES) {
            const float4 r = *(const float4*)(a.res + (int64_t)oo + co);
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (flags & EPI_RESMASK) {
            const float4 r = *(const float4*)(a.res + (int64_t)oo + co);
            const float4 mk = *(const float4*)(a.resmask + (int64_t)oo + co);
            v.x += mk.x > 0.f ? r.x : 0.f; v.y += mk.y > 0.f ? r.y : 0.f; v.z += mk.z > 0.f ? r.z : 0.f; v.w += mk.w > 0.f ? r.w : 0.f;
        }
        if (flags & EPI_ACCUM) {
            const float4 o = *(const float4*)op;
            v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
    }
    if (BNB && (flags & EPI_BNB)) {   // ReLU mask + the two batch sums of the BatchNorm this gradient enters; one channel quad per lane: the
                             // BatchNorm's parameters come straight from memory (no table), after the K loop (no registers across it)
        float b1[4] = {0.f, 0.f, 0.f, 0.f}, b2[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const int j = d1.y * a.Cout + co;
            const float4 mu = *(const float4*)(a.bnb_mean + j);
            float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sh = sc;
            if (!a.bnb_z) {
                const float4 is = *(const float4*)(a.bnb_invstd + j), gm = *(const float4*)(a.bnb_gamma + co), bt = *(const float4*)(a.bnb_beta + co);
                bn_scale_shift(gm.x, bt.x, mu.x, is.x, sc.x, sh.x); bn_scale_shift(gm.y, bt.y, mu.y, is.y, sc.y, sh.y);
                bn_scale_shift(gm.z, bt.z, mu.z, is.z, sc.z, sh.z); bn_scale_shift(gm.w, bt.w, mu.w, is.w, sc.w, sh.w);
            }
            bnb_apply(a, sc, sh, mu, (int64_t)oo + co, v, b1, b2);
        }
        const float s1x = row16_sum(b1[0]), s1y = row16_sum(b1[1]), s1z = row16_sum(b1[2]), s1w = row16_sum(b1[3]);
        const float s2x = row16_sum(b2[0]), s2y = row16_sum(b2[1]), s2z = row16_sum(b2[2]), s2w = row16_sum(b2[3]);
        if (r16 < 8 && co < a.Cout) {   // (every lane of the row holds the eight sums: lane j adds sum j -- one accumulation per lane)
            const int j = r16;
            const float v = j == 0 ? s1x : j == 1 ? s1y : j == 2 ? s1z : j == 3 ? s1w : j == 4 ? s2x : j == 5 ? s2y : j == 6 ? s2z : s2w;
            StatCell* st_ = a.stats + (int64_t)((blockIdx.x + blockIdx.y + wave) % kStatReps) * a.stat_rep_stride + ((int64_t)d1.y * 2) * a.Cout + co;
            fx_add<FXM>(st_ + (j >> 2) * a.Cout + (j & 3), (double)v);
        }
    }
    if (!live) return;
    if (flags & EPI_RELU) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    *(float4*)op = v;
    stamp(7);
}

conv_fn_t convs_fn(int nt, bool trace, bool bnb, bool det) {
    if (det) {
        if (bnb) return nt == 2 ? conv_s_kernel<2, false, true, true> : conv_s_kernel<1, false, true, true>;
        return nt == 2 ? conv_s_kernel<2, false, false, true> : conv_s_kernel<1, false, false, true>;
    }
    if (bnb) return nt == 2 ? conv_s_kernel<2, false, true> : conv_s_kernel<1, false, true>;
    if (trace) return nt == 2 ? conv_s_kernel<2, true> : conv_s_kernel<1, true>;
    return nt == 2 ? conv_s_kernel<2, false> : conv_s_kernel<1, false>;
}

}  // namespace ocl
