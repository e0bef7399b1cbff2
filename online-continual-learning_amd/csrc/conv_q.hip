// conv_q_kernel (<= 20 output channels on the 4x4x1 MFMA) and its selectors; planner (plan_conv_q) and launch in conv.hip.
#include "conv_stats_dev.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <cmath>

namespace ocl {

// =====================================================================================================
// conv_q_kernel: the convolutions with at most 20 output channels (stem, layer 1, their data gradients) on v_mfma_f32_4x4x1_16b_f32
// =====================================================================================================
// A 16x16x4 tile pads 20 output channels to 32 and 45 (tap, channel-quad) groups to 48: 41 % of the MFMAs issued by conv_t_kernel on
// layer 1 multiply zeros, and layer 1 is the largest single item of a replay step (8 launches, 28 % of the convolution time).  The
// 4x4x1 form is sixteen independent 4x4 outer products per instruction at the same MACs per cycle (profiles/r3_mfma_4x4x1_calibration.txt:
// 10.5 - 12 cycles against 8 ideal with this kernel's operand traffic):
//   block b = 4 consecutive pixels of the wave's 64-pixel set;  B: lane L supplies ITS pixel's input value x[pixel L][k];
//   A: lane L supplies w[channel 4m + (L & 3)][k] (every block multiplies the same four channels);  D: register i of lane L is
//   output channel 4m + i of pixel L.
// So a lane owns one pixel per set and, per block m of four channels, the same "4 consecutive channels of one pixel" accumulator
// layout as conv_t_kernel: the register epilogue carries over.  Nothing is padded: K runs over the 45 groups themselves (one group =
// one 16-byte read of the lane's pixel + 5 broadcast reads of the weights' k-quads for 4 * 5 * NTQ MFMAs), channels over 5 blocks.
// The operand traffic per MFMA is what limits the form (the weights are re-read per 64-pixel set), hence NTQ >= 2 sets per wave and one
// workgroups per CU kept at two by LDS and registers.  Weights are always resident (<= 14.4 KB); tables, patch staging, input transform and epilogue flags as in
// conv_t_kernel.
// TRACE = 1 (measurement build, launched when ConvArgs::trace is set: kbench KBENCH_TRACE): s_memtime stamps of thread 0 -- start |
// tables + weight DMA + first patch landed | per tile: passed barrier 1, patch stored + next patch requested + passed barrier 2, K loop
// done, epilogue done | statistics flushed.
template <int NTQ, int PF, int STATS, int TRACE = 0>   // STATS 0: no sums; 1: forward batch statistics (EPI_STATS); 2: BatchNorm-backward sums (EPI_BNB)
__global__ void __launch_bounds__(256, 2) conv_q_kernel(const ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int MB = kQBlocks, COPW = 4 * MB;
    int* tdesc = (int*)lds_raw;
    int* ctab = tdesc + kMaxWgTiles * 8;
    int* qoff = ctab + 16;
    int* qrow = qoff + a.Qpad;
    float* wl = (float*)(qrow + a.Qpad);                  // [Qpad][COPW][4]
    float* patch = wl + (size_t)a.Qpad * COPW * 4;
    float* xft = patch + a.patch_floats;
    const float* bnt = xft + (a.bnb_lds > 0 ? a.bnb_lds : 0);   // EPI_BNB table (see conv_t_kernel)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int LP = a.LH * a.LW;
    const int ntiles_all = a.groups * a.tiles_per_group;
    const int t_begin = (int)(((int64_t)blockIdx.x * ntiles_all) / gridDim.x), t_end = (int)(((int64_t)(blockIdx.x + 1) * ntiles_all) / gridDim.x);
    const int nwt = t_end - t_begin;
    if (nwt <= 0) return;
    int tr_n = 0;
    auto stamp = [&]() __attribute__((always_inline)) {
        if constexpr (TRACE) {
            if (tid == 0 && tr_n < 64) a.trace[(size_t)blockIdx.x * 64 + tr_n++] = __builtin_amdgcn_s_memtime();
        }
    };
    stamp();
    const int flags = STATS == 1 ? (a.flags & ~EPI_BNB) : STATS == 2 ? (a.flags & ~EPI_STATS) : (a.flags & ~(EPI_STATS | EPI_BNB));   // (instantiated without the statistics: no partial sums in registers)
    // ---- plan tables (conv_plan_tables) ----------------------------------------------------------------------------------------
    const int* __restrict__ blob = a.blob;
    // Register budget (two workgroups per CU: 256 registers, accumulators in ArchVGPRs so that the K loop carries no accvgpr copies
    // across its back edge): of the per-thread patch units only the LDS offset and the row word stay resident; the global offsets are
    // re-read from the plan tables whenever a patch is requested (12 coalesced loads from L2, a whole tile of MFMAs ahead of their use).
    int pu_lds[PF], pu_rp[PF];
    const int* pu_tab = blob + a.off_pu + tid;
    {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            pu_lds[i] = pu_tab[(3 * i + 1) * 256];
            pu_rp[i] = pu_tab[(3 * i + 2) * 256];
        }
    }
    int loc_p[NTQ], loc_o[NTQ], loc_il[NTQ];
    {
        const int* lc = blob + a.off_loc + tid;
#pragma unroll
        for (int nt = 0; nt < NTQ; ++nt) {
            loc_p[nt] = lc[(3 * nt + 0) * 256];
            loc_o[nt] = lc[(3 * nt + 1) * 256];
            loc_il[nt] = lc[(3 * nt + 2) * 256];
        }
    }
    const int4 tile0 = *(const int4*)(blob + a.off_tdesc + (size_t)t_begin * 8);
    const int ntab = 16 + 2 * a.Qpad, ntd = nwt * 8;
    const int* td = blob + a.off_tdesc + (size_t)t_begin * 8;
    const int tab0 = tid < ntab ? blob[tid] : 0, tab1 = tid + 256 < ntab ? blob[tid + 256] : 0;
    const int td0 = tid < ntd ? td[tid] : 0, td1 = tid + 256 < ntd ? td[tid + 256] : 0;
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(a.in), rs_w = make_rsrc(a.wT);
    float4 pv[PF];
    unsigned okm = 0;
    auto load_patch_d = [&](const int4 d) __attribute__((always_inline)) {
        okm = 0;
        int goff[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) goff[i] = pu_tab[(3 * i + 0) * 256];
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int row = pu_rp[i] & 0xffff, pr = (pu_rp[i] >> 16) & 0xff;
            const bool ok = (row < d.z) & ((unsigned)(d.y + pr) < (unsigned)a.Hin) & (goff[i] >= 0);
            pv[i] = buf_load16(rs_in, ok ? d.x + goff[i] : kOob);
            okm |= ok ? (1u << i) : 0u;
        }
    };
    auto store_patch = [&](int nrows, int grp) __attribute__((always_inline)) {
        const float* tb = xft + (size_t)(grp * a.C4tot) * 8;
#pragma unroll
        for (int i = 0; i < PF; ++i)
            if ((pu_rp[i] & 0xffff) < nrows) {
                float4 v = pv[i];
                if (a.xf) {   // block-uniform (ConvArgs::xf)
                    const float* t = tb + (pu_rp[i] >> 24) * 8;
                    const float4 sc = *(const float4*)t, sh = *(const float4*)(t + 4);
                    v.x = fmaxf(__fmaf_rn(v.x, sc.x, sh.x), 0.f); v.y = fmaxf(__fmaf_rn(v.y, sc.y, sh.y), 0.f);
                    v.z = fmaxf(__fmaf_rn(v.z, sc.z, sh.z), 0.f); v.w = fmaxf(__fmaf_rn(v.w, sc.w, sh.w), 0.f);
                    if (!((okm >> i) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                *(float4*)(patch + pu_lds[i]) = v;
            }
    };
    load_patch_d(tile0);
    if (a.xf) {
        const int C = a.Cin;
        const double M = (double)a.xf_m_per_group;
        const bool lead = blockIdx.x == 0;
        for (int j = tid; j < a.groups * C; j += 256) {
            const int gq = j / C, c = j - gq * C;
            double mean, var;
            bn_batch_moments(a.xf_stats, a.xf_rep_stride, gq, c, C, M, mean, var);
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
    if (STATS == 2 && (flags & EPI_BNB)) bnb_table(a, const_cast<float*>(bnt), tid, 256);
    if (tid < ntab) ctab[tid] = tab0;
    if (tid + 256 < ntab) ctab[tid + 256] = tab1;
    if (tid < ntd) tdesc[tid] = td0;
    if (tid + 256 < ntd) tdesc[tid + 256] = td1;
    __syncthreads();
    {   // resident weights: global -> LDS without registers, as conv_t_kernel (pack rows [tap * C4tot + c4][WPT][4], columns < Cout <= WPT)
        const int units = a.Qpad * COPW;
#pragma unroll 4
        for (int u0 = wave * 64; u0 < units; u0 += 256) {
            const int u = u0 + lane;
            const int q = min(u, units - 1) / COPW, c = min(u, units - 1) - q * COPW;
            const int row = qrow[q];
            const int off = (u < units && row >= 0 && c < a.WPT) ? ((row * a.WPT + c) * 4) * 4 : kOob;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(wl + (size_t)u0 * 4), 16, off, 0, 0, 0);
        }
    }
    // BatchNorm statistics without partial sums in registers (they would cost 40 registers across the K loop and, with them, the second
    // workgroup per CU): after every tile a wave reduces its 2 * 20 values over its 64 pixels -- DPP over the 16-lane rows, the four
    // row sums through a wave-private LDS slot -- and adds them to its own accumulator slot in a fixed order (deterministic); the
    // flush sums the four waves' slots in fp64 and issues one atomic per channel, as conv_t_kernel does.
    float* qrows = (float*)(lds_raw + a.qstat_off);   // [4 waves][4 rows][2 * COPW]
    float* qacc = qrows + 4 * 4 * 2 * COPW;            // [4 waves][2 * COPW]
    if (STATS && tid < 4 * 2 * COPW) qacc[tid] = 0.f;
    int run_grp = -1;
    auto flush_stats = [&]() __attribute__((always_inline)) {
        __syncthreads();
        if (STATS && tid < 2 * COPW && run_grp >= 0) {
            const int which = tid / COPW, c = tid - which * COPW;
            if (c < a.Cout) {
                const double v = ((double)qacc[0 * 2 * COPW + tid] + (double)qacc[1 * 2 * COPW + tid]) +
                                 ((double)qacc[2 * 2 * COPW + tid] + (double)qacc[3 * 2 * COPW + tid]);
                StatCell* st_ = a.stats + (int64_t)(blockIdx.x % kStatReps) * a.stat_rep_stride;
                fx_add(&st_[((int64_t)run_grp * 2 + which) * a.Cout + c], v);
            }
        }
        __syncthreads();
        if (STATS && tid < 4 * 2 * COPW) qacc[tid] = 0.f;
        __syncthreads();
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own weight DMA (and the first patch) landed; the tile loop's barriers publish
    stamp();
    const float* wlane = wl + (size_t)(lane & 3) * 4;
    for (int k = 0; k < nwt; ++k) {
        const int4 d0 = *(const int4*)(tdesc + k * 8);
        const int4 d1 = *(const int4*)(tdesc + k * 8 + 4);
        if ((flags & (EPI_STATS | EPI_BNB)) && d1.y != run_grp) {
            if (run_grp >= 0) flush_stats();
            run_grp = d1.y;
        }
        int pbase[NTQ], ooff[NTQ];
        if (a.aligned) {
#pragma unroll
            for (int nt = 0; nt < NTQ; ++nt) {
                const bool v = loc_il[nt] < d1.x;
                pbase[nt] = v ? loc_p[nt] : 0;
                ooff[nt] = v ? d0.w + loc_o[nt] : -1;
            }
        } else {
            const int img0 = d1.w & 0xfffff, ly0 = d1.w >> 20;
            const int grp_end = min(a.N, (d1.y + 1) * a.group_size);
#pragma unroll
            for (int nt = 0; nt < NTQ; ++nt) {
                const int r = wave * 64 * NTQ + nt * 64 + lane;
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
        f32x4 acc[MB][NTQ];
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int nt = 0; nt < NTQ; ++nt) acc[m][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        __syncthreads();   // consumers of the previous patch are done
        stamp();
        store_patch(d0.z, d1.y);
        if (k + 1 < nwt) load_patch_d(*(const int4*)(tdesc + (k + 1) * 8));
        __syncthreads();   // patch (and, the first time, the weights and the transform table) visible
        stamp();
        {   // K loop: one (tap, channel quad) group per step, operands of group q + 1 read while the MFMAs of group q issue
            const int nq = a.Qc;
            float4 bv[2][NTQ], av[2][MB];
            int fq = 0;
            int po = qoff[0], po1 = qoff[min(1, nq - 1)];
            auto fetch = [&](int set) __attribute__((always_inline)) {
#pragma unroll
                for (int nt = 0; nt < NTQ; ++nt) bv[set][nt] = *(const float4*)(patch + pbase[nt] + po);
#pragma unroll
                for (int m = 0; m < MB; ++m) av[set][m] = *(const float4*)(wlane + (size_t)(fq * COPW + 4 * m) * 4);
                ++fq;
                po = po1;
                po1 = qoff[min(fq + 1, nq - 1)];
            };
            auto fma = [&](int set) __attribute__((always_inline)) {
#define OCL_QSTEP(E)                                                                                                      \
    _Pragma("unroll") for (int m = 0; m < MB; ++m) _Pragma("unroll") for (int nt = 0; nt < NTQ; ++nt)                     \
        acc[m][nt] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[set][m].E, bv[set][nt].E, acc[m][nt], 0, 0, 0);
                OCL_QSTEP(x) OCL_QSTEP(y) OCL_QSTEP(z) OCL_QSTEP(w)
#undef OCL_QSTEP
            };
            fetch(0);
            int q = 0;
            for (; q + 2 <= nq; q += 2) {
                fetch(1);
                __builtin_amdgcn_sched_barrier(0);
                fma(0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(0);
                __builtin_amdgcn_sched_barrier(0);
                fma(1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (q < nq) fma(0);
        }
        stamp();
        if (STATS == 1 && (flags & EPI_STATS)) {   // this tile's sums over the wave's pixels -> the wave's accumulator slot
            float* rw = qrows + (size_t)(wave * 4 + (lane >> 4)) * 2 * COPW;
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t1 = 0.f, t2 = 0.f;
#pragma unroll
                    for (int nt = 0; nt < NTQ; ++nt) {
                        const float v = ooff[nt] >= 0 ? acc[m][nt][e] : 0.f;
                        t1 += v;
                        t2 = fmaf(v, v, t2);
                    }
                    t1 = row16_sum(t1);
                    t2 = row16_sum(t2);
                    if ((lane & 15) == 0) {
                        rw[m * 4 + e] = t1;
                        rw[COPW + m * 4 + e] = t2;
                    }
                }
            if (lane < 2 * COPW) {   // (same wave: the writes above are ordered before these reads)
                const float* r0 = qrows + (size_t)(wave * 4) * 2 * COPW + lane;
                qacc[wave * 2 * COPW + lane] += (r0[0] + r0[2 * COPW]) + (r0[4 * COPW] + r0[6 * COPW]);
            }
        }
        // ---- epilogue from registers: the lane holds channels 4m .. 4m + 3 of its NTQ pixels ---------------------------------------
        // one (pixel set, channel block) of the tile: the flag-driven register epilogue
        auto epi_one = [&](int nt, int m, float (&b1)[4], float (&b2)[4]) __attribute__((always_inline)) {
            const int co = 4 * m;
            if (ooff[nt] < 0 || co >= a.Cout) return;
            float4 v = make_float4(acc[m][nt][0], acc[m][nt][1], acc[m][nt][2], acc[m][nt][3]);
            float* op = a.out + (int64_t)ooff[nt] + co;
            if (flags & EPI_AFFINE) {
                const float4 sc = *(const float4*)(a.scale + co), sh = *(const float4*)(a.shift + co);
                v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
            }
            if (flags & EPI_RES) {
                const float4 r = *(const float4*)(a.res + (int64_t)ooff[nt] + co);
                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            if (flags & EPI_RESMASK) {
                const float4 r = *(const float4*)(a.res + (int64_t)ooff[nt] + co);
                const float4 mk = *(const float4*)(a.resmask + (int64_t)ooff[nt] + co);
                v.x += mk.x > 0.f ? r.x : 0.f; v.y += mk.y > 0.f ? r.y : 0.f; v.z += mk.z > 0.f ? r.z : 0.f; v.w += mk.w > 0.f ? r.w : 0.f;
            }
            if (flags & EPI_ACCUM) {
                const float4 o = *(const float4*)op;
                v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
            }
            if (STATS == 2 && (flags & EPI_BNB)) {
                const float* t = bnt + (size_t)(d1.y * (a.Cout >> 2) + m) * 12;
                bnb_apply(a, *(const float4*)t, *(const float4*)(t + 4), *(const float4*)(t + 8), (int64_t)ooff[nt] + co, v, b1, b2);
            }
            if (flags & EPI_RELU) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
            *(float4*)op = v;
        };
        if (STATS == 2 && (flags & EPI_BNB)) {
            // channel block by channel block (8 sum registers at a time): the block's sums over the wave's pixels -> the wave's
            // accumulator slot, as the forward's statistics
            float* rw = qrows + (size_t)(wave * 4 + (lane >> 4)) * 2 * COPW;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                float b1[4] = {0.f, 0.f, 0.f, 0.f}, b2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int nt = 0; nt < NTQ; ++nt) epi_one(nt, m, b1, b2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float r1 = row16_sum(b1[e]), r2 = row16_sum(b2[e]);
                    if ((lane & 15) == 0) {
                        rw[m * 4 + e] = r1;
                        rw[COPW + m * 4 + e] = r2;
                    }
                }
            }
            if (lane < 2 * COPW) {   // (same wave: the writes above are ordered before these reads)
                const float* r0 = qrows + (size_t)(wave * 4) * 2 * COPW + lane;
                qacc[wave * 2 * COPW + lane] += (r0[0] + r0[2 * COPW]) + (r0[4 * COPW] + r0[6 * COPW]);
            }
        } else {
            float nb1[4], nb2[4];   // (unused)
#pragma unroll
            for (int nt = 0; nt < NTQ; ++nt)
#pragma unroll
                for (int m = 0; m < MB; ++m) epi_one(nt, m, nb1, nb2);
        }
        stamp();
    }
    if ((flags & (EPI_STATS | EPI_BNB)) && run_grp >= 0) flush_stats();
    stamp();
}

conv_fn_t convq_trace_fn(int ntq, int pf, int stats) {   // measurement builds: the 220-view plans of layer 1
    if (ntq != 2 || pf != 12) return nullptr;
    return stats == 2 ? conv_q_kernel<2, 12, 2, 1> : stats == 1 ? conv_q_kernel<2, 12, 1, 1> : conv_q_kernel<2, 12, 0, 1>;
}
conv_fn_t convq_fn(int ntq, int pf, int stats) {   // stats: 0 none, 1 EPI_STATS, 2 EPI_BNB
#define OCL_CASE(N, P)                                                                                                         \
    if (ntq == N && pf == P) return stats == 2 ? conv_q_kernel<N, P, 2> : stats == 1 ? conv_q_kernel<N, P, 1> : conv_q_kernel<N, P, 0>;
    OCL_CASE(2, 4) OCL_CASE(2, 12) OCL_CASE(1, 12)
#undef OCL_CASE
    return nullptr;
}

}  // namespace ocl
