// bn_*: train-mode BatchNorm forward (normalise + residual + ReLU, running-stat update), eval-mode fold and backward, with their launchers.
//
// Replaces the ATen sequences behind models/resnet.py:32-37 and their autograd.
#include "conv_stats_dev.h"
#include <string.h>
#include <algorithm>
#include <type_traits>
#include <cmath>

namespace ocl {

// =====================================================================================================
// BatchNorm forward (train mode): normalise + optional residual + ReLU; block (0,0) updates running stats
// (nn.BatchNorm2d: biased variance to normalise, unbiased for the running update, momentum 0.1)
// =====================================================================================================
__global__ void __launch_bounds__(256) bn_fwd_kernel(const BnFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sc = sm;
    float* sh = sm + a.C;
    const int g = blockIdx.y, tid = threadIdx.x;
    const double M = (double)a.m_per_group;
    for (int c = tid; c < a.C; c += 256) {
        double mean, var;
        bn_batch_moments(a.stats, a.stat_rep_stride, g, c, a.C, M, mean, var);
        if (a.frozen_mean) {   // eval-mode BatchNorm on the tape: the running statistics, folded exactly as bn_fold_kernel does
            mean = (double)a.frozen_mean[c];
            var = (double)a.frozen_var[c];
        }
        const double invstd = 1.0 / sqrt(var + (double)a.eps);
        bn_scale_shift(a.gamma[c], a.beta[c], (float)mean, (float)invstd, sc[c], sh[c]);
        if (blockIdx.x == 0) {
            a.save_mean[(int64_t)g * a.C + c] = (float)mean;
            a.save_invstd[(int64_t)g * a.C + c] = (float)invstd;
        }
    }
    if (blockIdx.x == 0 && g == 0 && a.running_mean)
        bn_running_update(a.stats, a.stat_rep_stride, a.G, a.C, M, a.momentum, a.running_mean, a.running_var, a.nbt, tid, 256);
    float* scb = sm + 2 * a.C;
    float* shb = sm + 3 * a.C;
    if (a.yb) {   // the projection shortcut's BatchNorm: the same table, statistics and running update from its own arena
        for (int c = tid; c < a.C; c += 256) {
            double mean, var;
            bn_batch_moments(a.stats_b, a.stat_rep_stride, g, c, a.C, M, mean, var);
            if (a.frozen_mean_b) {
                mean = (double)a.frozen_mean_b[c];
                var = (double)a.frozen_var_b[c];
            }
            const double invstd = 1.0 / sqrt(var + (double)a.eps);
            bn_scale_shift(a.gamma_b[c], a.beta_b[c], (float)mean, (float)invstd, scb[c], shb[c]);
            if (blockIdx.x == 0) {
                a.save_mean_b[(int64_t)g * a.C + c] = (float)mean;
                a.save_invstd_b[(int64_t)g * a.C + c] = (float)invstd;
            }
        }
        if (blockIdx.x == 0 && g == 0 && a.running_mean_b)
            bn_running_update(a.stats_b, a.stat_rep_stride, a.G, a.C, M, a.momentum, a.running_mean_b, a.running_var_b, a.nbt_b, tid, 256);
    }
    __syncthreads();
    const int C4 = a.C >> 2;
    const int64_t units = a.m_per_group * C4;
    const float4* y4 = (const float4*)a.y + (int64_t)g * units;
    const float4* b4 = a.yb ? (const float4*)a.yb + (int64_t)g * units : nullptr;
    const float4* r4 = a.res ? (const float4*)a.res + (int64_t)g * units : nullptr;
    float4* z4 = (float4*)a.z + (int64_t)g * units;
    for (int64_t u = (int64_t)blockIdx.x * 256 + tid; u < units; u += (int64_t)gridDim.x * 256) {
        const int c = (int)(u % C4) * 4;
        float4 v = y4[u];
        v.x = __fmaf_rn(v.x, sc[c], sh[c]);
        v.y = __fmaf_rn(v.y, sc[c + 1], sh[c + 1]);
        v.z = __fmaf_rn(v.z, sc[c + 2], sh[c + 2]);
        v.w = __fmaf_rn(v.w, sc[c + 3], sh[c + 3]);
        if (r4) {
            const float4 r = r4[u];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (b4) {
            float4 r = b4[u];
            r.x = __fmaf_rn(r.x, scb[c], shb[c]);
            r.y = __fmaf_rn(r.y, scb[c + 1], shb[c + 1]);
            r.z = __fmaf_rn(r.z, scb[c + 2], shb[c + 2]);
            r.w = __fmaf_rn(r.w, scb[c + 3], shb[c + 3]);
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        if (a.relu) {
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        z4[u] = v;
    }
}

int launch_bn_fwd(const BnFwdArgs& a, hipStream_t s) {
    const int64_t units = a.m_per_group * (a.C / 4);
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (units + 1023) / 1024));
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(bn_fwd_kernel, dim3(bx, a.G), dim3(256), (size_t)a.C * (a.yb ? 16 : 8), s, a);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// z = relu(fma(y, scale, shift)) with scale / shift from SAVED statistics: materialises the activation a fused pass never wrote
__global__ void __launch_bounds__(256) bn_apply_saved_kernel(const float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ z,
                                                             int64_t m_per_group, int C) {
    const int g = blockIdx.y, C4 = C >> 2;
    const int64_t units = m_per_group * C4;
    for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
        const int c = (int)(u % C4) * 4;
        float4 v = ((const float4*)y)[(int64_t)g * units + u];
        float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float sc, sh;
            bn_scale_shift(gamma[c + e], beta[c + e], mean[(int64_t)g * C + c + e], invstd[(int64_t)g * C + c + e], sc, sh);
            o[e] = fmaxf(__fmaf_rn(o[e], sc, sh), 0.f);
        }
        ((float4*)z)[(int64_t)g * units + u] = make_float4(o[0], o[1], o[2], o[3]);
    }
}
int launch_bn_apply_saved(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta, float* z,
                          int64_t m_per_group, int G, int C, hipStream_t s) {
    const int64_t units = m_per_group * (C / 4);
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (units + 1023) / 1024));
    hipLaunchKernelGGL(bn_apply_saved_kernel, dim3(bx, G), dim3(256), 0, s, y, mean, invstd, gamma, beta, z, m_per_group, C);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

__global__ void __launch_bounds__(256) bn_fold_kernel(const float* __restrict__ params, const float* __restrict__ running,
                                                      float* __restrict__ out, const BnFoldDesc* __restrict__ descs, float eps) {
    const BnFoldDesc d = descs[blockIdx.x];
    for (int c = threadIdx.x; c < d.C; c += 256) {
        const float rm = running[d.stat_off + c], rv = running[d.stat_off + d.C + c];
        const float invstd = (float)(1.0 / sqrt((double)rv + (double)eps));
        const float scale = params[d.gamma_off + c] * invstd;
        out[d.out_off + c] = scale;
        out[d.out_off + d.C + c] = params[d.beta_off + c] - rm * scale;
    }
}
int launch_bn_fold(const float* params, const float* running, float* out, const BnFoldDesc* descs_dev, int n_bn, float eps,
                   hipStream_t s) {
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(bn_fold_kernel, dim3(n_bn), dim3(256), 0, s, params, running, out, descs_dev, eps);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// =====================================================================================================
// BatchNorm backward (+ReLU mask), one or two BNs sharing the incoming gradient
// =====================================================================================================
// One block walks a contiguous pixel range: thread t < PT*C4 owns (pixel lane t / C4, channel quad t % C4), so one pass of the block
// reads PT*C4 consecutive float4s of each tensor.  U passes are loaded before any is consumed (3U 16-byte loads in flight per lane).
template <int U>
__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(const BnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int C4 = a.C >> 2;
    const int PT = 256 / C4;  // pixel lanes
    const int tid = threadIdx.x;
    const int c4 = tid % C4, pl = tid / C4;
    const int g = blockIdx.y;
    const int64_t M = a.m_per_group;
    const int64_t per = (M + gridDim.x - 1) / gridDim.x;
    const int64_t pbeg = (int64_t)blockIdx.x * per, pend = min(M, pbeg + per);
    float4 sd[2], sx[2];
    float4 mean[2], istd[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        sd[k] = sx[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        mean[k] = istd[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (pl < PT) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < a.nsets) {
                mean[k] = *(const float4*)(a.mean[k] + (int64_t)g * a.C + c4 * 4);
                istd[k] = *(const float4*)(a.invstd[k] + (int64_t)g * a.C + c4 * 4);
            }
        const float4* dz4 = (const float4*)a.dz + (int64_t)g * M * C4;
        const float4* z4 = a.z ? (const float4*)a.z + (int64_t)g * M * C4 : nullptr;
        const float4* y40 = (const float4*)a.y[0] + (int64_t)g * M * C4;
        const float4* y41 = a.nsets > 1 ? (const float4*)a.y[1] + (int64_t)g * M * C4 : y40;
        const int64_t step = (int64_t)PT * C4;
        const int64_t eend = pend * C4;
        int64_t e = (pbeg + pl) * C4 + c4;
        float4 msc = make_float4(0.f, 0.f, 0.f, 0.f), msh = msc;   // mask_from_y: scale / shift of this thread's channel quad
        if (a.mask_from_y) {
            const float4 gm = *(const float4*)(a.gamma[0] + c4 * 4), bt = *(const float4*)(a.beta[0] + c4 * 4);
            bn_scale_shift(gm.x, bt.x, mean[0].x, istd[0].x, msc.x, msh.x); bn_scale_shift(gm.y, bt.y, mean[0].y, istd[0].y, msc.y, msh.y);
            bn_scale_shift(gm.z, bt.z, mean[0].z, istd[0].z, msc.z, msh.z); bn_scale_shift(gm.w, bt.w, mean[0].w, istd[0].w, msc.w, msh.w);
        }
        auto consume = [&](float4 d, float4 zz, const float4& ya, const float4& yb) __attribute__((always_inline)) {
            if (a.mask_from_y)
                zz = make_float4(__fmaf_rn(ya.x, msc.x, msh.x), __fmaf_rn(ya.y, msc.y, msh.y), __fmaf_rn(ya.z, msc.z, msh.z), __fmaf_rn(ya.w, msc.w, msh.w));
            if (z4 || a.mask_from_y) {
                d.x = zz.x > 0.f ? d.x : 0.f; d.y = zz.y > 0.f ? d.y : 0.f;
                d.z = zz.z > 0.f ? d.z : 0.f; d.w = zz.w > 0.f ? d.w : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (k < a.nsets) {
                    const float4& y = k ? yb : ya;
                    sd[k].x += d.x; sd[k].y += d.y; sd[k].z += d.z; sd[k].w += d.w;
                    sx[k].x = fmaf(d.x, (y.x - mean[k].x) * istd[k].x, sx[k].x);
                    sx[k].y = fmaf(d.y, (y.y - mean[k].y) * istd[k].y, sx[k].y);
                    sx[k].z = fmaf(d.z, (y.z - mean[k].z) * istd[k].z, sx[k].z);
                    sx[k].w = fmaf(d.w, (y.w - mean[k].w) * istd[k].w, sx[k].w);
                }
        };
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (; e + (U - 1) * step < eend; e += U * step) {
            float4 d[U], zz[U], ya[U], yb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                d[u] = dz4[e + u * step];
                zz[u] = z4 ? z4[e + u * step] : zero4;
                ya[u] = y40[e + u * step];
                yb[u] = a.nsets > 1 ? y41[e + u * step] : zero4;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) consume(d[u], zz[u], ya[u], yb[u]);
        }
        for (; e < eend; e += step)
            consume(dz4[e], z4 ? z4[e] : zero4, y40[e], a.nsets > 1 ? y41[e] : zero4);
    }
    // LDS layout: [set][2][PT][C]
    float* base = sm;
    if (pl < PT) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < a.nsets) {
                *(float4*)(base + ((size_t)(k * 2 + 0) * PT + pl) * a.C + c4 * 4) = sd[k];
                *(float4*)(base + ((size_t)(k * 2 + 1) * PT + pl) * a.C + c4 * 4) = sx[k];
            }
    }
    __syncthreads();
    for (int j = tid; j < a.nsets * 2 * a.C; j += 256) {
        const int c = j % a.C, kk = j / a.C;  // kk = set*2 + which
        double t = 0.0;
        for (int r = 0; r < PT; ++r) t += (double)base[((size_t)kk * PT + r) * a.C + c];
        const int k = kk >> 1, which = kk & 1;
        fx_add(&a.sums[(((int64_t)k * a.G + g) * 2 + which) * a.C + c], t);
    }
}

__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const BnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    // per set: k1[C] (mean dpre), k2[C] (mean dpre*xhat), scale[C], mean[C], invstd[C]
    const int g = blockIdx.y, tid = threadIdx.x;
    const double Md = (double)a.m_per_group;
    for (int j = tid; j < a.nsets * a.C; j += 256) {
        const int c = j % a.C, k = j / a.C;
        const StatCell cdy = a.sums[(((int64_t)k * a.G + g) * 2 + 0) * a.C + c], cdx = a.sums[(((int64_t)k * a.G + g) * 2 + 1) * a.C + c];
        const double sdy = fx_decode(cdy.hi, cdy.lo), sdx = fx_decode(cdx.hi, cdx.lo);
        float* s = sm + (size_t)k * 6 * a.C;
        const float istd = a.invstd[k][(int64_t)g * a.C + c];
        s[c] = a.frozen ? 0.f : (float)(sdy / Md);
        s[a.C + c] = a.frozen ? 0.f : (float)(sdx / Md);
        s[2 * a.C + c] = a.gamma[k][c] * istd;
        s[3 * a.C + c] = a.mean[k][(int64_t)g * a.C + c];
        s[4 * a.C + c] = istd;
        if (a.mask_from_y) {
            float sc_, sh_;
            bn_scale_shift(a.gamma[k][c], a.beta[k][c], a.mean[k][(int64_t)g * a.C + c], istd, sc_, sh_);
            s[5 * a.C + c] = sh_;   // (scale: s[2C + c] = gamma * invstd, the same product)
        }
        if (blockIdx.x == 0 && g == 0) {
            double dg = 0.0, db = 0.0;
            for (int gg = 0; gg < a.G; ++gg) {
                const StatCell cb = a.sums[(((int64_t)k * a.G + gg) * 2 + 0) * a.C + c], cg = a.sums[(((int64_t)k * a.G + gg) * 2 + 1) * a.C + c];
                db += fx_decode(cb.hi, cb.lo);
                dg += fx_decode(cg.hi, cg.lo);
            }
            if (a.accumulate) {
                a.dgamma[k][c] += (float)dg;
                a.dbeta[k][c] += (float)db;
            } else {
                a.dgamma[k][c] = (float)dg;
                a.dbeta[k][c] = (float)db;
            }
        }
    }
    __syncthreads();
    const int C4 = a.C >> 2;
    const int64_t units = a.m_per_group * C4;
    for (int64_t u = (int64_t)blockIdx.x * 256 + tid; u < units; u += (int64_t)gridDim.x * 256) {
        const int c = (int)(u % C4) * 4;
        const int64_t e = (int64_t)g * units + u;
        float4 d = ((const float4*)a.dz)[e];
        if (a.z) {
            const float4 zz = ((const float4*)a.z)[e];
            d.x = zz.x > 0.f ? d.x : 0.f; d.y = zz.y > 0.f ? d.y : 0.f;
            d.z = zz.z > 0.f ? d.z : 0.f; d.w = zz.w > 0.f ? d.w : 0.f;
        } else if (a.mask_from_y) {
            const float4 y = ((const float4*)a.y[0])[e];
            d.x = __fmaf_rn(y.x, sm[2 * a.C + c], sm[5 * a.C + c]) > 0.f ? d.x : 0.f;
            d.y = __fmaf_rn(y.y, sm[2 * a.C + c + 1], sm[5 * a.C + c + 1]) > 0.f ? d.y : 0.f;
            d.z = __fmaf_rn(y.z, sm[2 * a.C + c + 2], sm[5 * a.C + c + 2]) > 0.f ? d.z : 0.f;
            d.w = __fmaf_rn(y.w, sm[2 * a.C + c + 3], sm[5 * a.C + c + 3]) > 0.f ? d.w : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k < a.nsets) {
                const float* s = sm + (size_t)k * 6 * a.C;
                const float4 y = ((const float4*)a.y[k])[e];
                float4 o;
                o.x = s[2 * a.C + c] * (d.x - s[c] - (y.x - s[3 * a.C + c]) * s[4 * a.C + c] * s[a.C + c]);
                o.y = s[2 * a.C + c + 1] * (d.y - s[c + 1] - (y.y - s[3 * a.C + c + 1]) * s[4 * a.C + c + 1] * s[a.C + c + 1]);
                o.z = s[2 * a.C + c + 2] * (d.z - s[c + 2] - (y.z - s[3 * a.C + c + 2]) * s[4 * a.C + c + 2] * s[a.C + c + 2]);
                o.w = s[2 * a.C + c + 3] * (d.w - s[c + 3] - (y.w - s[3 * a.C + c + 3]) * s[4 * a.C + c + 3] * s[a.C + c + 3]);
                ((float4*)a.dy[k])[e] = o;
            }
    }
}

// One-pass BatchNorm backward (one BatchNorm, <= 2 groups): every thread keeps its share of the masked gradient and of xhat in
// registers (<= E float4 each), the workgroups reduce, meet at a grid-wide arrival counter, and apply from registers: dz, z, y are
// read once and dy written once (4 tensor passes instead of the 7 of reduce + apply).  All workgroups must be resident at once:
// the grid is one 512-thread workgroup per CU (54-160 VGPRs, 17 KB LDS); workgroups that find their CU full of weight-gradient
// workgroups of the second stream start when one of those retires; the wait is bounded so that a scheduling surprise shows up as a parity failure, not as a hung GPU.
constexpr int kBnFusedThreads = 512;
// accumulator replicas (same-address returning atomics serialise at the coherence point: 256 workgroups on one address cost ~20 us)
constexpr int kBnFusedReps = 8;
#ifndef OCL_BN_FLAT
#define OCL_BN_FLAT 40
#endif
constexpr int kBnFusedFlat = OCL_BN_FLAT;   // grids up to this size arrive at one counter
// NS = 2: the two BatchNorms of a projection block (main path + shortcut) share the masked gradient dz; their outputs differ only
// in xhat.  One launch reads dz, z, y_a, y_b and writes dy_a, dy_b (6 tensor passes, one grid arrival) instead of reduce + apply
// (10 passes, 2 launches).  The sum of the masked gradient is the same for both; each BatchNorm's arena receives it with its own
// sum of d * xhat.
template <int E, int NS = 1>
__global__ void __launch_bounds__(kBnFusedThreads) bn_bwd_fused_kernel(const BnBwdArgs a) {
    __shared__ float4 red[1 + NS][kBnFusedThreads];
    __shared__ float kk[1 + NS][4 * 40];
    __shared__ bool timed_out;   // some workgroup never arrived (not all resident at once): the results are poisoned with NaN
    const int C4 = a.C >> 2;
    const int tid = threadIdx.x;
    if (tid == 0) timed_out = false;
    const int wpg = gridDim.x / a.G;                   // workgroups per group
    const int g = blockIdx.x / wpg;
    const int S = (wpg * kBnFusedThreads / C4) * C4;   // unit stride of a thread: a multiple of C4, so its channel quad is fixed
    const int gt = (blockIdx.x - g * wpg) * kBnFusedThreads + tid;
    const int c4 = gt % C4;
    const int64_t M = a.m_per_group;
    const int64_t units = M * C4;
    const float4* dz4 = (const float4*)a.dz + (int64_t)g * units;
    const float4* z4 = a.z ? (const float4*)a.z + (int64_t)g * units : nullptr;
    const bool live = g < a.G && gt < S;
    float4 d[E], xh[NS][E];
    float4 sd = make_float4(0.f, 0.f, 0.f, 0.f), sx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sx[k] = sd;
    if (live) {
        float4 zz[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int64_t u = (int64_t)gt + (int64_t)e * S;
            const bool in = u < units;
            const int64_t uu = in ? u : 0;
            d[e] = dz4[uu];
#pragma unroll
            for (int k = 0; k < NS; ++k) xh[k][e] = ((const float4*)a.y[k] + (int64_t)g * units)[uu];
            zz[e] = z4 ? z4[uu] : make_float4(1.f, 1.f, 1.f, 1.f);
            if (!in) d[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (a.mask_from_y) {   // the activation was never written: its sign from the raw output, with the staging kernels' arithmetic
            const float4 gm = *(const float4*)(a.gamma[0] + c4 * 4), bt = *(const float4*)(a.beta[0] + c4 * 4);
            const float4 mn = *(const float4*)(a.mean[0] + (int64_t)g * a.C + c4 * 4), is = *(const float4*)(a.invstd[0] + (int64_t)g * a.C + c4 * 4);
            float4 sc, sh;
            bn_scale_shift(gm.x, bt.x, mn.x, is.x, sc.x, sh.x); bn_scale_shift(gm.y, bt.y, mn.y, is.y, sc.y, sh.y);
            bn_scale_shift(gm.z, bt.z, mn.z, is.z, sc.z, sh.z); bn_scale_shift(gm.w, bt.w, mn.w, is.w, sc.w, sh.w);
#pragma unroll
            for (int e = 0; e < E; ++e)
                zz[e] = make_float4(__fmaf_rn(xh[0][e].x, sc.x, sh.x), __fmaf_rn(xh[0][e].y, sc.y, sh.y), __fmaf_rn(xh[0][e].z, sc.z, sh.z),
                                    __fmaf_rn(xh[0][e].w, sc.w, sh.w));
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            d[e].x = zz[e].x > 0.f ? d[e].x : 0.f; d[e].y = zz[e].y > 0.f ? d[e].y : 0.f;
            d[e].z = zz[e].z > 0.f ? d[e].z : 0.f; d[e].w = zz[e].w > 0.f ? d[e].w : 0.f;
            sd.x += d[e].x; sd.y += d[e].y; sd.z += d[e].z; sd.w += d[e].w;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float4 mean = *(const float4*)(a.mean[k] + (int64_t)g * a.C + c4 * 4);
            const float4 istd = *(const float4*)(a.invstd[k] + (int64_t)g * a.C + c4 * 4);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                xh[k][e].x = (xh[k][e].x - mean.x) * istd.x; xh[k][e].y = (xh[k][e].y - mean.y) * istd.y;
                xh[k][e].z = (xh[k][e].z - mean.z) * istd.z; xh[k][e].w = (xh[k][e].w - mean.w) * istd.w;
                sx[k].x = fmaf(d[e].x, xh[k][e].x, sx[k].x); sx[k].y = fmaf(d[e].y, xh[k][e].y, sx[k].y);
                sx[k].z = fmaf(d[e].z, xh[k][e].z, sx[k].z); sx[k].w = fmaf(d[e].w, xh[k][e].w, sx[k].w);
            }
        }
    }
    red[0][tid] = sd;
#pragma unroll
    for (int k = 0; k < NS; ++k) red[1 + k][tid] = sx[k];
    __syncthreads();
    // threads of this workgroup with channel quad q: tid = first(q) + k*C4
    if (g < a.G && tid < (1 + NS) * C4) {
        const int which = tid / C4, q = tid - which * C4;   // 0: sum d; 1 + k: sum d * xhat of BatchNorm k
        const int base = (blockIdx.x - g * wpg) * kBnFusedThreads;
        int first = (q - base % C4 + C4) % C4;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
        for (int t = first; t < kBnFusedThreads; t += C4) {
            const float4 v = red[which][t];
            t0 += (double)v.x; t1 += (double)v.y; t2 += (double)v.z; t3 += (double)v.w;
        }
        unsigned long long r = 0ull;
        // returning atomics: the wave waits for them to have executed (at the device-wide coherence point) before the barrier below
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (which != 0 && which != 1 + k) continue;   // the sum of d goes to both arenas, the sum of d * xhat_k to its own
            StatCell* arena = k == 0 ? a.fsums : a.fsums_b;
            StatCell* dst = arena + ((int64_t)(blockIdx.x % kBnFusedReps) * a.G * 2 + (int64_t)g * 2 + (which ? 1 : 0)) * a.C + q * 4;
            r += fx_fetch_add(dst + 0, t0) + fx_fetch_add(dst + 1, t1) + fx_fetch_add(dst + 2, t2) + fx_fetch_add(dst + 3, t3);
        }
        if (r == 0x123456789abcdef1ull) red[0][0].x = 0.f;   // keeps the returns (practically never true)
    }
    // ---- grid-wide arrival ---------------------------------------------------------------------------
    // Relaxed device-scope atomics only: they execute at the coherence point and bypass the per-XCD L2, so no release / acquire
    // fence (an L2 write-back + invalidate per fence on this part: ~50 us per launch when the spin loop carried an acquire).
    __syncthreads();
    if (tid == 0) {
        // two-level arrival: 8 sub-counters (same-address atomics serialise: 256 arrivals on one counter cost ~15 us), the last
        // arrival of each sub-counter reports to the master counter a.barrier[0]
        const unsigned sub = blockIdx.x % kBnFusedReps;
        const unsigned members = (gridDim.x - sub + kBnFusedReps - 1) / kBnFusedReps;
        // (replay-sized passes run 8 - 33 workgroups: they arrive at the master counter directly -- one device-scope round trip less in a
        // kernel that is nothing but such round trips there, profiles/r6_bn_flat_arrival_ab.txt)
        const bool flat = gridDim.x <= (unsigned)kBnFusedFlat;
        const unsigned groups_total = flat ? gridDim.x : (unsigned)kBnFusedReps;
        if (flat || __hip_atomic_fetch_add(a.barrier + 1 + sub, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1)
            __hip_atomic_fetch_add(a.barrier, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(a.barrier, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < groups_total && ++spins < (1 << 22))
            __builtin_amdgcn_s_sleep(1);
        timed_out = spins >= (1 << 22);
        if (timed_out && a.err) __hip_atomic_fetch_or(a.err, (unsigned)ASYNC_ERR_BN_BARRIER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    const double Md = (double)M;
    if (g < a.G && tid < (1 + NS) * a.C) {
        const int which = tid / a.C, c = tid - which * a.C;
        const StatCell* arena = which <= 1 ? a.fsums : a.fsums_b;
        const double v = fx_total_atomic(arena, (int64_t)a.G * 2 * a.C, ((int64_t)g * 2 + (which ? 1 : 0)) * a.C + c);
        kk[which][c] = timed_out ? __builtin_nanf("") : (float)(v / Md);
    }
    if (blockIdx.x == 0 && tid < NS * a.C) {   // dgamma / dbeta over all groups
        const int k = tid / a.C, c = tid - k * a.C;
        const StatCell* arena = k == 0 ? a.fsums : a.fsums_b;
        double db = 0.0, dg = 0.0;
        for (int gg = 0; gg < a.G; ++gg) {   // (each group's total is exact; the groups are added in order)
            db += fx_total_atomic(arena, (int64_t)a.G * 2 * a.C, ((int64_t)gg * 2 + 0) * a.C + c);
            dg += fx_total_atomic(arena, (int64_t)a.G * 2 * a.C, ((int64_t)gg * 2 + 1) * a.C + c);
        }
        if (a.accumulate) {
            a.dgamma[k][c] += (float)dg;
            a.dbeta[k][c] += (float)db;
        } else {
            a.dgamma[k][c] = (float)dg;
            a.dbeta[k][c] = (float)db;
        }
    }
    __syncthreads();
    if (live) {
        const float4 k1 = *(const float4*)&kk[0][c4 * 4];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float4 k2 = *(const float4*)&kk[1 + k][c4 * 4];
            const float4 gm = *(const float4*)(a.gamma[k] + c4 * 4);
            const float4 istd = *(const float4*)(a.invstd[k] + (int64_t)g * a.C + c4 * 4);
            const float4 sc = make_float4(gm.x * istd.x, gm.y * istd.y, gm.z * istd.z, gm.w * istd.w);
            float4* o4 = (float4*)a.dy[k] + (int64_t)g * units;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int64_t u = (int64_t)gt + (int64_t)e * S;
                if (u < units) {
                    float4 o;
                    o.x = sc.x * (d[e].x - k1.x - xh[k][e].x * k2.x);
                    o.y = sc.y * (d[e].y - k1.y - xh[k][e].y * k2.y);
                    o.z = sc.z * (d[e].z - k1.z - xh[k][e].z * k2.z);
                    o.w = sc.w * (d[e].w - k1.w - xh[k][e].w * k2.w);
                    o4[u] = o;
                }
            }
        }
    }
}

// BatchNorm backward of a SMALL map (layer 4 of a replay-sized pass), partitioned by CHANNEL: one workgroup
// owns one channel quad for every pixel of every group, so its batch sums need nobody else -- no atomics, no grid-wide arrival, no replicas
// to read back.  bn_bwd_fused_kernel on such a map is five dependent device-scope round trips (10.8 - 12.5 us for a few hundred KB); here:
// one strided read of dz, z, y (16 bytes per lane at a stride of C floats), a wave butterfly + the wave totals in fp64 in a fixed order
// (deterministic), the apply from registers: 6.7 - 8.4 us at one unit per thread (profiles/r6_bn_chan_ab.txt; at four units per thread --
// layer 3 of a 20-image pass on 20 workgroups -- it LOSES to the one-pass kernel, hence the size gate in launch_bn_bwd).  Two groups split
// the workgroup's threads (the two-group replay pass of ER: 10 + 10 images).  NS as bn_bwd_fused_kernel.
constexpr int kBnChanThreads = 512;
template <int E, int NS>
__global__ void __launch_bounds__(kBnChanThreads) bn_bwd_chan_kernel(const BnBwdArgs a) {
    constexpr int NW = kBnChanThreads / 64;
    __shared__ double wred[1 + NS][4][NW];
    __shared__ double tot[2][1 + NS][4];
    __shared__ float kk[2][1 + NS][4];
    const int c4 = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C4 = a.C >> 2;
    const int T = kBnChanThreads / a.G;           // threads per group (G = 1 or 2)
    const int g = tid / T, pt = tid - g * T;
    const int64_t M = a.m_per_group;
    const float4 f4z = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t base = (int64_t)g * M * C4 + c4;
    float4 d[E], xh[NS][E], zz[E];
    float4 sd = f4z, sx[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) sx[k] = f4z;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int64_t pix = pt + (int64_t)e * T;
        const bool in = pix < M;
        const int64_t u = base + (in ? pix : 0) * C4;
        d[e] = ((const float4*)a.dz)[u];
#pragma unroll
        for (int k = 0; k < NS; ++k) xh[k][e] = ((const float4*)a.y[k])[u];
        zz[e] = a.z ? ((const float4*)a.z)[u] : make_float4(1.f, 1.f, 1.f, 1.f);
        if (!in) d[e] = f4z;
    }
    if (a.mask_from_y) {   // (the arithmetic of the staging kernels, as in bn_bwd_fused_kernel)
        const float4 gm = *(const float4*)(a.gamma[0] + c4 * 4), bt = *(const float4*)(a.beta[0] + c4 * 4);
        const float4 mn = *(const float4*)(a.mean[0] + (int64_t)g * a.C + c4 * 4), is = *(const float4*)(a.invstd[0] + (int64_t)g * a.C + c4 * 4);
        float4 sc, sh;
        bn_scale_shift(gm.x, bt.x, mn.x, is.x, sc.x, sh.x); bn_scale_shift(gm.y, bt.y, mn.y, is.y, sc.y, sh.y);
        bn_scale_shift(gm.z, bt.z, mn.z, is.z, sc.z, sh.z); bn_scale_shift(gm.w, bt.w, mn.w, is.w, sc.w, sh.w);
#pragma unroll
        for (int e = 0; e < E; ++e)
            zz[e] = make_float4(__fmaf_rn(xh[0][e].x, sc.x, sh.x), __fmaf_rn(xh[0][e].y, sc.y, sh.y), __fmaf_rn(xh[0][e].z, sc.z, sh.z),
                                __fmaf_rn(xh[0][e].w, sc.w, sh.w));
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        d[e].x = zz[e].x > 0.f ? d[e].x : 0.f; d[e].y = zz[e].y > 0.f ? d[e].y : 0.f;
        d[e].z = zz[e].z > 0.f ? d[e].z : 0.f; d[e].w = zz[e].w > 0.f ? d[e].w : 0.f;
        sd.x += d[e].x; sd.y += d[e].y; sd.z += d[e].z; sd.w += d[e].w;
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const float4 mean = *(const float4*)(a.mean[k] + (int64_t)g * a.C + c4 * 4);
        const float4 istd = *(const float4*)(a.invstd[k] + (int64_t)g * a.C + c4 * 4);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            xh[k][e].x = (xh[k][e].x - mean.x) * istd.x; xh[k][e].y = (xh[k][e].y - mean.y) * istd.y;
            xh[k][e].z = (xh[k][e].z - mean.z) * istd.z; xh[k][e].w = (xh[k][e].w - mean.w) * istd.w;
            sx[k].x = fmaf(d[e].x, xh[k][e].x, sx[k].x); sx[k].y = fmaf(d[e].y, xh[k][e].y, sx[k].y);
            sx[k].z = fmaf(d[e].z, xh[k][e].z, sx[k].z); sx[k].w = fmaf(d[e].w, xh[k][e].w, sx[k].w);
        }
    }
    // wave butterfly in fp64 (a lane's partial covers <= E values; a wave lies inside one group), wave totals to LDS
    auto wsum = [&](float v) __attribute__((always_inline)) -> double {
        double t = (double)v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    {
        const double t0 = wsum(sd.x), t1 = wsum(sd.y), t2 = wsum(sd.z), t3 = wsum(sd.w);
        if (lane == 0) { wred[0][0][wave] = t0; wred[0][1][wave] = t1; wred[0][2][wave] = t2; wred[0][3][wave] = t3; }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double t0 = wsum(sx[k].x), t1 = wsum(sx[k].y), t2 = wsum(sx[k].z), t3 = wsum(sx[k].w);
        if (lane == 0) { wred[1 + k][0][wave] = t0; wred[1 + k][1][wave] = t1; wred[1 + k][2][wave] = t2; wred[1 + k][3][wave] = t3; }
    }
    __syncthreads();
    if (tid < (1 + NS) * 4 * a.G) {
        const int gg = tid / ((1 + NS) * 4), r = tid - gg * (1 + NS) * 4;
        const int which = r >> 2, c = r & 3;
        const int wpg = NW / a.G;
        double t = 0.0;
        for (int w = gg * wpg; w < (gg + 1) * wpg; ++w) t += wred[which][c][w];
        tot[gg][which][c] = t;
        kk[gg][which][c] = (float)(t / (double)M);
    }
    __syncthreads();
    if (tid < (1 + NS) * 4) {   // dbeta = sum(d), dgamma_k = sum(d * xhat_k), over the groups in order
        const int which = tid >> 2, c = tid & 3, ch = c4 * 4 + c;
        double t = tot[0][which][c];
        if (a.G == 2) t += tot[1][which][c];
        if (which == 0) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                if (a.accumulate) a.dbeta[k][ch] += (float)t;
                else a.dbeta[k][ch] = (float)t;
            }
        } else {
            if (a.accumulate) a.dgamma[which - 1][ch] += (float)t;
            else a.dgamma[which - 1][ch] = (float)t;
        }
    }
    const float4 k1 = *(const float4*)&kk[g][0][0];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const float4 k2 = *(const float4*)&kk[g][1 + k][0];
        const float4 gm = *(const float4*)(a.gamma[k] + c4 * 4);
        const float4 istd = *(const float4*)(a.invstd[k] + (int64_t)g * a.C + c4 * 4);
        const float4 sc = make_float4(gm.x * istd.x, gm.y * istd.y, gm.z * istd.z, gm.w * istd.w);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int64_t pix = pt + (int64_t)e * T;
            if (pix < M) {
                float4 o;
                o.x = sc.x * (d[e].x - k1.x - xh[k][e].x * k2.x);
                o.y = sc.y * (d[e].y - k1.y - xh[k][e].y * k2.y);
                o.z = sc.z * (d[e].z - k1.z - xh[k][e].z * k2.z);
                o.w = sc.w * (d[e].w - k1.w - xh[k][e].w * k2.w);
                ((float4*)a.dy[k])[base + pix * C4] = o;
            }
        }
    }
}

static int g_bn_bwd_cap = 0, g_bn_bwd_unroll = 0, g_bn_bwd_phase = 0;   // micro-benchmark overrides (kbench)
void bn_bwd_tune(int cap, int unroll, int phase) { g_bn_bwd_cap = cap; g_bn_bwd_unroll = unroll; g_bn_bwd_phase = phase; }

static int g_bn_fused = -1;   // -1: environment (OCL_BN_FUSED, default on; 0 = the reduce + apply pair that passes of > 2 groups use anyway: the way out when a
                              // shared GPU cannot hold the one-pass kernel's grid-wide arrival, see check_async_error; tests/test_gpu_ring.py)
static int g_num_cus = 0;
void bn_bwd_fused_enable(int on) { g_bn_fused = on; }

static int g_bn_bwd_last_path = 0;   // host: the path of the last launch_bn_bwd (bn_bwd_last_path)
int bn_bwd_last_path() { return g_bn_bwd_last_path; }

int launch_bn_bwd(const BnBwdArgs& a, hipStream_t s) {
    OCL_REQUIRE(a.nsets == 1 || a.nsets == 2, "bn_bwd: nsets=%d", a.nsets);
    const int C4 = a.C / 4, PT = 256 / C4;
    if (g_bn_fused < 0) g_bn_fused = env_int("OCL_BN_FUSED", 1);
    // small maps: one workgroup per channel quad, no cross-workgroup reduction (bn_bwd_chan_kernel; OCL_BN_CHAN=0: off).  Gate: ONE unit per
    // thread (all groups' pixels <= 512: layer 4 up to 32 images) and >= 16 channel quads; at two units per thread it is neutral (6 x 84x84) or
    // loses (64 images in two groups: +7.5 us per pass), at four (layer 3 of a 20-image pass) it loses -- profiles/r6_bn_chan_ab.txt
    static const bool bn_chan = env_not_off("OCL_BN_CHAN");
    if (bn_chan && g_bn_fused && !a.frozen && g_bn_bwd_phase == 0 && a.G <= 2 && C4 >= 16 && a.m_per_group * a.G <= kBnChanThreads) {
        ProfScope ps(PROF_BN, s);
        g_bn_bwd_last_path = 1010 + a.nsets;
        if (a.nsets == 2) hipLaunchKernelGGL((bn_bwd_chan_kernel<1, 2>), dim3(C4), dim3(kBnChanThreads), 0, s, a);
        else hipLaunchKernelGGL((bn_bwd_chan_kernel<1, 1>), dim3(C4), dim3(kBnChanThreads), 0, s, a);
        OCL_LAUNCH_CHECK();
        return OCL_OK;
    }
    if (g_bn_fused && a.barrier && a.fsums && (a.nsets == 1 || a.fsums_b) && a.G <= 2 && a.C <= 160 && g_bn_bwd_phase == 0 && !a.frozen) {
        if (!g_num_cus) {
            int dev = 0;
            hipDeviceProp_t prop;
            OCL_HIP(hipGetDevice(&dev));
            OCL_HIP(hipGetDeviceProperties(&prop, dev));
            // residency: the grid never exceeds one workgroup per CU, and every instantiation must be admissible at that rate
            // (checked once against the occupancy query); a time-out at run time is reported through the asynchronous error word
            int b3 = 0, b6 = 0, b12 = 0, c3 = 0, c6 = 0;
            OCL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b3, bn_bwd_fused_kernel<3>, kBnFusedThreads, 0));
            OCL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b6, bn_bwd_fused_kernel<6>, kBnFusedThreads, 0));
            OCL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b12, bn_bwd_fused_kernel<12>, kBnFusedThreads, 0));
            OCL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c3, (bn_bwd_fused_kernel<3, 2>), kBnFusedThreads, 0));
            OCL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&c6, (bn_bwd_fused_kernel<6, 2>), kBnFusedThreads, 0));
            if (std::min(std::min(b3, std::min(b6, b12)), std::min(c3, c6)) < 1) g_bn_fused = 0;   // cannot be co-resident: two-kernel path
            g_num_cus = std::max(2, prop.multiProcessorCount);
        }
        // about 6 float4 per thread and tensor; never more workgroups than CUs (all must be resident), fewer for the small maps
        // (the arrival costs grow with the workgroup count, the small maps are latency-bound anyway)
        const int64_t total_units = a.m_per_group * C4 * a.G;
        const int per_thread = a.nsets == 2 ? 5 : 6;   // (two sets keep one more register array per unit: at most 6 units per thread)
        int grid = (int)std::min<int64_t>(g_num_cus, std::max<int64_t>(8, (total_units + kBnFusedThreads * per_thread - 1) / (kBnFusedThreads * per_thread)));
        grid = std::max(a.G, grid / a.G * a.G);
        const int wpg = grid / a.G;
        const int64_t S = (int64_t)(wpg * kBnFusedThreads / C4) * C4;
        const int64_t need = (a.m_per_group * C4 + S - 1) / S;
        if (a.nsets == 2 && need <= 6 && g_bn_fused) {   // two BatchNorms sharing dz (projection blocks)
            ProfScope ps(PROF_BN, s);
            BnBwdArgs af = a;
            af.err = async_error_word_device();
            g_bn_bwd_last_path = 2000 + (need <= 3 ? 30 : 60) + 2;
            if (need <= 3) hipLaunchKernelGGL((bn_bwd_fused_kernel<3, 2>), dim3(grid), dim3(kBnFusedThreads), 0, s, af);
            else hipLaunchKernelGGL((bn_bwd_fused_kernel<6, 2>), dim3(grid), dim3(kBnFusedThreads), 0, s, af);
            OCL_LAUNCH_CHECK();
            return OCL_OK;
        }
        if (a.nsets == 1 && need <= 12 && g_bn_fused) {
            ProfScope ps(PROF_BN, s);
            BnBwdArgs af = a;
            af.err = async_error_word_device();
            g_bn_bwd_last_path = 2000 + (need <= 3 ? 30 : need <= 6 ? 60 : 120) + 1;
            if (need <= 3) hipLaunchKernelGGL(bn_bwd_fused_kernel<3>, dim3(grid), dim3(kBnFusedThreads), 0, s, af);
            else if (need <= 6) hipLaunchKernelGGL(bn_bwd_fused_kernel<6>, dim3(grid), dim3(kBnFusedThreads), 0, s, af);
            else hipLaunchKernelGGL(bn_bwd_fused_kernel<12>, dim3(grid), dim3(kBnFusedThreads), 0, s, af);
            OCL_LAUNCH_CHECK();
            return OCL_OK;
        }
    }
    const int U = g_bn_bwd_unroll ? g_bn_bwd_unroll : 4;
    // passes per block: 8 for the large maps, 4 once a group has fewer than 1024 passes in total (more, shorter blocks: the
    // small layers are latency-bound) -- profiles/r1_kbench_bn_sweep.txt
    const int passes = g_bn_bwd_cap > 1024 ? (g_bn_bwd_cap > 2048 ? 2 : 4) : (g_bn_bwd_cap == 0 && a.m_per_group / PT < 1024 ? 4 : 8);
    const int cap = g_bn_bwd_cap ? g_bn_bwd_cap : 1024;
    const int64_t per_block_pixels = (int64_t)PT * passes;
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(1, cap / a.G), (a.m_per_group + per_block_pixels - 1) / per_block_pixels));
    ProfScope ps(PROF_BN, s);
    g_bn_bwd_last_path = 3000 + a.nsets;
    const size_t sm1 = (size_t)a.nsets * 2 * PT * a.C * 4;
    if (g_bn_bwd_phase != 2) {
        if (U == 1) hipLaunchKernelGGL(bn_bwd_reduce_kernel<1>, dim3(bx, a.G), dim3(256), sm1, s, a);
        else if (U == 2) hipLaunchKernelGGL(bn_bwd_reduce_kernel<2>, dim3(bx, a.G), dim3(256), sm1, s, a);
        else hipLaunchKernelGGL(bn_bwd_reduce_kernel<4>, dim3(bx, a.G), dim3(256), sm1, s, a);
        OCL_LAUNCH_CHECK();
    }
    if (g_bn_bwd_phase == 1) return OCL_OK;
    const int64_t units = a.m_per_group * C4;
    const int bx2 = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (units + 1023) / 1024));
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(bx2, a.G), dim3(256), (size_t)a.nsets * 6 * a.C * 4, s, a);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// ---- apply half of a BatchNorm backward whose two batch sums came out of the producing data gradient's epilogue (EPI_BNB) ------------
// d is the ReLU-masked gradient; per (group, channel): k1 = sum(d) / M, k2 = invstd * sum(d * (y - mean)) / M (= mean of d * xhat);
// dy = gamma * invstd * (d - k1 - xhat * k2), the statement of bn_bwd_apply_kernel.  The replicas are summed in a fixed order.
__global__ void __launch_bounds__(256) bn_bwd_apply_e_kernel(const BnApplyEArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // k1[C], k2[C], scale[C], mean[C], invstd[C]
    const int g = blockIdx.y, tid = threadIdx.x;
    const double Md = (double)a.m_per_group;
    for (int c = tid; c < a.C; c += 256) {
        const float istd = a.invstd[(int64_t)g * a.C + c];
        double s1, s2;
        fx_total2(a.esums, a.esums_rep_stride, ((int64_t)g * 2 + 0) * a.C + c, ((int64_t)g * 2 + 1) * a.C + c, s1, s2);
        sm[c] = (float)(s1 / Md);
        sm[a.C + c] = (float)(s2 * (double)istd / Md);
        sm[2 * a.C + c] = a.gamma[c] * istd;
        sm[3 * a.C + c] = a.mean[(int64_t)g * a.C + c];
        sm[4 * a.C + c] = istd;
        if (blockIdx.x == 0 && g == 0) {   // dgamma = sum over the groups of sum(d * xhat), dbeta = sum(d)
            double dg = 0.0, db = 0.0;
            for (int gg = 0; gg < a.G; ++gg) {
                double t1, t2;
                fx_total2(a.esums, a.esums_rep_stride, ((int64_t)gg * 2 + 0) * a.C + c, ((int64_t)gg * 2 + 1) * a.C + c, t1, t2);
                db += t1;
                dg += t2 * (double)a.invstd[(int64_t)gg * a.C + c];
            }
            if (a.accumulate) {
                a.dgamma[c] += (float)dg;
                a.dbeta[c] += (float)db;
            } else {
                a.dgamma[c] = (float)dg;
                a.dbeta[c] = (float)db;
            }
        }
    }
    __syncthreads();
    const int C4 = a.C >> 2;
    const int64_t units = a.m_per_group * C4;
    const float4* d4 = (const float4*)a.d + (int64_t)g * units;
    const float4* y4 = (const float4*)a.y + (int64_t)g * units;
    float4* o4 = (float4*)a.dy + (int64_t)g * units;
    const int64_t stride = (int64_t)gridDim.x * 256;
    auto one = [&](int64_t u, const float4 d, const float4 y) __attribute__((always_inline)) {
        const int c = (int)(u % C4) * 4;
        float4 o;
        o.x = sm[2 * a.C + c] * (d.x - sm[c] - (y.x - sm[3 * a.C + c]) * sm[4 * a.C + c] * sm[a.C + c]);
        o.y = sm[2 * a.C + c + 1] * (d.y - sm[c + 1] - (y.y - sm[3 * a.C + c + 1]) * sm[4 * a.C + c + 1] * sm[a.C + c + 1]);
        o.z = sm[2 * a.C + c + 2] * (d.z - sm[c + 2] - (y.z - sm[3 * a.C + c + 2]) * sm[4 * a.C + c + 2] * sm[a.C + c + 2]);
        o.w = sm[2 * a.C + c + 3] * (d.w - sm[c + 3] - (y.w - sm[3 * a.C + c + 3]) * sm[4 * a.C + c + 3] * sm[a.C + c + 3]);
        o4[u] = o;
    };
    int64_t u = (int64_t)blockIdx.x * 256 + tid;
    for (; u + 3 * stride < units; u += 4 * stride) {   // four units in flight per thread
        const float4 d0 = d4[u], d1 = d4[u + stride], d2 = d4[u + 2 * stride], d3 = d4[u + 3 * stride];
        const float4 y0 = y4[u], y1 = y4[u + stride], y2 = y4[u + 2 * stride], y3 = y4[u + 3 * stride];
        one(u, d0, y0); one(u + stride, d1, y1); one(u + 2 * stride, d2, y2); one(u + 3 * stride, d3, y3);
    }
    for (; u < units; u += stride) one(u, d4[u], y4[u]);
}

int launch_bn_apply_e(const BnApplyEArgs& a, hipStream_t s) {
    OCL_REQUIRE(a.C % 4 == 0 && a.G >= 1 && a.m_per_group > 0, "bn_apply_e: C=%d G=%d", a.C, a.G);
    const int64_t units = a.m_per_group * (a.C / 4);
    const int bx = (int)std::max<int64_t>(1, std::min<int64_t>(1024 / a.G, (units + 1023) / 1024));
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(bn_bwd_apply_e_kernel, dim3(bx, a.G), dim3(256), (size_t)5 * a.C * 4, s, a);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

}  // namespace ocl
