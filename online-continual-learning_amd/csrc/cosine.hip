// GSS: the largest cosine similarity between a gradient vector and k stored ones, in two deterministic passes (no atomics).
#include "small_ops.h"
#include <math.h>
#include <algorithm>

using namespace ocl;

constexpr int kCosChunk = 4;   // float4 per thread and pass
constexpr int kCosMaxBlocks = 512;
// (the size and form variants of a path are consecutive codes: plan_cosine and plan_supcon add an offset to the first)
static_assert(OCL_PATH_COS_VEC_CAP == OCL_PATH_COS_VEC_ONE + 2 && OCL_PATH_COS_VEC_MULTI == OCL_PATH_COS_VEC_ONE + 1 &&
              OCL_PATH_COS_SCALAR_CAP == OCL_PATH_COS_SCALAR_ONE + 2 && OCL_PATH_COS_SCALAR_MULTI == OCL_PATH_COS_SCALAR_ONE + 1, "cosine path codes");
namespace ocl {
SPlan plan_cosine(const void* mem, const void* g, int k, int64_t n) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kCosMaxBlocks, (n / 4 + 256 * kCosChunk - 1) / (256 * kCosChunk)));
    const bool vec = n % 4 == 0 && aligned16(mem, g);   // rows are 16-byte aligned -> float4 loads; otherwise scalar loads (any n)
    const int size = blocks == 1 ? 0 : blocks == kCosMaxBlocks ? 2 : 1;
    SPlan p = splan((vec ? OCL_PATH_COS_VEC_ONE : OCL_PATH_COS_SCALAR_ONE) + size, (unsigned)blocks, 1, 256);
    p.aux = blocks;
    p.grid2_x = 1; p.block2 = 64;
    return p;
}
}  // namespace ocl

// =====================================================================================================
// GSS: max_i cos(mem_i, g) over k stored gradient vectors (utils/buffer/buffer_utils.py:51-56, gss_greedy_update.py:79,121)
// =====================================================================================================
// Pass 1: every workgroup owns a contiguous range of the vector; g's chunk stays in registers while the k rows stream past
// it; fp32 lane partials, fp64 from the wave reduction on, one fp64 partial per (workgroup, row) in the workspace
// [blocks][2k + 1] -- no atomics: pass 2 (one wave) sums the workgroups' partials in a fixed order, so the scores (which feed hard
// decisions: `batch_sim < 0`, multinomial weights, the stored buffer_score) are bit-reproducible run to run.
// (kCosChunk float4 per thread and pass size the grid: plan_cosine)
// VEC: rows are 16-byte aligned (n % 4 == 0) -> float4 loads; otherwise scalar loads (any n)
template <bool VEC>
__global__ void __launch_bounds__(256) cosine_partial_kernel(const float* __restrict__ mem, int k, int64_t n,
                                                             const float* __restrict__ g, double* __restrict__ acc) {
    __shared__ double red[4];
    const int64_t units = VEC ? (n >> 2) : n;
    const int64_t per = (units + gridDim.x - 1) / gridDim.x;
    const int64_t beg = (int64_t)blockIdx.x * per, end = min(units, beg + per);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    auto block_add = [&](double v, double* dst) {
        v = wave_sum_d(v);
        __syncthreads();
        if (lane == 0) red[wid] = v;
        __syncthreads();
        if (threadIdx.x == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
    };
    acc += (int64_t)blockIdx.x * (2 * k + 1);   // this workgroup's row of partials
    for (int r = -1; r < k; ++r) {   // r = -1: |g|^2
        const float* row = r < 0 ? g : mem + (int64_t)r * n;
        float sd = 0.f, sm = 0.f;
        if (VEC) {
            const float4* m4 = (const float4*)row;
            const float4* g4 = (const float4*)g;
            for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
                const float4 a = m4[i], b = g4[i];
                sd = fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, sd))));
                sm = fmaf(a.x, a.x, fmaf(a.y, a.y, fmaf(a.z, a.z, fmaf(a.w, a.w, sm))));
            }
        } else {
            for (int64_t i = beg + threadIdx.x; i < end; i += 256) {
                const float a = row[i], b = g[i];
                sd = fmaf(a, b, sd);
                sm = fmaf(a, a, sm);
            }
        }
        if (r < 0) {
            block_add((double)sm, acc + 2 * k);
        } else {
            block_add((double)sd, acc + 2 * r);
            block_add((double)sm, acc + 2 * r + 1);
        }
    }
}
__global__ void __launch_bounds__(64) cosine_finish_kernel(const double* __restrict__ acc, int nblocks, int k, float eps, float* __restrict__ out) {
    const int lane = threadIdx.x;
    float best = -INFINITY;
    const int W = 2 * k + 1;
    auto total = [&](int col) {   // workgroups in ascending order
        double t = 0.0;
        for (int b = 0; b < nblocks; ++b) t += acc[(int64_t)b * W + col];
        return t;
    };
    const float ng = sqrtf((float)total(2 * k));
    for (int r = lane; r < k; r += 64) {
        const float w = fmaxf(sqrtf((float)total(2 * r + 1)) * ng, eps);
        best = fmaxf(best, (float)total(2 * r) / w);
    }
    best = wave_max(best);
    if (lane == 0) out[0] = best;
}

int64_t ocl_cosine_max_workspace_bytes(int k) { return (int64_t)kCosMaxBlocks * (2 * (int64_t)k + 1) * 8; }

int ocl_cosine_max(const float* mem, int k, int64_t n, const float* g, float eps, float* out, void* workspace, void* stream) {
    OCL_REQUIRE(mem && g && out && workspace && k > 0 && n > 0, "cosine_max: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_cosine(mem, g, k, n);
    if (pl.path >= OCL_PATH_COS_VEC_ONE && pl.path <= OCL_PATH_COS_VEC_CAP)
        hipLaunchKernelGGL(cosine_partial_kernel<true>, dim3(pl.grid_x), dim3(pl.block), 0, s, mem, k, n, g, (double*)workspace);
    else
        hipLaunchKernelGGL(cosine_partial_kernel<false>, dim3(pl.grid_x), dim3(pl.block), 0, s, mem, k, n, g, (double*)workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cosine_finish_kernel, dim3(pl.grid2_x), dim3(pl.block2), 0, s, (const double*)workspace, pl.aux, k, eps, out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
