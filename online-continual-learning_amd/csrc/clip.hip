// K8e: the global L2-norm clip of the flat gradient array (torch.nn.utils.clip_grad_norm_ with norm_type 2, error_if_nonfinite off;
// agents/gdumb.py:82 of the reference), between backward and the optimiser step.  Two launches, ordered on the stream, no host
// synchronisation, no atomics, no grid-wide arrival (the discipline of gradproj.hip):
//   clip_sumsq_kernel  per-block partial sums of g * g, every square and every sum in double (a float squared is exact in double),
//                      wave reduction by shuffles and block reduction through LDS in a fixed order;
//   clip_apply_kernel  the first wave of every block adds the partials in one fixed order (lane l takes partials l, l + 64, ... in
//                      index order, then the shuffle tree: all blocks get the same double), forms total = sqrt(sum) and
//                      coef = max_norm / (total + 1e-6) in double, and multiplies every element by (float)coef -- or, where the
//                      coefficient is at least 1 (torch clamps it to exactly 1.0 there), returns without touching an element.
// HBM/L2-bound fp32 streaming: 4 bytes per element read, then at most 4 read and 4 written.  IEEE '/' and sqrt (the compiler's
// default): nothing in this file may be built with fast-math.
#include "common.h"

using namespace ocl;

static constexpr int CLIP_THREADS = 256;
static constexpr int CLIP_MAX_BLOCKS = 512;

// a function of n alone: the partial sums, and with them the result, do not depend on the device or on the launch
static inline int clip_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(CLIP_MAX_BLOCKS, ((n >> 2) + CLIP_THREADS - 1) / CLIP_THREADS));
}

__global__ void __launch_bounds__(CLIP_THREADS) clip_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
    __shared__ double red[CLIP_THREADS / 64];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float4* g4 = (const float4*)g;
    double sq = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 a = g4[i];
        const double ax = a.x, ay = a.y, az = a.z, aw = a.w;
        sq += ax * ax;
        sq += ay * ay;
        sq += az * az;
        sq += aw * aw;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double a = g[i];
        sq += a * a;
    }
    sq = wave_sum_d(sq);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = red[0];
        for (int w = 1; w < CLIP_THREADS / 64; ++w) p += red[w];
        partial[blockIdx.x] = p;
    }
}

// every element is read and then written by the same thread
__global__ void __launch_bounds__(CLIP_THREADS) clip_apply_kernel(float* __restrict__ g, int64_t n, float max_norm,
                                                                  const double* __restrict__ partial, int nb, float* __restrict__ info4) {
    __shared__ double tot;
    if (threadIdx.x < 64) {   // at most 8 dependent adds per lane and the shuffle tree
        double p = 0.0;
        for (int b = threadIdx.x; b < nb; b += 64) p += partial[b];
        p = wave_sum_d(p);
        if (threadIdx.x == 0) tot = p;
    }
    __syncthreads();
    const double sumsq = tot;
    const double total = sqrt(sumsq);
    const double coef_d = (double)max_norm / (total + 1e-6);
    float coef = (float)coef_d;
    // !(>=), not (<): a NaN norm multiplies through, as torch's clamp(NaN, max=1) does; an infinite one gives coef = 0
    const bool clipped = !(coef_d >= 1.0) && !(coef == 1.0f);
    if (!clipped) coef = 1.0f;
    if (info4 != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        info4[0] = (float)total;
        info4[1] = coef;
        info4[2] = clipped ? 1.f : 0.f;
        info4[3] = (float)sumsq;
    }
    if (!clipped) return;   // torch multiplies by exactly 1.0 here: the array is the same bits either way
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* g4 = (float4*)g;
    for (int64_t i = first; i < n4; i += stride) {
        float4 a = g4[i];
        a.x *= coef;
        a.y *= coef;
        a.z *= coef;
        a.w *= coef;
        g4[i] = a;
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) g[i] *= coef;
}

int64_t ocl_clip_workspace_doubles(int64_t n) { return (int64_t)clip_blocks(n); }

int ocl_clip_grad_norm(float* grads_inout, int64_t n, float max_norm, double* workspace, int64_t workspace_doubles, float* info4,
                       void* stream) {
    OCL_REQUIRE(grads_inout && workspace, "clip: null pointer");
    OCL_REQUIRE(n > 0, "clip: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE(((uintptr_t)grads_inout % 16) == 0, "clip: the gradient array must be 16-B aligned");
    OCL_REQUIRE(((uintptr_t)workspace % 8) == 0, "clip: workspace must be 8-B aligned");
    OCL_REQUIRE(max_norm >= 0.f, "clip: max_norm=%g (must be >= 0 and not NaN)", (double)max_norm);
    const int blocks = clip_blocks(n);
    OCL_REQUIRE(workspace_doubles >= (int64_t)blocks, "clip: workspace of %lld doubles, %lld needed (ocl_clip_workspace_doubles)",
                (long long)workspace_doubles, (long long)blocks);
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_agem_project does)
    if (int arc = ocl::check_async_error("clip_grad_norm")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // the per-class profile has no class for flat-array passes: booked under BN, as ocl_agem_project is
    hipLaunchKernelGGL(clip_sumsq_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, s, (const float*)grads_inout, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(clip_apply_kernel, dim3(blocks), dim3(CLIP_THREADS), 0, s, grads_inout, n, max_norm, (const double*)workspace, blocks,
                       info4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
