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
#include "flat_dev.h"

using namespace ocl;

__global__ void __launch_bounds__(FLAT_THREADS) clip_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
    double acc[1] = {0.0};
    flat_for_each(n, [&](auto at) {
        const auto a = at.load(g);
#pragma unroll
        for (int k = 0; k < at.W; ++k) {
            const double ak = a[k];
            acc[0] += ak * ak;
        }
    });
    flat_block_partial(acc, partial);
}

// every element is read and then written by the same thread
__global__ void __launch_bounds__(FLAT_THREADS) clip_apply_kernel(float* __restrict__ g, int64_t n, float max_norm,
                                                                  const double* __restrict__ partial, int nb, float* __restrict__ info4) {
    double tot[1];
    flat_grid_fold(partial, nb, tot);
    const double sumsq = tot[0];
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
    flat_for_each(n, [&](auto at) {
        auto a = at.load(g);
#pragma unroll
        for (int k = 0; k < at.W; ++k) a[k] *= coef;
        at.store(g, a);
    });
}

int64_t ocl_clip_workspace_doubles(int64_t n) { return (int64_t)flat_reduce_blocks(n); }

int ocl_clip_grad_norm(float* grads_inout, int64_t n, float max_norm, double* workspace, int64_t workspace_doubles, float* info4,
                       void* stream) {
    if (int rc = flat_check_args("clip", n, {{grads_inout, "the gradient array"}})) return rc;
    OCL_REQUIRE(workspace != nullptr, "clip: null workspace");
    OCL_REQUIRE(((uintptr_t)workspace % 8) == 0, "clip: workspace must be 8-B aligned");
    OCL_REQUIRE(max_norm >= 0.f, "clip: max_norm=%g (must be >= 0 and not NaN)", (double)max_norm);
    const int blocks = flat_reduce_blocks(n);
    OCL_REQUIRE(workspace_doubles >= (int64_t)blocks, "clip: workspace of %lld doubles, %lld needed (ocl_clip_workspace_doubles)",
                (long long)workspace_doubles, (long long)blocks);
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_agem_project does)
    if (int arc = ocl::check_async_error("clip_grad_norm")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // the per-class profile has no class for flat-array passes: booked under BN, as ocl_agem_project is
    hipLaunchKernelGGL(clip_sumsq_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, (const float*)grads_inout, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(clip_apply_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, grads_inout, n, max_norm, (const double*)workspace, blocks,
                       info4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
