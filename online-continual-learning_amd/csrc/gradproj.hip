// K8c: A-GEM's gradient projection (agents/agem.py:72-80 of the reference) on the flat gradient array, between backward and the
// optimiser step.  Two launches, ordered on the stream, no host synchronisation, no atomics, no grid-wide arrival:
//   agem_dots_kernel   per-block partial sums of g.g_ref and g_ref.g_ref, every product and every sum in double (a product of two
//                      floats is exact in double), wave reduction by shuffles and block reduction through LDS in a fixed order;
//   agem_apply_kernel  the first wave of every block adds the partial pairs in one fixed order (lane l takes pairs l, l + 64, ... in
//                      index order, then the shuffle tree: all blocks get the same two doubles), decides `prod < 0` and writes
//                      g - (prod / prod_ref) * g_ref, or a bit copy of g, over g_ref.
// HBM-bound fp32 streaming: 8 bytes per element read twice and 4 written.  IEEE '/' (the compiler's default): nothing in this file
// may be built with fast-math.
#include "flat_dev.h"

using namespace ocl;

__global__ void __launch_bounds__(FLAT_THREADS) agem_dots_kernel(const float* __restrict__ g, const float* __restrict__ r, int64_t n,
                                                                 double* __restrict__ partial) {
    double acc[2] = {0.0, 0.0};   // g.g_ref, g_ref.g_ref
    flat_for_each(n, [&](auto at) {
        const auto a = at.load(g), b = at.load(r);
#pragma unroll
        for (int k = 0; k < at.W; ++k) {
            const double bk = b[k];
            acc[0] += (double)a[k] * bk;
            acc[1] += bk * bk;
        }
    });
    flat_block_partial(acc, partial);
}

// `out` is g_ref itself: every element is read and then written by the same thread
__global__ void __launch_bounds__(FLAT_THREADS) agem_apply_kernel(const float* __restrict__ g, float* __restrict__ r, int64_t n,
                                                                  const double* __restrict__ partial, int nb, float* __restrict__ info4) {
    double tot[2];
    flat_grid_fold(partial, nb, tot);
    const double prod = tot[0], prod_ref = tot[1];
    const bool projected = prod < 0.0;   // false for NaN; prod_ref == 0 means g_ref == 0, so prod == 0: no division by zero below
    const float coef = projected ? (float)(prod / prod_ref) : 0.f;
    if (info4 != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        info4[0] = (float)prod;
        info4[1] = (float)prod_ref;
        info4[2] = coef;
        info4[3] = projected ? 1.f : 0.f;
    }
    if (!projected) {   // a bit copy: no arithmetic touches the values (a NaN keeps its payload)
        flat_for_each(n, [&](auto at) { at.store(r, at.load(g)); });
        return;
    }
    flat_for_each(n, [&](auto at) {
        const auto a = at.load(g);
        auto b = at.load(r);
#pragma unroll
        for (int k = 0; k < at.W; ++k) b[k] = fmaf(-coef, b[k], a[k]);
        at.store(r, b);
    });
}

int64_t ocl_agem_workspace_doubles(int64_t n) { return 2 * (int64_t)flat_reduce_blocks(n); }

int ocl_agem_project(const float* g, float* g_ref_inout, int64_t n, double* workspace, int64_t workspace_doubles, float* info4,
                     void* stream) {
    if (int rc = flat_check_args("agem", n, {{g, "g"}, {g_ref_inout, "g_ref"}})) return rc;
    OCL_REQUIRE(workspace != nullptr, "agem: null workspace");
    OCL_REQUIRE(((uintptr_t)workspace % 8) == 0, "agem: workspace must be 8-B aligned");
    const int blocks = flat_reduce_blocks(n);
    OCL_REQUIRE(workspace_doubles >= 2 * (int64_t)blocks, "agem: workspace of %lld doubles, %lld needed (ocl_agem_workspace_doubles)",
                (long long)workspace_doubles, (long long)(2 * (int64_t)blocks));
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_adam_step does)
    if (int arc = ocl::check_async_error("agem_project")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // the per-class profile has no class for flat-array passes: booked under BN, as ocl_adam_step is
    hipLaunchKernelGGL(agem_dots_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, g, (const float*)g_ref_inout, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(agem_apply_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, g, g_ref_inout, n, (const double*)workspace, blocks, info4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
