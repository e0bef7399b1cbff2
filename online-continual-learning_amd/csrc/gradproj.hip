// K8c: A-GEM's gradient projection (agents/agem.py:72-80 of the reference) on the flat gradient array, between backward and the
// optimiser step.  Two launches, ordered on the stream, no host synchronisation, no atomics, no grid-wide arrival:
//   agem_dots_kernel   per-block partial sums of g.g_ref and g_ref.g_ref, every product and every sum in double (a product of two
//                      floats is exact in double), wave reduction by shuffles and block reduction through LDS in a fixed order;
//   agem_apply_kernel  the first wave of every block adds the partial pairs in one fixed order (lane l takes pairs l, l + 64, ... in
//                      index order, then the shuffle tree: all blocks get the same two doubles), decides `prod < 0` and writes
//                      g - (prod / prod_ref) * g_ref, or a bit copy of g, over g_ref.
// HBM-bound fp32 streaming: 8 bytes per element read twice and 4 written.  IEEE '/' (the compiler's default): nothing in this file
// may be built with fast-math.
#include "common.h"

using namespace ocl;

static constexpr int AGEM_THREADS = 256;
static constexpr int AGEM_MAX_BLOCKS = 512;

// a function of n alone: the partial sums, and with them the result, do not depend on the device or on the launch
static inline int agem_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(AGEM_MAX_BLOCKS, ((n >> 2) + AGEM_THREADS - 1) / AGEM_THREADS));
}

__global__ void __launch_bounds__(AGEM_THREADS) agem_dots_kernel(const float* __restrict__ g, const float* __restrict__ r, int64_t n,
                                                                 double* __restrict__ partial) {
    __shared__ double red[2][AGEM_THREADS / 64];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const float4* g4 = (const float4*)g;
    const float4* r4 = (const float4*)r;
    double prod = 0.0, ref = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 a = g4[i], b = r4[i];
        const double bx = b.x, by = b.y, bz = b.z, bw = b.w;
        prod += (double)a.x * bx;
        prod += (double)a.y * by;
        prod += (double)a.z * bz;
        prod += (double)a.w * bw;
        ref += bx * bx;
        ref += by * by;
        ref += bz * bz;
        ref += bw * bw;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double b = r[i];
        prod += (double)g[i] * b;
        ref += b * b;
    }
    prod = wave_sum_d(prod);
    ref = wave_sum_d(ref);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wid] = prod;
        red[1][wid] = ref;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double p = red[0][0], q = red[1][0];
        for (int w = 1; w < AGEM_THREADS / 64; ++w) {
            p += red[0][w];
            q += red[1][w];
        }
        partial[2 * blockIdx.x] = p;
        partial[2 * blockIdx.x + 1] = q;
    }
}

// `out` is g_ref itself: every element is read and then written by the same thread
__global__ void __launch_bounds__(AGEM_THREADS) agem_apply_kernel(const float* __restrict__ g, float* __restrict__ r, int64_t n,
                                                                  const double* __restrict__ partial, int nb, float* __restrict__ info4) {
    __shared__ double tot[2];
    if (threadIdx.x < 64) {   // at most 8 dependent adds per lane and the shuffle tree, not nb adds on one thread while 255 wait
        double p = 0.0, q = 0.0;
        for (int b = threadIdx.x; b < nb; b += 64) {
            p += partial[2 * b];
            q += partial[2 * b + 1];
        }
        p = wave_sum_d(p);
        q = wave_sum_d(q);
        if (threadIdx.x == 0) {
            tot[0] = p;
            tot[1] = q;
        }
    }
    __syncthreads();
    const double prod = tot[0], prod_ref = tot[1];
    const bool projected = prod < 0.0;   // false for NaN; prod_ref == 0 means g_ref == 0, so prod == 0: no division by zero below
    const float coef = projected ? (float)(prod / prod_ref) : 0.f;
    if (info4 != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        info4[0] = (float)prod;
        info4[1] = (float)prod_ref;
        info4[2] = coef;
        info4[3] = projected ? 1.f : 0.f;
    }
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float4* g4 = (const float4*)g;
    float4* r4 = (float4*)r;
    if (!projected) {   // a bit copy: no arithmetic touches the values (a NaN keeps its payload)
        for (int64_t i = first; i < n4; i += stride) r4[i] = g4[i];
        for (int64_t i = (n4 << 2) + first; i < n; i += stride) r[i] = g[i];
        return;
    }
    for (int64_t i = first; i < n4; i += stride) {
        const float4 a = g4[i], b = r4[i];
        float4 o;
        o.x = fmaf(-coef, b.x, a.x);
        o.y = fmaf(-coef, b.y, a.y);
        o.z = fmaf(-coef, b.z, a.z);
        o.w = fmaf(-coef, b.w, a.w);
        r4[i] = o;
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) r[i] = fmaf(-coef, r[i], g[i]);
}

int64_t ocl_agem_workspace_doubles(int64_t n) { return 2 * (int64_t)agem_blocks(n); }

int ocl_agem_project(const float* g, float* g_ref_inout, int64_t n, double* workspace, int64_t workspace_doubles, float* info4,
                     void* stream) {
    OCL_REQUIRE(g && g_ref_inout && workspace, "agem: null pointer");
    OCL_REQUIRE(n > 0, "agem: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE((((uintptr_t)g | (uintptr_t)g_ref_inout) % 16) == 0, "agem: g and g_ref must be 16-B aligned");
    OCL_REQUIRE(((uintptr_t)workspace % 8) == 0, "agem: workspace must be 8-B aligned");
    OCL_REQUIRE(n <= (int64_t)(UINTPTR_MAX / 8), "agem: n=%lld is too large", (long long)n);
    {
        const uintptr_t a = (uintptr_t)g, b = (uintptr_t)g_ref_inout, bytes = (uintptr_t)n * 4;
        OCL_REQUIRE(a + bytes <= b || b + bytes <= a, "agem: g and g_ref overlap");
    }
    const int blocks = agem_blocks(n);
    OCL_REQUIRE(workspace_doubles >= 2 * (int64_t)blocks, "agem: workspace of %lld doubles, %lld needed (ocl_agem_workspace_doubles)",
                (long long)workspace_doubles, (long long)(2 * (int64_t)blocks));
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_adam_step does)
    if (int arc = ocl::check_async_error("agem_project")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // the per-class profile has no class for flat-array passes: booked under BN, as ocl_adam_step is
    hipLaunchKernelGGL(agem_dots_kernel, dim3(blocks), dim3(AGEM_THREADS), 0, s, g, (const float*)g_ref_inout, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(agem_apply_kernel, dim3(blocks), dim3(AGEM_THREADS), 0, s, g, g_ref_inout, n, (const double*)workspace, blocks, info4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
