// K8d: EWC++'s bookkeeping (agents/ewc_pp.py of the reference) on the flat parameter and gradient arrays.  Three entry points, all
// ordered on the stream, no host synchronisation, no atomics, no grid-wide arrival:
//   ocl_ewc_accumulate        once per step, between backward and the optimiser step (:83-92 and :104-106): the penalty's gradient
//                             added to the batch gradient and the square of the sum added to the temporary Fisher, one launch; with
//                             penalty_out, per-block double partials of sum f*d*d and a one-block launch that adds them in index order;
//   ocl_ewc_fisher_ema        every fisher_update_after steps (:97-102): running = keep*running + gain*tmp, tmp = 0, one launch,
//                             separately rounded products and sum (what torch's three float32 passes compute);
//   ocl_ewc_fisher_normalize  at a task's end (:76-80): per-block min / max partials, then every block reduces the partials again (min
//                             and max do not depend on the order) and writes (r - min) / (max - min + 1e-32f).
// HBM-bound fp32 streaming: the accumulate reads five arrays and writes two, 28 bytes per element.  IEEE '/' and no reassociation:
// nothing in this file may be built with fast-math.
#include "flat_dev.h"

#include <cmath>

using namespace ocl;

// one element of the accumulate step.  PEN: the penalty's gradient is added (prev and fisher_hat given and scale != 0); without it g
// is not written at all.  d in float for the gradient (the reference's p - prev), in double (exact) for the penalty's value.
template <bool PEN, bool WANT>
__device__ __forceinline__ void ewc_elem(float& g, float& t, float p, float pp, float f, float scale, double& pen) {
    if (PEN) {
        const float d = p - pp;
        g = g + (scale * f) * d;
    }
    t = t + g * g;
    if (WANT) {
        const double dd = (double)p - (double)pp;
        pen += (double)f * dd * dd;
    }
}

// HAS_PREV: prev and fisher_hat are read.  PEN implies HAS_PREV; WANT without HAS_PREV writes zero partials (the penalty of the first task).
template <bool HAS_PREV, bool PEN, bool WANT>
__global__ void __launch_bounds__(FLAT_THREADS) ewc_accumulate_kernel(float* __restrict__ g, float* __restrict__ tmp, const float* __restrict__ p,
                                                                     const float* __restrict__ prev, const float* __restrict__ fh, int64_t n,
                                                                     float scale, double* __restrict__ partial) {
    double pen[1] = {0.0};
    flat_for_each(n, [&](auto at) {
        constexpr int W = decltype(at)::W;
        auto a = at.load(g), t = at.load(tmp);
        FlatVals<W> w = {}, q = {}, f = {};
        if constexpr (HAS_PREV && (PEN || WANT)) {
            w = at.load(p);
            q = at.load(prev);
            f = at.load(fh);
        }
#pragma unroll
        for (int k = 0; k < W; ++k) ewc_elem<PEN, HAS_PREV && WANT>(a[k], t[k], w[k], q[k], f[k], scale, pen[0]);
        if constexpr (PEN) at.store(g, a);
        at.store(tmp, t);
    });
    if constexpr (WANT) flat_block_partial(pen, partial);
}

// one block of one wave; thread 0 adds the partials in index order
__global__ void __launch_bounds__(64) ewc_penalty_kernel(const double* __restrict__ partial, int nb, float* __restrict__ out) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += partial[b];
        out[0] = (float)s;
    }
}

// three roundings, no fma.  __fmul_rn / __fadd_rn are plain '*' and '+' in this HIP, and the back end fuses a product it can see into
// the sum that uses it (fp-contract=fast is the compiler's default, and a contract(off) pragma did not stop the packed form): each
// product passes through an empty asm statement, which the combiner cannot look through.
__device__ __forceinline__ float ewc_ema(float r, float t, float keep, float gain) {
    float a = __fmul_rn(keep, r);
    float b = __fmul_rn(gain, t);
    asm volatile("" : "+v"(a), "+v"(b));
    return __fadd_rn(a, b);
}

__global__ void __launch_bounds__(FLAT_THREADS) ewc_fisher_ema_kernel(float* __restrict__ run, float* __restrict__ tmp, int64_t n, float keep,
                                                                     float gain) {
    flat_for_each(n, [&](auto at) {
        constexpr int W = decltype(at)::W;
        auto r = at.load(run);
        const auto t = at.load(tmp);
#pragma unroll
        for (int k = 0; k < W; ++k) r[k] = ewc_ema(r[k], t[k], keep, gain);
        at.store(run, r);
        at.store(tmp, FlatVals<W>{});
    });
}

// min and max that keep a NaN (fminf / fmaxf drop it): the flag travels beside the two values
struct MinMax {
    float lo, hi;
    int nan;
};
__device__ __forceinline__ void mm_take(MinMax& m, float v) {
    m.lo = fminf(m.lo, v);
    m.hi = fmaxf(m.hi, v);
    m.nan |= (v != v);
}
__device__ __forceinline__ MinMax mm_wave(MinMax m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m.lo = fminf(m.lo, __shfl_xor(m.lo, o, 64));
        m.hi = fmaxf(m.hi, __shfl_xor(m.hi, o, 64));
        m.nan |= __shfl_xor(m.nan, o, 64);
    }
    return m;
}

// partial[2b], partial[2b + 1]: block b's min and max, both NaN where the block saw one
__global__ void __launch_bounds__(FLAT_THREADS) ewc_minmax_kernel(const float* __restrict__ run, int64_t n, float* __restrict__ partial) {
    __shared__ float lo_s[FLAT_THREADS / 64], hi_s[FLAT_THREADS / 64];
    __shared__ int nan_s[FLAT_THREADS / 64];
    MinMax m = {INFINITY, -INFINITY, 0};
    flat_for_each(n, [&](auto at) {
        const auto r = at.load(run);
#pragma unroll
        for (int k = 0; k < at.W; ++k) mm_take(m, r[k]);
    });
    m = mm_wave(m);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        lo_s[wid] = m.lo;
        hi_s[wid] = m.hi;
        nan_s[wid] = m.nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FLAT_THREADS / 64; ++w) {
            m.lo = fminf(m.lo, lo_s[w]);
            m.hi = fmaxf(m.hi, hi_s[w]);
            m.nan |= nan_s[w];
        }
        partial[2 * blockIdx.x] = m.nan ? NAN : m.lo;
        partial[2 * blockIdx.x + 1] = m.nan ? NAN : m.hi;
    }
}

// (a block that holds no element -- more blocks than float4 groups happens only for n < 4, where there is one block -- would write
// +inf / -inf partials, which min and max ignore)
__global__ void __launch_bounds__(FLAT_THREADS) ewc_normalize_kernel(const float* __restrict__ run, float* __restrict__ out, int64_t n,
                                                                    const float* __restrict__ partial, int nb, float* __restrict__ minmax2) {
    __shared__ float tot[2];
    if (threadIdx.x < 64) {
        MinMax m = {INFINITY, -INFINITY, 0};
        for (int b = threadIdx.x; b < nb; b += 64) {
            mm_take(m, partial[2 * b]);
            m.hi = fmaxf(m.hi, partial[2 * b + 1]);
        }
        m = mm_wave(m);
        if (threadIdx.x == 0) {
            tot[0] = m.nan ? NAN : m.lo;
            tot[1] = m.nan ? NAN : m.hi;
        }
    }
    __syncthreads();
    const float lo = tot[0], hi = tot[1];
    if (minmax2 != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        minmax2[0] = lo;
        minmax2[1] = hi;
    }
    const float den = __fadd_rn(__fsub_rn(hi, lo), 1e-32f);
    flat_for_each(n, [&](auto at) {
        auto r = at.load(run);
#pragma unroll
        for (int k = 0; k < at.W; ++k) r[k] = __fdiv_rn(__fsub_rn(r[k], lo), den);
        at.store(out, r);
    });
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------

// the doubles of workspace the accumulate step needs (one per block), rounded up to a whole number of 16-byte pairs; the same
// workspace read as floats holds the normalisation's min / max pair per block
int64_t ocl_ewc_workspace_doubles(int64_t n) { return ((int64_t)flat_reduce_blocks(n) + 1) / 2 * 2; }

int ocl_ewc_accumulate(float* grads_inout, float* tmp_fisher_inout, const float* params, const float* prev_params, const float* fisher_hat,
                       int64_t n, float scale, double* workspace, int64_t workspace_doubles, float* penalty_out, void* stream) {
    OCL_REQUIRE((prev_params == nullptr) == (fisher_hat == nullptr), "ewc: prev_params and fisher_hat are given together or not at all");
    const bool has_prev = prev_params != nullptr;
    const FlatArg arr[5] = {{grads_inout, "grads"}, {tmp_fisher_inout, "tmp_fisher"}, {params, "params"}, {prev_params, "prev_params"},
                            {fisher_hat, "fisher_hat"}};
    const int n_arr = has_prev ? 5 : 3;
    if (int rc = flat_check_args("ewc", n, arr, n_arr)) return rc;
    const size_t bytes = (size_t)n * 4;
    const int blocks = flat_reduce_blocks(n);
    if (penalty_out != nullptr) {
        OCL_REQUIRE(workspace != nullptr, "ewc: null workspace (needed with penalty_out)");
        OCL_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)penalty_out % 4) == 0, "ewc: workspace must be 8-B aligned, penalty_out 4-B");
        OCL_REQUIRE(workspace_doubles >= (int64_t)blocks, "ewc: workspace of %lld doubles, %lld needed (ocl_ewc_workspace_doubles)",
                    (long long)workspace_doubles, (long long)ocl_ewc_workspace_doubles(n));
        for (int i = 0; i < n_arr; ++i) {
            OCL_REQUIRE(!ranges_overlap(arr[i].ptr, bytes, workspace, (size_t)blocks * 8), "ewc: %s and the workspace overlap", arr[i].name);
            OCL_REQUIRE(!ranges_overlap(arr[i].ptr, bytes, penalty_out, 4), "ewc: %s and penalty_out overlap", arr[i].name);
        }
    }
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_agem_project does)
    if (int arc = ocl::check_async_error("ewc_accumulate")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // flat-array passes are booked under BN, as ocl_adam_step and ocl_agem_project are
    // scale == 0 adds nothing: g is then not rewritten at all (g + 0 * f * d would turn a -0 into +0, and an infinite d into NaN)
    const bool pen = has_prev && scale != 0.f;
    const dim3 grid(blocks), block(FLAT_THREADS);
#define EWC_LAUNCH(HP, PEN, WANT)                                                                                                          \
    hipLaunchKernelGGL((ewc_accumulate_kernel<HP, PEN, WANT>), grid, block, 0, s, grads_inout, tmp_fisher_inout, params, prev_params, \
                       fisher_hat, n, scale, workspace)
    if (penalty_out != nullptr) {
        if (pen) EWC_LAUNCH(true, true, true);
        else if (has_prev) EWC_LAUNCH(true, false, true);
        else EWC_LAUNCH(false, false, true);
    } else {
        if (pen) EWC_LAUNCH(true, true, false);
        else EWC_LAUNCH(false, false, false);
    }
#undef EWC_LAUNCH
    OCL_LAUNCH_CHECK();
    if (penalty_out != nullptr) {
        hipLaunchKernelGGL(ewc_penalty_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, penalty_out);
        OCL_LAUNCH_CHECK();
    }
    return OCL_OK;
}

int ocl_ewc_fisher_ema(float* running_inout, float* tmp_inout, int64_t n, float keep, float gain, void* stream) {
    if (int rc = flat_check_args("ewc", n, {{running_inout, "running_fisher"}, {tmp_inout, "tmp_fisher"}})) return rc;
    if (int arc = ocl::check_async_error("ewc_fisher_ema")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(ewc_fisher_ema_kernel, dim3(flat_reduce_blocks(n)), dim3(FLAT_THREADS), 0, s, running_inout, tmp_inout, n, keep, gain);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_ewc_fisher_normalize(const float* running, float* fisher_hat_out, int64_t n, float* workspace, int64_t workspace_floats,
                             float* minmax_out2, void* stream) {
    if (int rc = flat_check_args("ewc", n, {{running, "running_fisher"}, {fisher_hat_out, "fisher_hat"}})) return rc;
    OCL_REQUIRE(workspace != nullptr, "ewc: null workspace");
    OCL_REQUIRE(((uintptr_t)workspace % 4) == 0 && ((uintptr_t)minmax_out2 % 4) == 0, "ewc: workspace and minmax_out must be 4-B aligned");
    const int blocks = flat_reduce_blocks(n);
    const size_t bytes = (size_t)n * 4, ws_bytes = (size_t)blocks * 8;
    OCL_REQUIRE(workspace_floats >= 2 * (int64_t)blocks, "ewc: workspace of %lld floats, %lld needed (2 * ocl_ewc_workspace_doubles)",
                (long long)workspace_floats, (long long)(2 * ocl_ewc_workspace_doubles(n)));
    OCL_REQUIRE(!ranges_overlap(running, bytes, workspace, ws_bytes) && !ranges_overlap(fisher_hat_out, bytes, workspace, ws_bytes),
                "ewc: an array and the workspace overlap");
    if (minmax_out2 != nullptr)
        OCL_REQUIRE(!ranges_overlap(running, bytes, minmax_out2, 8) && !ranges_overlap(fisher_hat_out, bytes, minmax_out2, 8),
                    "ewc: an array and minmax_out overlap");
    if (int arc = ocl::check_async_error("ewc_fisher_normalize")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(ewc_minmax_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, running, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ewc_normalize_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, running, fisher_hat_out, n, (const float*)workspace, blocks,
                       minmax_out2);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
