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
#include "common.h"

#include <cmath>

using namespace ocl;

static constexpr int EWC_THREADS = 256;
static constexpr int EWC_MAX_BLOCKS = 512;

// a function of n alone: the partials, and with them the penalty, do not depend on the device or on the launch
static inline int ewc_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(EWC_MAX_BLOCKS, ((n >> 2) + EWC_THREADS - 1) / EWC_THREADS));
}

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
__global__ void __launch_bounds__(EWC_THREADS) ewc_accumulate_kernel(float* __restrict__ g, float* __restrict__ tmp, const float* __restrict__ p,
                                                                     const float* __restrict__ prev, const float* __restrict__ fh, int64_t n,
                                                                     float scale, double* __restrict__ partial) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* g4 = (float4*)g;
    float4* t4 = (float4*)tmp;
    const float4* p4 = (const float4*)p;
    const float4* q4 = (const float4*)prev;
    const float4* f4 = (const float4*)fh;
    double pen = 0.0;
    for (int64_t i = first; i < n4; i += stride) {
        float4 a = g4[i], t = t4[i];
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f), q = w, f = w;
        if (HAS_PREV && (PEN || WANT)) {
            w = p4[i];
            q = q4[i];
            f = f4[i];
        }
        ewc_elem<PEN, HAS_PREV && WANT>(a.x, t.x, w.x, q.x, f.x, scale, pen);
        ewc_elem<PEN, HAS_PREV && WANT>(a.y, t.y, w.y, q.y, f.y, scale, pen);
        ewc_elem<PEN, HAS_PREV && WANT>(a.z, t.z, w.z, q.z, f.z, scale, pen);
        ewc_elem<PEN, HAS_PREV && WANT>(a.w, t.w, w.w, q.w, f.w, scale, pen);
        if (PEN) g4[i] = a;
        t4[i] = t;
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) {
        float a = g[i], t = tmp[i], w = 0.f, q = 0.f, f = 0.f;
        if (HAS_PREV && (PEN || WANT)) {
            w = p[i];
            q = prev[i];
            f = fh[i];
        }
        ewc_elem<PEN, HAS_PREV && WANT>(a, t, w, q, f, scale, pen);
        if (PEN) g[i] = a;
        tmp[i] = t;
    }
    if (WANT) {
        __shared__ double red[EWC_THREADS / 64];
        pen = wave_sum_d(pen);
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        if (lane == 0) red[wid] = pen;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = red[0];
            for (int w = 1; w < EWC_THREADS / 64; ++w) s += red[w];
            partial[blockIdx.x] = s;
        }
    }
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

__global__ void __launch_bounds__(EWC_THREADS) ewc_fisher_ema_kernel(float* __restrict__ run, float* __restrict__ tmp, int64_t n, float keep,
                                                                     float gain) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4* r4 = (float4*)run;
    float4* t4 = (float4*)tmp;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = first; i < n4; i += stride) {
        float4 r = r4[i];
        const float4 t = t4[i];
        r.x = ewc_ema(r.x, t.x, keep, gain);
        r.y = ewc_ema(r.y, t.y, keep, gain);
        r.z = ewc_ema(r.z, t.z, keep, gain);
        r.w = ewc_ema(r.w, t.w, keep, gain);
        r4[i] = r;
        t4[i] = zero;
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) {
        run[i] = ewc_ema(run[i], tmp[i], keep, gain);
        tmp[i] = 0.f;
    }
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
__global__ void __launch_bounds__(EWC_THREADS) ewc_minmax_kernel(const float* __restrict__ run, int64_t n, float* __restrict__ partial) {
    __shared__ float lo_s[EWC_THREADS / 64], hi_s[EWC_THREADS / 64];
    __shared__ int nan_s[EWC_THREADS / 64];
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float4* r4 = (const float4*)run;
    MinMax m = {INFINITY, -INFINITY, 0};
    for (int64_t i = first; i < n4; i += stride) {
        const float4 r = r4[i];
        mm_take(m, r.x);
        mm_take(m, r.y);
        mm_take(m, r.z);
        mm_take(m, r.w);
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) mm_take(m, run[i]);
    m = mm_wave(m);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        lo_s[wid] = m.lo;
        hi_s[wid] = m.hi;
        nan_s[wid] = m.nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EWC_THREADS / 64; ++w) {
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
__global__ void __launch_bounds__(EWC_THREADS) ewc_normalize_kernel(const float* __restrict__ run, float* __restrict__ out, int64_t n,
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
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float4* r4 = (const float4*)run;
    float4* o4 = (float4*)out;
    for (int64_t i = first; i < n4; i += stride) {
        const float4 r = r4[i];
        float4 o;
        o.x = __fdiv_rn(__fsub_rn(r.x, lo), den);
        o.y = __fdiv_rn(__fsub_rn(r.y, lo), den);
        o.z = __fdiv_rn(__fsub_rn(r.z, lo), den);
        o.w = __fdiv_rn(__fsub_rn(r.w, lo), den);
        o4[i] = o;
    }
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) out[i] = __fdiv_rn(__fsub_rn(run[i], lo), den);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------

static inline bool ewc_disjoint(const void* a, const void* b, uintptr_t bytes_a, uintptr_t bytes_b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + bytes_a <= y || y + bytes_b <= x;
}

// the doubles of workspace the accumulate step needs (one per block), rounded up to a whole number of 16-byte pairs; the same
// workspace read as floats holds the normalisation's min / max pair per block
int64_t ocl_ewc_workspace_doubles(int64_t n) { return ((int64_t)ewc_blocks(n) + 1) / 2 * 2; }

int ocl_ewc_accumulate(float* grads_inout, float* tmp_fisher_inout, const float* params, const float* prev_params, const float* fisher_hat,
                       int64_t n, float scale, double* workspace, int64_t workspace_doubles, float* penalty_out, void* stream) {
    OCL_REQUIRE(grads_inout && tmp_fisher_inout && params, "ewc: null pointer (grads, tmp_fisher or params)");
    OCL_REQUIRE((prev_params == nullptr) == (fisher_hat == nullptr), "ewc: prev_params and fisher_hat are given together or not at all");
    OCL_REQUIRE(n > 0, "ewc: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE(n <= (int64_t)(UINTPTR_MAX / 8), "ewc: n=%lld is too large", (long long)n);
    const bool has_prev = prev_params != nullptr;
    const void* arr[5] = {grads_inout, tmp_fisher_inout, params, prev_params, fisher_hat};
    static const char* const name[5] = {"grads", "tmp_fisher", "params", "prev_params", "fisher_hat"};
    const int n_arr = has_prev ? 5 : 3;
    const uintptr_t bytes = (uintptr_t)n * 4;
    for (int i = 0; i < n_arr; ++i) OCL_REQUIRE(((uintptr_t)arr[i] % 16) == 0, "ewc: %s must be 16-B aligned", name[i]);
    for (int i = 0; i < n_arr; ++i)
        for (int j = i + 1; j < n_arr; ++j) OCL_REQUIRE(ewc_disjoint(arr[i], arr[j], bytes, bytes), "ewc: %s and %s overlap", name[i], name[j]);
    const int blocks = ewc_blocks(n);
    if (penalty_out != nullptr) {
        OCL_REQUIRE(workspace != nullptr, "ewc: null workspace (needed with penalty_out)");
        OCL_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)penalty_out % 4) == 0, "ewc: workspace must be 8-B aligned, penalty_out 4-B");
        OCL_REQUIRE(workspace_doubles >= (int64_t)blocks, "ewc: workspace of %lld doubles, %lld needed (ocl_ewc_workspace_doubles)",
                    (long long)workspace_doubles, (long long)ocl_ewc_workspace_doubles(n));
        for (int i = 0; i < n_arr; ++i) {
            OCL_REQUIRE(ewc_disjoint(arr[i], workspace, bytes, (uintptr_t)blocks * 8), "ewc: %s and the workspace overlap", name[i]);
            OCL_REQUIRE(ewc_disjoint(arr[i], penalty_out, bytes, 4), "ewc: %s and penalty_out overlap", name[i]);
        }
    }
    // a backward whose one-pass BatchNorm timed out has poisoned the gradients with NaN: refuse (as ocl_agem_project does)
    if (int arc = ocl::check_async_error("ewc_accumulate")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);   // flat-array passes are booked under BN, as ocl_adam_step and ocl_agem_project are
    // scale == 0 adds nothing: g is then not rewritten at all (g + 0 * f * d would turn a -0 into +0, and an infinite d into NaN)
    const bool pen = has_prev && scale != 0.f;
    const dim3 grid(blocks), block(EWC_THREADS);
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
    OCL_REQUIRE(running_inout && tmp_inout, "ewc: null pointer (running_fisher or tmp_fisher)");
    OCL_REQUIRE(n > 0, "ewc: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE(n <= (int64_t)(UINTPTR_MAX / 8), "ewc: n=%lld is too large", (long long)n);
    OCL_REQUIRE((((uintptr_t)running_inout | (uintptr_t)tmp_inout) % 16) == 0, "ewc: running_fisher and tmp_fisher must be 16-B aligned");
    OCL_REQUIRE(ewc_disjoint(running_inout, tmp_inout, (uintptr_t)n * 4, (uintptr_t)n * 4), "ewc: running_fisher and tmp_fisher overlap");
    if (int arc = ocl::check_async_error("ewc_fisher_ema")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(ewc_fisher_ema_kernel, dim3(ewc_blocks(n)), dim3(EWC_THREADS), 0, s, running_inout, tmp_inout, n, keep, gain);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_ewc_fisher_normalize(const float* running, float* fisher_hat_out, int64_t n, float* workspace, int64_t workspace_floats,
                             float* minmax_out2, void* stream) {
    OCL_REQUIRE(running && fisher_hat_out && workspace, "ewc: null pointer (running_fisher, fisher_hat or workspace)");
    OCL_REQUIRE(n > 0, "ewc: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE(n <= (int64_t)(UINTPTR_MAX / 8), "ewc: n=%lld is too large", (long long)n);
    OCL_REQUIRE((((uintptr_t)running | (uintptr_t)fisher_hat_out) % 16) == 0, "ewc: running_fisher and fisher_hat must be 16-B aligned");
    OCL_REQUIRE(((uintptr_t)workspace % 4) == 0 && ((uintptr_t)minmax_out2 % 4) == 0, "ewc: workspace and minmax_out must be 4-B aligned");
    const int blocks = ewc_blocks(n);
    const uintptr_t bytes = (uintptr_t)n * 4;
    OCL_REQUIRE(workspace_floats >= 2 * (int64_t)blocks, "ewc: workspace of %lld floats, %lld needed (2 * ocl_ewc_workspace_doubles)",
                (long long)workspace_floats, (long long)(2 * ocl_ewc_workspace_doubles(n)));
    OCL_REQUIRE(ewc_disjoint(running, fisher_hat_out, bytes, bytes), "ewc: running_fisher and fisher_hat overlap");
    OCL_REQUIRE(ewc_disjoint(running, workspace, bytes, (uintptr_t)blocks * 8) && ewc_disjoint(fisher_hat_out, workspace, bytes, (uintptr_t)blocks * 8),
                "ewc: an array and the workspace overlap");
    if (minmax_out2 != nullptr)
        OCL_REQUIRE(ewc_disjoint(running, minmax_out2, bytes, 8) && ewc_disjoint(fisher_hat_out, minmax_out2, bytes, 8),
                    "ewc: an array and minmax_out overlap");
    if (int arc = ocl::check_async_error("ewc_fisher_normalize")) return arc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(ewc_minmax_kernel, dim3(blocks), dim3(EWC_THREADS), 0, s, running, n, workspace);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ewc_normalize_kernel, dim3(blocks), dim3(EWC_THREADS), 0, s, running, fisher_hat_out, n, (const float*)workspace, blocks,
                       minmax_out2);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
