// K8 / K8b: the two optimisers over the flat parameter array, one flat_dev.h kernel each.
// K8: torch.optim.SGD (weight decay, no momentum): 16-byte loads of p and g, one store, 12 bytes per element.
// K8b: torch.optim.Adam over the flat parameter array as one kernel.  HBM-bound fp32 streaming like sgd_flat: four
// 16-byte loads (p, g, m, v) and three stores (p, m, v) per four elements, 28 bytes per element; no LDS, no atomics, no reduction.
// IEEE sqrtf and '/' (the compiler's default): nothing in this file may be built with fast-math or replaced by an approximation.
#include "flat_dev.h"
#include "small_ops.h"
#include <math.h>

using namespace ocl;

// =====================================================================================================
// K8 SGD (flat)
// =====================================================================================================
namespace ocl {
SPlan plan_sgd(const void* params, const void* grads, const void* out, int64_t n) {
    if (!aligned16(params, grads, out)) return splan(OCL_PATH_SGD_REFUSED);
    const int blocks = (int)min((int64_t)2048, (n / 4 + 255) / 256 + 1);
    const bool more_trips = n / 4 > (int64_t)blocks * 256;
    return splan(more_trips ? OCL_PATH_SGD_GRID_CAP : (n % 4) ? OCL_PATH_SGD_TAIL : OCL_PATH_SGD_VEC, (unsigned)blocks, 1, 256);
}
}  // namespace ocl

__global__ void __launch_bounds__(256) sgd_flat(float* __restrict__ p, const float* __restrict__ g, int64_t n, float lr,
                                                float wd, float gs, float* __restrict__ out) {
    float* o = out ? out : p;
    flat_for_each(n, [&](auto at) {
        auto a = at.load(p);
        const auto b = at.load(g);
#pragma unroll
        for (int k = 0; k < at.W; ++k) a[k] = fmaf(-lr, fmaf(wd, a[k], b[k] * gs), a[k]);
        at.store(o, a);
    });
}

int ocl_sgd_step(float* params, const float* grads, int64_t n, float lr, float weight_decay, float grad_scale, float* out,
                 void* stream) {
    OCL_REQUIRE(params && grads && n > 0, "sgd: null pointer or n<=0");
    // a backward whose one-pass BatchNorm timed out has poisoned `grads` with NaN: refuse the step instead of applying it (the word
    // is read without synchronising; a time-out that lands after this check is caught by the next forward, before its step)
    if (int arc = ocl::check_async_error("sgd_step")) return arc;
    const SPlan pl = plan_sgd(params, grads, out, n);
    OCL_REQUIRE(pl.path != OCL_PATH_SGD_REFUSED, "sgd: pointers must be 16-B aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(sgd_flat, dim3(pl.grid_x), dim3(pl.block), 0, s, params, grads, n, lr, weight_decay, grad_scale, out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// =====================================================================================================
// K8b Adam (flat)
// =====================================================================================================
// the constants of one step, formed in double on the host (ocl_adam_step) and passed by value
struct AdamStep {
    float omb1, beta2, omb2;   // 1 - beta1, beta2, 1 - beta2
    float eps, wd, gs;
    float step_size, bc2_sqrt;   // lr / (1 - beta1^t), sqrt(1 - beta2^t)
};

// torch's _single_tensor_adam (amsgrad off, maximize off, L2 weight decay added to the gradient), one element
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamStep& c) {
    const float gp = fmaf(c.wd, p, g * c.gs);          // grad.add(param, alpha = wd); wd == 0: g * gs exactly
    m = fmaf(c.omb1, gp - m, m);                       // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(c.omb2 * gp, gp, c.beta2 * v);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float den = sqrtf(v) / c.bc2_sqrt + c.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = fmaf(-c.step_size, m / den, p);                // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// elements [skip_begin, skip_end) keep p, m and v (parameters that never get a gradient: torch skips a tensor whose .grad is None)
__global__ void __launch_bounds__(FLAT_THREADS) adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, AdamStep c, int64_t skip_begin, int64_t skip_end) {
    flat_for_each(n, [&](auto at) {
        constexpr int W = decltype(at)::W;
        const int64_t e = at.e;
        if (e >= skip_begin && e + W <= skip_end) return;   // wholly inside the range: neither read nor written
        const auto po = at.load(p), b = at.load(g), mo = at.load(m), vo = at.load(v);
        auto pn = po, mn = mo, vn = vo;
#pragma unroll
        for (int k = 0; k < W; ++k) adam_one(pn[k], b[k], mn[k], vn[k], c);
        if (e + W - 1 >= skip_begin && e < skip_end) {   // a boundary of the range falls into this vector: per-element choice
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const bool skip = e + k >= skip_begin && e + k < skip_end;
                pn[k] = skip ? po[k] : pn[k];
                mn[k] = skip ? mo[k] : mn[k];
                vn[k] = skip ? vo[k] : vn[k];
            }
        }
        at.store(p, pn);
        at.store(m, mn);
        at.store(v, vn);
    });
}

int ocl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int64_t step, int64_t skip_begin, int64_t skip_end, void* stream) {
    if (int rc = flat_check_args("adam", n, {{params, "params"}, {grads, "grads"}, {exp_avg, "exp_avg"}, {exp_avg_sq, "exp_avg_sq"}})) return rc;
    OCL_REQUIRE(step >= 1, "adam: step=%lld (1-based)", (long long)step);
    OCL_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "adam: betas (%g, %g) outside [0, 1)", beta1, beta2);
    OCL_REQUIRE(eps >= 0.f, "adam: eps=%g (must be >= 0)", eps);
    OCL_REQUIRE(0 <= skip_begin && skip_begin <= skip_end && skip_end <= n, "adam: skip range [%lld, %lld) outside [0, %lld]",
                (long long)skip_begin, (long long)skip_end, (long long)n);
    // a backward whose one-pass BatchNorm timed out has poisoned `grads` with NaN: refuse the step (as ocl_sgd_step does)
    if (int arc = ocl::check_async_error("adam_step")) return arc;
    // torch's non-capturable path: the bias corrections in double on the host, from the float values the caller passed
    const double b1 = beta1, b2 = beta2;
    AdamStep c;
    c.omb1 = (float)(1.0 - b1);
    c.beta2 = beta2;
    c.omb2 = (float)(1.0 - b2);
    c.eps = eps;
    c.wd = weight_decay;
    c.gs = grad_scale;
    c.step_size = (float)((double)lr / (1.0 - pow(b1, (double)step)));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(b2, (double)step));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, ((n >> 2) + FLAT_THREADS - 1) / FLAT_THREADS));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks), dim3(FLAT_THREADS), 0, s, params, grads, exp_avg, exp_avg_sq, n, c, skip_begin, skip_end);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
