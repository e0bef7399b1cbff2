// K8b: torch.optim.Adam over the flat parameter array as one kernel.  HBM-bound fp32 streaming like sgd_flat (small_ops.hip): four
// 16-byte loads (p, g, m, v) and three stores (p, m, v) per four elements, 28 bytes per element; no LDS, no atomics, no reduction.
// IEEE sqrtf and '/' (the compiler's default): nothing in this file may be built with fast-math or replaced by an approximation.
#include "common.h"
#include <math.h>

using namespace ocl;

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
__global__ void __launch_bounds__(256) adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n, AdamStep c, int64_t skip_begin, int64_t skip_end) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* p4 = (float4*)p;
    const float4* g4 = (const float4*)g;
    float4* m4 = (float4*)m;
    float4* v4 = (float4*)v;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const int64_t e = i << 2;
        if (e >= skip_begin && e + 4 <= skip_end) continue;   // wholly inside the range: neither read nor written
        const float4 a = p4[i], b = g4[i], mo = m4[i], vo = v4[i];
        float4 pn = a, mn = mo, vn = vo;
        adam_one(pn.x, b.x, mn.x, vn.x, c);
        adam_one(pn.y, b.y, mn.y, vn.y, c);
        adam_one(pn.z, b.z, mn.z, vn.z, c);
        adam_one(pn.w, b.w, mn.w, vn.w, c);
        if (e + 3 >= skip_begin && e < skip_end) {   // a boundary of the range falls into this vector: per-element choice
            const bool s0 = e >= skip_begin && e < skip_end, s1 = e + 1 >= skip_begin && e + 1 < skip_end;
            const bool s2 = e + 2 >= skip_begin && e + 2 < skip_end, s3 = e + 3 >= skip_begin && e + 3 < skip_end;
            pn.x = s0 ? a.x : pn.x; mn.x = s0 ? mo.x : mn.x; vn.x = s0 ? vo.x : vn.x;
            pn.y = s1 ? a.y : pn.y; mn.y = s1 ? mo.y : mn.y; vn.y = s1 ? vo.y : vn.y;
            pn.z = s2 ? a.z : pn.z; mn.z = s2 ? mo.z : mn.z; vn.z = s2 ? vo.z : vn.z;
            pn.w = s3 ? a.w : pn.w; mn.w = s3 ? mo.w : mn.w; vn.w = s3 ? vo.w : vn.w;
        }
        p4[i] = pn;
        m4[i] = mn;
        v4[i] = vn;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (i >= skip_begin && i < skip_end) continue;
        float pn = p[i], mn = m[i], vn = v[i];
        adam_one(pn, g[i], mn, vn, c);
        p[i] = pn;
        m[i] = mn;
        v[i] = vn;
    }
}

int ocl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int64_t step, int64_t skip_begin, int64_t skip_end, void* stream) {
    OCL_REQUIRE(params && grads && exp_avg && exp_avg_sq, "adam: null pointer");
    OCL_REQUIRE(n > 0, "adam: n=%lld (must be > 0)", (long long)n);
    OCL_REQUIRE((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16) == 0,
                "adam: pointers must be 16-B aligned");
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
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, ((n >> 2) + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n, c, skip_begin, skip_end);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
