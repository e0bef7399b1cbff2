// K6b: Learning without Forgetting's loss (agents/lwf.py:36-39 of the reference) -- the cross-entropy of the student's logits
// (agents/base.py:113) blended with the distillation loss against the teacher's (utils/kd_manager.py:6-11) -- and its gradient with
// respect to the student's logits, in ONE launch:
//   ce   = mean_r( lse(s_r) - s_r[y_r] )
//   kd   = mean_r( -sum_j softmax(t_r / T)_j * log_softmax(s_r / T)_j ) * T^2
//   loss_out = { w_new * ce + w_old * kd, ce, kd }
//   dlogits[r][j] = w_new * (softmax(s_r)_j - [j == y_r]) / n + w_old * (softmax(s_r / T)_j - softmax(t_r / T)_j) * T / n
// The shape of the CE family (small_ops.hip): a single workgroup of four waves, one wave per row, reductions by wave shuffles, the
// per-wave partial sums through LDS and added in index order -- no atomics, a fixed order of summation, two runs give the same bits.
// The row arithmetic is that of ce_row and of kd_kernel, restated statement by statement: without a teacher (LwF's first task) and
// with w_new == 1 the cross-entropy and its gradient are ocl_ce_fwd_bwd's bits.
//
// A row of up to BLEND_REG * 64 logits is read from memory once and kept in registers (lane l holds columns l, l + 64, ...: the
// elements the strided loops of ce_row give that lane, in the same order); a longer row takes the strided loops themselves.
// x / T is a true division, as in kd_kernel (whose comment has the numbers): a multiplication by the rounded 1 / T moves the logit
// by up to |x| / T * 2^-24 for a T that is no power of two.  Nothing in this file may be built with fast-math.
#include <cmath>

#include "common.h"

using namespace ocl;

static constexpr int BLEND_REG = 4;   // registers per lane and per operand: rows of up to 256 columns stay in registers

// One row, by one wave.  REG: the row and the teacher's sit in sv / tv; otherwise every pass reads s / t again.  KD: a teacher is
// present.  Returns the row's cross-entropy; *kd_row receives the row's distillation term (before the mean and T^2).
template <bool REG, bool KD>
__device__ __forceinline__ float blend_row(const float* __restrict__ s, const float* __restrict__ t, int c, int64_t y, int lane, float T,
                                           float scale_new, float w_old, float n_f, float* __restrict__ dx, float* __restrict__ kd_row) {
    float sv[BLEND_REG], tv[BLEND_REG];
    if (REG) {
#pragma unroll
        for (int k = 0; k < BLEND_REG; ++k) {
            const int j = lane + 64 * k;
            sv[k] = j < c ? s[j] : 0.f;
            tv[k] = (KD && j < c) ? t[j] : 0.f;
        }
    }
    // f(j, s_j, t_j) over the lane's columns in increasing j.  (The quotients by T are formed where they are used: holding s / T and
    // t / T in registers as well measured no faster, 8.1 us per launch at 10 x 10 against 7.2 - 7.6 us in separate runs.)
    auto each = [&](auto f) {
        if (REG) {
#pragma unroll
            for (int k = 0; k < BLEND_REG; ++k) {
                const int j = lane + 64 * k;
                if (j < c) f(j, sv[k], tv[k]);
            }
        } else {
            for (int j = lane; j < c; j += 64) f(j, s[j], KD ? t[j] : 0.f);
        }
    };

    // ---- ce_row -----------------------------------------------------------------------------------------------------------------
    float m = -INFINITY, ms = -INFINITY, mt = -INFINITY, xy = 0.f;
    each([&](int j, float sj, float tj) {
        m = fmaxf(m, sj);
        if (j == (int)y) xy = sj;   // the label's logit from the row in hand (a label outside [0, c) reads nothing)
        if (KD) {
            ms = fmaxf(ms, sj / T);
            mt = fmaxf(mt, tj / T);
        }
    });
    m = wave_max(m);
    xy = wave_sum(xy);              // one lane holds it, the others 0: exact
    if (KD) {
        ms = wave_max(ms);
        mt = wave_max(mt);
    }
    float sum = 0.f, ss = 0.f, st = 0.f;
    each([&](int j, float sj, float tj) {
        sum += expf(sj - m);
        if (KD) {
            ss += expf(sj / T - ms);
            st += expf(tj / T - mt);
        }
    });
    sum = wave_sum(sum);
    const float lse = logf(sum) + m;
    const float inv = 1.0f / sum;
    if (!KD) {
        if (dx) {
            each([&](int j, float sj, float) {
                float p = expf(sj - m) * inv;
                dx[j] = (p - (j == (int)y ? 1.f : 0.f)) * scale_new;
            });
        }
        *kd_row = 0.f;
        return lse - xy;
    }
    // ---- kd_kernel's row ------------------------------------------------------------------------------------------------------------
    ss = wave_sum(ss);
    st = wave_sum(st);
    const float lse_t = logf(ss) + ms, inv_s = 1.0f / ss, inv_t = 1.0f / st;
    float row = 0.f;
    each([&](int j, float sj, float tj) {
        float pt = expf(tj / T - mt) * inv_t;
        row -= pt * (sj / T - lse_t);
        if (dx) {
            float p = expf(sj - m) * inv;
            const float g_new = (p - (j == (int)y ? 1.f : 0.f)) * scale_new;
            // both probabilities rounded before they are subtracted (the empty asm keeps the back end from fusing one product into the
            // difference, see ewc.hip): a teacher that equals the student bit for bit contributes exactly 0
            float ps = expf(sj / T - ms) * inv_s;
            asm volatile("" : "+v"(ps), "+v"(pt));
            const float g_old = (ps - pt) * T / n_f;
            dx[j] = g_new + w_old * g_old;
        }
    });
    *kd_row = wave_sum(row);
    return lse - xy;
}

template <bool REG, bool KD>
__global__ void __launch_bounds__(256) ce_kd_blend_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                          const float* __restrict__ teacher, int n, int c, float T, float w_new, float w_old,
                                                          float* __restrict__ loss_out, float* __restrict__ dlogits) {
    __shared__ float part[2][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float n_f = (float)n;
    const float scale_new = w_new * (1.0f / n_f);   // w_new == 1: ce_kernel's scale
    float acc = 0.f, acc_kd = 0.f;
    for (int r = wid; r < n; r += 4) {
        const int64_t at = (int64_t)r * c;
        float kd_row;
        acc += blend_row<REG, KD>(logits + at, KD ? teacher + at : nullptr, c, y[r], lane, T, scale_new, w_old, n_f,
                                  dlogits ? dlogits + at : nullptr, &kd_row);
        acc_kd += kd_row;
    }
    if (lane == 0) {
        part[0][wid] = acc;
        part[1][wid] = acc_kd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ce = (part[0][0] + part[0][1] + part[0][2] + part[0][3]) / n_f;
        const float kd = KD ? (part[1][0] + part[1][1] + part[1][2] + part[1][3]) / n_f * T * T : 0.f;
        loss_out[0] = KD ? w_new * ce + w_old * kd : w_new * ce;
        loss_out[1] = ce;
        loss_out[2] = kd;
    }
}

int ocl_ce_kd_blend_fwd_bwd(const float* logits, const int64_t* y, const float* teacher, int n, int c, float T, float w_new, float w_old,
                            float* loss_out, float* dlogits, void* stream) {
    OCL_REQUIRE(logits && y && loss_out, "ce_kd_blend: null pointer (logits, y and loss_out are required)");
    OCL_REQUIRE(n >= 1 && c >= 1, "ce_kd_blend: n=%d c=%d (both must be >= 1)", n, c);
    OCL_REQUIRE(std::isfinite(T) && T > 0.f, "ce_kd_blend: T=%g (must be finite and > 0)", (double)T);
    OCL_REQUIRE(std::isfinite(w_new) && std::isfinite(w_old), "ce_kd_blend: weights %g, %g (must be finite)", (double)w_new, (double)w_old);
    const size_t bytes = (size_t)n * (size_t)c * sizeof(float);
    if (dlogits) {
        OCL_REQUIRE(!ranges_overlap(dlogits, bytes, logits, bytes), "ce_kd_blend: dlogits overlaps logits");
        OCL_REQUIRE(!(teacher && ranges_overlap(dlogits, bytes, teacher, bytes)), "ce_kd_blend: dlogits overlaps teacher");
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const bool reg = c <= BLEND_REG * 64;
    auto k = teacher ? (reg ? ce_kd_blend_kernel<true, true> : ce_kd_blend_kernel<false, true>)
                     : (reg ? ce_kd_blend_kernel<true, false> : ce_kd_blend_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, logits, y, teacher, n, c, T, w_new, w_old, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
