// K6b: Learning without Forgetting's loss (agents/lwf.py:36-39 of the reference) -- the cross-entropy of the student's logits
// (agents/base.py:113) blended with the distillation loss against the teacher's (utils/kd_manager.py:6-11) -- and its gradient with
// respect to the student's logits, in ONE launch:
//   ce   = mean_r( lse(s_r) - s_r[y_r] )
//   kd   = mean_r( -sum_j softmax(t_r / T)_j * log_softmax(s_r / T)_j ) * T^2
//   loss_out = { w_new * ce + w_old * kd, ce, kd }
//   dlogits[r][j] = w_new * (softmax(s_r)_j - [j == y_r]) / n + w_old * (softmax(s_r / T)_j - softmax(t_r / T)_j) * T / n
// The shape of the CE family (row_dev.h): a single workgroup of four waves, one wave per row, a fixed order of summation.  The row
// calls the cross-entropy row and the distillation row of row_dev.h from its own three passes over the columns (independent accumulators
// fused into one pass keep their bits): without a teacher (LwF's first task) and with w_new == 1 the cross-entropy and its gradient are
// ocl_ce_fwd_bwd's bits, because they are its code.  A row of up to ROW_REG * 64 logits is read from memory once and kept in registers.
// Nothing in this file may be built with fast-math.
#include <cmath>

#include "row_dev.h"

using namespace ocl;

// One row, by one wave.  KD: a teacher is present.  Returns the row's cross-entropy; kd_acc gains the row's distillation term
// (before the mean and T^2).  (The quotients by T are formed where they are used: holding s / T and t / T in registers as well measured
// no faster, 8.1 us per launch at 10 x 10 against 7.2 - 7.6 us in separate runs.)
template <bool REG, bool KD>
__device__ __forceinline__ float blend_row(const float* __restrict__ s, const float* __restrict__ t, int c, int64_t y, int lane, float T,
                                           float scale_new, float w_old, float n_f, float* __restrict__ dx, float& kd_acc) {
    // (its own iterator, not RowCols: see "not shared" in row_dev.h)  f(j, s_j, t_j) over the lane's columns in increasing j
    float sv[ROW_REG], tv[ROW_REG];
    if (REG) {
#pragma unroll
        for (int k = 0; k < ROW_REG; ++k) {
            const int j = lane + 64 * k;
            sv[k] = j < c ? s[j] : 0.f;
            tv[k] = (KD && j < c) ? t[j] : 0.f;
        }
    }
    auto each = [&](auto f) {
        if (REG) {
#pragma unroll
            for (int k = 0; k < ROW_REG; ++k) {
                const int j = lane + 64 * k;
                if (j < c) f(j, sv[k], tv[k]);
            }
        } else {
            for (int j = lane; j < c; j += 64) f(j, s[j], KD ? t[j] : 0.f);
        }
    };
    RowSoftmax ce;
    KdRow kd(T);
    float xy = 0.f;
    each([&](int j, float sj, float tj) {
        ce.max_of(sj);
        if (j == (int)y) xy = sj;   // the label's logit from the row in hand (a label outside [0, c) reads nothing)
        if (KD) kd.max_of(sj, tj);
    });
    ce.max_done();
    xy = wave_sum(xy);              // one lane holds it, the others 0: exact
    if (KD) kd.max_done();
    each([&](int, float sj, float tj) {
        ce.sum_of(sj);
        if (KD) kd.sum_of(sj, tj);
    });
    ce.sum_done();
    if (KD) kd.sum_done();
    if (KD || dx)
        each([&](int j, float sj, float tj) {
            float pt = 0.f;
            if (KD) {
                pt = kd.pt_of(tj);
                kd.term(sj, pt);
            }
            if (!dx) return;
            float g = ce_grad(ce.p(sj), j == (int)y, scale_new);
            if (KD) {
                // both probabilities rounded before they are subtracted (the empty asm keeps the back end from fusing one product into the
                // difference, see ewc.hip): a teacher that equals the student bit for bit contributes exactly 0
                float ps = kd.ps_of(sj);
                asm volatile("" : "+v"(ps), "+v"(pt));
                g += w_old * kd.grad(ps, pt, n_f);
            }
            dx[j] = g;
        });
    kd_acc += KD ? wave_sum(kd.row) : 0.f;
    return ce.lse() - xy;
}

template <bool REG, bool KD>
__global__ void __launch_bounds__(256) ce_kd_blend_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                          const float* __restrict__ teacher, int n, int c, float T, float w_new, float w_old,
                                                          float* __restrict__ loss_out, float* __restrict__ dlogits) {
    __shared__ float part[2][4];   // (its own row loop and fold, not row_dev.h's: see "not shared" there)
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float n_f = (float)n;
    const float scale_new = w_new * (1.0f / n_f);   // w_new == 1: ce_kernel's scale
    float acc = 0.f, acc_kd = 0.f;
    for (int r = wid; r < n; r += 4) {
        const int64_t at = (int64_t)r * c;
        acc += blend_row<REG, KD>(logits + at, KD ? teacher + at : nullptr, c, y[r], lane, T, scale_new, w_old, n_f,
                                  dlogits ? dlogits + at : nullptr, acc_kd);
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
    if (int rc = row_check_output("ce_kd_blend", {dlogits, bytes, "dlogits"}, {{logits, bytes, "logits"}, {teacher, bytes, "teacher"}})) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const bool reg = row_in_regs(c);
    auto k = teacher ? (reg ? ce_kd_blend_kernel<true, true> : ce_kd_blend_kernel<false, true>)
                     : (reg ? ce_kd_blend_kernel<true, false> : ce_kd_blend_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, logits, y, teacher, n, c, T, w_new, w_old, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
