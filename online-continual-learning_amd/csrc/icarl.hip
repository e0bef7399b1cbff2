// K6c: iCaRL's loss (agents/icarl.py:42-62 of the reference) -- the binary cross-entropy of the student's logits against a target that is
// the teacher's sigmoid on the old classes' columns and the one-hot of the stream rows' labels on the new ones -- and its gradient with
// respect to the student's logits, in ONE launch.  With s the student's logits, t the teacher's, sig(x) = 1 / (1 + exp(-x)):
//   z[r][j] = sig(t[r][j])                                     j <  n_old             (every row, stream and memory)
//           = 1 if r < n_stream and j == pos[r], else 0        n_old <= j < n_cls
//   l[r][j] = max(s, 0) - s * z + log1p(exp(-|s|))
//   old = (1/n) sum_r sum_{j < n_old} l        new = (1/n) sum_r sum_{n_old <= j < n_cls} l
//   loss_out = { old + new, old, new }
//   dlogits[r][j] = (sig(s[r][j]) - z[r][j]) / n   for j < n_cls;   +0.0 for n_cls <= j < c
// which is F.binary_cross_entropy_with_logits(logits[:, :n_cls], target, reduction='none').sum(1).mean() with the reference's target:
// the one-hot scatter, zeros_like, the two cats, the sigmoid, the `for k in old_labels: target[:, k] = q[:, k]` loop of one strided
// copy per old class, the loss, its row sum and mean, and autograd's walk back through them.
//
// The shape of the CE family (row_losses.hip) and of distill.hip: a single workgroup of four waves, one wave per row, reductions by wave
// shuffles, the per-wave partial sums through LDS and added in index order -- no atomics, a fixed order of summation, two runs give the
// same bits.  The loss is element-wise, so a row is read exactly once either way; a row of up to ROW_REG * 64 columns has all its loads
// issued before the arithmetic and sits in registers (lane l holds columns l, l + 64, ...), a longer row takes a strided loop.
//
// Columns the reference slices away are never READ: logits and teacher columns j >= n_cls, teacher columns j >= n_old (a NaN there
// changes nothing; a product with 0 would not do).  sig(s) and sig(t) come from one device function and each is rounded before they are
// subtracted, so a teacher that equals the student bit for bit gives exactly 0 on the old columns.  An element's three terms are added
// in double (the product of two floats is exact there: no cancellation between max(s, 0) and s * z at large |s|), and so are the row
// and cross-row sums, as clip.hip and gradproj.hip carry theirs; the transcendental functions are float.  Nothing in this file may be
// built with fast-math.
#include <cmath>

#include "row_dev.h"

using namespace ocl;

// (Its own iterator, row loop and fold, not row_dev.h's: see "not shared" there.  ROW_REG, row_in_regs and row_check_output are shared.)
// sig(x) = 1 / (1 + exp(-x)) without overflow, from e = exp(-|x|) (which the loss's log1p term needs as well)
__device__ __forceinline__ float exp_neg_abs(float x) { return expf(-fabsf(x)); }
__device__ __forceinline__ float sigmoid(float x) {
    const float e = exp_neg_abs(x);
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// One row, by one wave.  REG: the row's live columns sit in sv / tv; otherwise the loop reads s / t as it goes.  KD: a teacher is present
// and n_old > 0.  p: the row's target column (a stream row's pos; -1 for a memory row; anything outside [n_old, n_cls) sets no target).
// acc_old, acc_new: the lane's running sums of l over the old and the new columns of its rows (reduced across the wave once, by the caller).
template <bool REG, bool KD>
__device__ __forceinline__ void bce_row(const float* __restrict__ s, const float* __restrict__ t, int c, int n_cls, int n_old, int64_t p,
                                        int lane, float n_f, float* __restrict__ dx, double& acc_old, double& acc_new) {
    float sv[ROW_REG], tv[ROW_REG];
    if (REG) {
#pragma unroll
        for (int k = 0; k < ROW_REG; ++k) {
            const int j = lane + 64 * k;
            sv[k] = j < n_cls ? s[j] : 0.f;
            tv[k] = (KD && j < n_old) ? t[j] : 0.f;
        }
    }
    auto f = [&](int j, float sj, float tj) {
        const float e = exp_neg_abs(sj);   // (the same expression as inside sigmoid(sj): evaluated once)
        float ps = sigmoid(sj);
        const bool old = KD && j < n_old;
        float z = (int64_t)j == p ? 1.f : 0.f;
        if (old) z = sigmoid(tj);
        // both rounded before they are subtracted (the empty asm keeps the back end from fusing anything into the difference, see
        // distill.hip and ewc.hip): equal logits give exactly 0
        asm volatile("" : "+v"(ps), "+v"(z));
        const double l = (double)fmaxf(sj, 0.f) - (double)sj * (double)z + (double)log1pf(e);
        acc_old += old ? l : 0.0;   // (two selects: an if / else over the two sums becomes an indexed array in scratch)
        acc_new += old ? 0.0 : l;
        if (dx) dx[j] = (ps - z) / n_f;
    };
    if (REG) {
#pragma unroll
        for (int k = 0; k < ROW_REG; ++k) {
            const int j = lane + 64 * k;
            if (j < n_cls) f(j, sv[k], tv[k]);
        }
    } else {
        for (int j = lane; j < n_cls; j += 64) f(j, s[j], (KD && j < n_old) ? t[j] : 0.f);
    }
    if (dx)
        for (int j = n_cls + lane; j < c; j += 64) dx[j] = 0.f;   // the columns the reference's slice leaves out of the graph
}

template <bool REG, bool KD>
__global__ void __launch_bounds__(256) bce_distill_kernel(const float* __restrict__ logits, const float* __restrict__ teacher,
                                                          const int64_t* __restrict__ pos, int n, int n_stream, int c, int n_cls, int n_old,
                                                          float* __restrict__ loss_out, float* __restrict__ dlogits) {
    __shared__ double part[2][4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float n_f = (float)n;
    double acc_old = 0.0, acc_new = 0.0;
    for (int r = wid; r < n; r += 4) {
        const int64_t at = (int64_t)r * c;
        bce_row<REG, KD>(logits + at, KD ? teacher + at : nullptr, c, n_cls, n_old, r < n_stream ? pos[r] : (int64_t)-1, lane, n_f,
                         dlogits ? dlogits + at : nullptr, acc_old, acc_new);
    }
    // each lane has added its columns of the wave's rows in row order; one shuffle tree per sum and per wave
    acc_old = KD ? wave_sum_d(acc_old) : 0.0;
    acc_new = wave_sum_d(acc_new);
    if (lane == 0) {
        part[0][wid] = acc_old;
        part[1][wid] = acc_new;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double old = (part[0][0] + part[0][1] + part[0][2] + part[0][3]) / (double)n;
        const double nw = (part[1][0] + part[1][1] + part[1][2] + part[1][3]) / (double)n;
        loss_out[0] = (float)(old + nw);
        loss_out[1] = (float)old;
        loss_out[2] = (float)nw;
    }
}

int ocl_bce_distill_fwd_bwd(const float* logits, const float* teacher, const int64_t* pos, int n, int n_stream, int c, int n_cls, int n_old,
                            float* loss_out, float* dlogits, void* stream) {
    OCL_REQUIRE(logits && pos && loss_out, "bce_distill: null pointer (logits, pos and loss_out are required)");
    OCL_REQUIRE(n >= 1 && c >= 1, "bce_distill: n=%d c=%d (both must be >= 1)", n, c);
    OCL_REQUIRE(n_stream >= 1 && n_stream <= n, "bce_distill: n_stream=%d with n=%d (1 <= n_stream <= n)", n_stream, n);
    OCL_REQUIRE(n_old >= 0 && n_old <= n_cls && n_cls <= c, "bce_distill: n_old=%d n_cls=%d c=%d (0 <= n_old <= n_cls <= c)", n_old, n_cls, c);
    OCL_REQUIRE(teacher || n_old == 0, "bce_distill: n_old=%d without a teacher (a null teacher requires n_old == 0)", n_old);
    const size_t bytes = (size_t)n * (size_t)c * sizeof(float);
    if (int rc = row_check_output("bce_distill", {dlogits, bytes, "dlogits"},
                                  {{logits, bytes, "logits"}, {teacher, bytes, "teacher"}, {pos, (size_t)n_stream * sizeof(int64_t), "pos"}}))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const bool reg = row_in_regs(c), kd = n_old > 0;
    auto k = kd ? (reg ? bce_distill_kernel<true, true> : bce_distill_kernel<false, true>)
                : (reg ? bce_distill_kernel<true, false> : bce_distill_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, logits, teacher, pos, n, n_stream, c, n_cls, n_old, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
