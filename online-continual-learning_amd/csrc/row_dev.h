// The one row skeleton of the per-row loss kernels (K6 cross-entropy, segmented cross-entropy and distillation, K12 MIR in row_losses.hip;
// K6b ce_kd_blend in distill.hip; K6c bce_distill in icarl.hip; K6d row_argmax_groupsum in rowstats.hip; K6e der_loss in der.hip): one
// wave per row, lane l owning columns l, l + 64, ..., and the two row formulas that more than one of them evaluates.
//
// What is fixed here, and why the code has this shape:
//   * RowCols: the lane's columns of a row and of a second operand beside it (a teacher's row, the columns' segment or group ids),
//     visited by each(f) as f(j, s_j, t_j) in ascending j.  REG: both are loaded into ROW_REG registers each before any arithmetic
//     (rows of up to ROW_REG * 64 columns, row_in_regs()); otherwise every pass reads memory again.  The row is read below column ns,
//     the second operand below column nt and is `fill` from there on: a column the reference slices away is never READ.
//   * a loss over the rows is ONE workgroup of ROW_WAVES waves: wave w takes rows w, w + 4, ... (ROW_FOR_EACH), lane 0 of every wave
//     writes its K sums to LDS and thread 0 adds the four slots in index order (row_fold).  No atomics, a fixed order of summation:
//     two runs give the same bits.  What is summed before the fold is the caller's (a wave_sum per row, or per-lane doubles across
//     the rows and one wave_sum_d).
//   * the softmax cross-entropy row (RowSoftmax, ce_grad, ce_row) and the distillation row (KdRow: two softmaxes at temperature T) are
//     written once; ce_kd_blend's row calls both from its own fused passes, so without a teacher and with w_new == 1 it IS ce_kernel's
//     arithmetic.  x / T is a true division, as the reference divides (kd_manager.py:7-8): a multiplication by the rounded 1 / T moves
//     the logit by up to |x| / T * 2^-24 for a T that is no power of two, 2e-5 at |x| = 2000, T = 3.
//   * nothing that includes this header may be built with fast-math.
// What is not shared: the label's logit (ce_row reads x[y], NaN for a label outside the row; ce_kd_blend picks it up from the row in
// hand and reads nothing), the rounding barriers of ce_kd_blend's and bce_distill's gradients (they stay at their sites), the register
// form for ce_kernel, ce_seg_kernel, kd_kernel and mir_kernel (strided today; moving them would be a speed change), the grids of
// mir_kernel and row_argmax_groupsum_kernel (four rows per workgroup and no cross-row sum: ROW_WAVES alone), supcon_rows, the NCM
// kernels and the cosine kernels' (r0 + r1) + (r2 + r3) block stage (supcon.hip, ncm.hip, cosine.hip), and the head chain of net.hip.
// Sent back to their own statements for speed (same bits on the header, but a mean kernel time above the parent's by more than the
// parent's own run-to-run difference of 0.00 - 0.02 us, at n = 10 and 20 rows of c = 100; profiles/row_family_kernel_times.txt):
//   * ce_seg_kernel: its own row (ce_row_seg), loop and fold.  On ce_row with a column predicate, ROW_FOR_EACH and row_fold: 9.16 - 9.27 us
//     against 9.12 - 9.14; on its own row with ROW_FOR_EACH and row_fold: 9.10 - 9.21 against 9.09 - 9.11.
//   * bce_distill_kernel: its own iterator, loop and fold.  On RowCols, ROW_FOR_EACH and row_fold: 6.02 - 6.43 us against 5.95 - 5.97; on
//     its own iterator with ROW_FOR_EACH and row_fold: 6.04 - 6.49 against 5.90 - 5.91.
//   * ce_kd_blend_kernel: its own iterator, loop and fold; it still calls RowSoftmax, ce_grad and KdRow.  On RowCols, ROW_FOR_EACH and
//     row_fold: 9.14 - 9.40 us against 9.03 - 9.05 (RowCols<true> left four more exec-mask regions per row in the register form).
#pragma once
#include "common.h"

namespace ocl {

static constexpr int ROW_REG = 4;     // registers per lane and per operand: rows of up to 256 columns stay in registers
static constexpr int ROW_WAVES = 4;   // waves per workgroup: rows in flight
static inline bool row_in_regs(int c) { return c <= ROW_REG * 64; }

// ---- device: the lane's columns of a row --------------------------------------------------------------------------------------------
template <bool REG, class B = float>
struct RowCols {
    const float* __restrict__ s;
    const B* __restrict__ t;
    int lane, ns, nt;
    B fill;
    float sv[ROW_REG];
    B tv[ROW_REG];
    __device__ __forceinline__ RowCols(const float* s_, const B* t_, int lane_, int ns_, int nt_, B fill_)
        : s(s_), t(t_), lane(lane_), ns(ns_), nt(nt_), fill(fill_) {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < ROW_REG; ++k) {
                const int j = lane + 64 * k;
                sv[k] = j < ns ? s[j] : 0.f;
                tv[k] = j < nt ? t[j] : fill;
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < ROW_REG; ++k) {
                const int j = lane + 64 * k;
                if (j < ns) f(j, sv[k], tv[k]);
            }
        } else {
            for (int j = lane; j < ns; j += 64) f(j, s[j], j < nt ? t[j] : fill);
        }
    }
};

// ---- device: the one-workgroup row loop and its fold -------------------------------------------------------------------------------
// (a macro, not row_for_each(n, body): with the row's body as a [&] lambda, AMD clang 22.0.0git (roc-7.2.0, HIP 7.2.26015) at -O3
// dies with a segmentation fault in the inliner (updateCGAndAnalysisManagerForPass) on a kernel template whose body goes on to
// RowCols<true>::each -- bce_distill_kernel<true, *> and ce_kd_blend_kernel<true, *> when they were written over it)
#define ROW_FOR_EACH(r, n) for (int r = threadIdx.x >> 6; r < (n); r += ROW_WAVES)

// every wave's K sums (as its lane 0 holds them) -> their sums over the waves, in thread 0's acc.  Call it once per kernel: the LDS
// slots belong to <T, K> and nothing fences thread 0's reads from a second call's writes.
template <class T, int K>
__device__ __forceinline__ void row_fold(T (&acc)[K]) {
    __shared__ T part[K][ROW_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[k][wid] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = part[k][0] + part[k][1] + part[k][2] + part[k][3];
    }
}

// ---- device: the two row formulas -------------------------------------------------------------------------------------------------
// A softmax over the lane's share of a row in three passes, an element at a time; a wave calls the *_done() between the passes.
struct RowSoftmax {
    float m = -INFINITY, sum = 0.f, inv;
    __device__ __forceinline__ void max_of(float x) { m = fmaxf(m, x); }
    __device__ __forceinline__ void max_done() { m = wave_max(m); }
    __device__ __forceinline__ void sum_of(float x) { sum += expf(x - m); }
    __device__ __forceinline__ void sum_done() {
        sum = wave_sum(sum);
        inv = 1.0f / sum;
    }
    __device__ __forceinline__ float lse() const { return logf(sum) + m; }
    __device__ __forceinline__ float p(float x) const { return expf(x - m) * inv; }
};

// d (lse - x[label]) / d x_j * scale, from the column's probability
__device__ __forceinline__ float ce_grad(float p, bool is_label, float scale) { return (p - (is_label ? 1.f : 0.f)) * scale; }

// The cross-entropy lse - x[y] of the row x of c columns, and its gradient into dx (optional).  A label outside the row is no address:
// the loss is NaN (K6, K12).  exact (optional): the loss with its three pieces (log of the sum, the max,
// x[y]) combined in double, for a caller that subtracts two row losses (mir_kernel: their fp32 roundings would dominate the difference)
template <class Cols>
__device__ __forceinline__ float ce_row(const Cols& cols, int c, int64_t y, float* __restrict__ dx, float scale, double* exact = nullptr) {
    RowSoftmax sm;
    cols.each([&](int, float x, float) { sm.max_of(x); });
    sm.max_done();
    cols.each([&](int, float x, float) { sm.sum_of(x); });
    sm.sum_done();
    const float xy = (uint64_t)y < (uint64_t)c ? cols.s[y] : NAN;
    if (dx) cols.each([&](int j, float x, float) { dx[j] = ce_grad(sm.p(x), (int64_t)j == y, scale); });
    if (exact) *exact = ((double)logf(sm.sum) + (double)sm.m) - (double)xy;
    return sm.lse() - xy;
}

// The distillation row (utils/kd_manager.py:6-11): -sum_j softmax(t / T)_j * log_softmax(s / T)_j in `row` (the lane's share: the
// caller's wave_sum), and the gradient element (softmax(s / T)_j - softmax(t / T)_j) * T / n
struct KdRow {
    float T, lse, row = 0.f;
    RowSoftmax s, t;
    __device__ __forceinline__ explicit KdRow(float T_) : T(T_) {}
    __device__ __forceinline__ void max_of(float sj, float tj) {
        s.max_of(sj / T);
        t.max_of(tj / T);
    }
    __device__ __forceinline__ void max_done() {
        s.max_done();
        t.max_done();
    }
    __device__ __forceinline__ void sum_of(float sj, float tj) {
        s.sum_of(sj / T);
        t.sum_of(tj / T);
    }
    __device__ __forceinline__ void sum_done() {
        s.sum_done();
        t.sum_done();
        lse = s.lse();
    }
    __device__ __forceinline__ float ps_of(float sj) const { return s.p(sj / T); }
    __device__ __forceinline__ float pt_of(float tj) const { return t.p(tj / T); }
    __device__ __forceinline__ void term(float sj, float pt) { row -= pt * (sj / T - lse); }
    __device__ __forceinline__ float grad(float ps, float pt, float n_f) const { return (ps - pt) * T / n_f; }
};

// ---- host: the argument check of an entry point ------------------------------------------------------------------------------------
struct RowArg {
    const void* ptr;
    size_t bytes;
    const char* name;
};

// `out` (when given) shares no byte with any of the inputs that are given.  Sets the error text "<op>: <out> overlaps <input>" and
// returns OCL_ERR_ARG, or returns OCL_OK.
template <int N>
static inline int row_check_output(const char* op, const RowArg& out, const RowArg (&in)[N]) {
    for (int i = 0; i < N; ++i)
        OCL_REQUIRE(!(out.ptr && in[i].ptr && ranges_overlap(out.ptr, out.bytes, in[i].ptr, in[i].bytes)), "%s: %s overlaps %s", op, out.name,
                    in[i].name);
    return OCL_OK;
}

}  // namespace ocl
