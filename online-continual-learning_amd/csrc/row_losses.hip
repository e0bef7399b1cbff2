// K6 + K12: the founding members of the per-row loss family (row_dev.h): cross-entropy, cross-entropy over a column segment,
// knowledge distillation, and the MIR score (a difference of two cross-entropies per row).  One wave per row.
#include "row_dev.h"
#include "small_ops.h"
#include <limits.h>
#include <math.h>

using namespace ocl;

namespace ocl {
SPlan plan_ce(int path) { return splan(path, 1, 1, 256); }   // ce / ce_seg / kd: a single workgroup, one wave per row
SPlan plan_mir(int n) { return splan(OCL_PATH_MIR, (unsigned)cdiv(n, 4), 1, 256); }
}  // namespace ocl

// =====================================================================================================
// K6 cross-entropy: single workgroup, one wave per row, deterministic mean (row_dev.h has the loop, the fold and the row formulas)
// =====================================================================================================
__global__ void __launch_bounds__(256) ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y, int n, int c,
                                                 int reduction, float* __restrict__ loss_out, float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const float scale = reduction == 1 ? 1.0f / (float)n : 1.0f;
    float acc[1] = {0.f};
    ROW_FOR_EACH(r, n) {
        float l = ce_row(RowCols<false>(logits + (int64_t)r * c, nullptr, lane, c, 0, 0.f), c, y[r],
                         dlogits ? dlogits + (int64_t)r * c : nullptr, scale);
        if (reduction == 0) {
            if (lane == 0) loss_out[r] = l;
        } else {
            acc[0] += l;
        }
    }
    if (reduction == 1) {
        row_fold(acc);
        if (threadIdx.x == 0) loss_out[0] = acc[0] / (float)n;
    }
}

// Cross-entropy over a column segment (agents/base.py:96-108, the labels trick and the separated softmax): seg[j] in {-1, 0, 1, ...}
// assigns every logit column to a segment (-1: takes no part); row r is a softmax over the columns of its label's segment.
// (Its own row and loop, not row_dev.h's: see "not shared" there.)
__device__ __forceinline__ float ce_row_seg(const float* __restrict__ x, const int* __restrict__ seg, int c, int64_t y, int lane,
                                            float* __restrict__ dx, float scale) {
    // a label outside the row is no address (K6): its segment id is one no column has (ids are >= -1), so the row's softmax is empty
    // (dx = 0 in every column) and its loss NaN
    const bool in_row = (uint64_t)y < (uint64_t)c;
    const int sid = in_row ? seg[y] : INT_MIN;
    float m = -INFINITY;
    for (int j = lane; j < c; j += 64)
        if (seg[j] == sid) m = fmaxf(m, x[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < c; j += 64)
        if (seg[j] == sid) s += expf(x[j] - m);
    s = wave_sum(s);
    const float lse = logf(s) + m;
    const float xy = in_row ? x[y] : NAN;
    if (dx) {
        const float inv = 1.0f / s;
        for (int j = lane; j < c; j += 64) {
            const float p = seg[j] == sid ? expf(x[j] - m) * inv : 0.f;
            dx[j] = (p - ((int64_t)j == y ? 1.f : 0.f)) * scale;
        }
    }
    return lse - xy;
}

__global__ void __launch_bounds__(256) ce_seg_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y,
                                                     const int* __restrict__ seg, int n, int c, float* __restrict__ loss_out,
                                                     float* __restrict__ dlogits) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const float scale = 1.0f / (float)n;
    float acc = 0.f;
    for (int r = wid; r < n; r += 4)
        acc += ce_row_seg(logits + (int64_t)r * c, seg, c, y[r], lane, dlogits ? dlogits + (int64_t)r * c : nullptr, scale);
    if (lane == 0) part[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss_out[0] = (part[0] + part[1] + part[2] + part[3]) / (float)n;
}

// Knowledge-distillation loss (utils/kd_manager.py:6-11): mean_r( -sum_j softmax(t_r/T)_j * log_softmax(s_r/T)_j ) * T^2, and its
// gradient w.r.t. the student scores, (softmax(s/T) - softmax(t/T)) * T / n.  One wave per row.
__global__ void __launch_bounds__(256) kd_kernel(const float* __restrict__ scores, const float* __restrict__ target, int n, int c,
                                                 float T, float* __restrict__ loss_out, float* __restrict__ dscores) {
    const int lane = threadIdx.x & 63;
    float acc[1] = {0.f};
    ROW_FOR_EACH(r, n) {
        const RowCols<false> cols(scores + (int64_t)r * c, target + (int64_t)r * c, lane, c, c, 0.f);
        KdRow kd(T);
        cols.each([&](int, float s, float t) { kd.max_of(s, t); });
        kd.max_done();
        cols.each([&](int, float s, float t) { kd.sum_of(s, t); });
        kd.sum_done();
        cols.each([&](int j, float s, float t) {
            const float pt = kd.pt_of(t);
            kd.term(s, pt);
            if (dscores) dscores[(int64_t)r * c + j] = kd.grad(kd.ps_of(s), pt, (float)n);
        });
        acc[0] += wave_sum(kd.row);
    }
    row_fold(acc);
    if (threadIdx.x == 0) loss_out[0] = acc[0] / (float)n * T * T;
}

// K12 MIR: post CE - pre CE per sample; four rows per workgroup, no sum across the rows
__global__ void __launch_bounds__(256) mir_kernel(const float* __restrict__ pre, const float* __restrict__ post,
                                                  const int64_t* __restrict__ y, int n, int c, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = blockIdx.x * ROW_WAVES + wid;
    if (r >= n) return;
    double a, b;
    ce_row(RowCols<false>(pre + (int64_t)r * c, nullptr, lane, c, 0, 0.f), c, y[r], nullptr, 1.f, &a);
    ce_row(RowCols<false>(post + (int64_t)r * c, nullptr, lane, c, 0, 0.f), c, y[r], nullptr, 1.f, &b);
    if (lane == 0) out[r] = (float)(b - a);
}

int ocl_ce_fwd_bwd(const float* logits, const int64_t* y, int n, int c, int reduction, float* loss_out, float* dlogits,
                   void* stream) {
    OCL_REQUIRE(logits && y && loss_out && n > 0 && c > 0, "ce: bad arguments");
    OCL_REQUIRE(reduction == 0 || reduction == 1, "ce: reduction must be 0 (none) or 1 (mean)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const SPlan pl = plan_ce(reduction ? OCL_PATH_CE_MEAN : OCL_PATH_CE_NONE);
    hipLaunchKernelGGL(ce_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, logits, y, n, c, reduction, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_ce_segmented_fwd_bwd(const float* logits, const int64_t* y, const int32_t* seg, int n, int c, float* loss_out, float* dlogits,
                             void* stream) {
    OCL_REQUIRE(logits && y && seg && loss_out && n > 0 && c > 0, "ce_segmented: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const SPlan pl = plan_ce(OCL_PATH_CE_SEG);
    hipLaunchKernelGGL(ce_seg_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, logits, y, seg, n, c, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_kd_fwd_bwd(const float* scores, const float* target_scores, int n, int c, float T, float* loss_out, float* dscores,
                   void* stream) {
    OCL_REQUIRE(scores && target_scores && loss_out && n > 0 && c > 0 && T > 0.f, "kd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const SPlan pl = plan_ce(OCL_PATH_KD);
    hipLaunchKernelGGL(kd_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, scores, target_scores, n, c, T, loss_out, dscores);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_mir_scores(const float* logits_pre, const float* logits_post, const int64_t* y, int n, int c, float* scores_out,
                   void* stream) {
    OCL_REQUIRE(logits_pre && logits_post && y && scores_out && n > 0 && c > 0, "mir_scores: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_mir(n);
    hipLaunchKernelGGL(mir_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, logits_pre, logits_post, y, n, c, scores_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
