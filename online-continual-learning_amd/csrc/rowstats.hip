// K6d: the two per-row statistics evaluate()'s error analysis needs of a batch of logits (agents/base.py:179-203 of the reference) and of
// the last layer's weight (:217-218), in ONE launch.  With x [n, c] row-major, per row r:
//   argmax_out[r] = the smallest column index among the row's maxima, under the order of torch.max(x, 1) on the CPU: a NaN is larger than
//                   everything and the first NaN wins; -0.0 and +0.0 are equal
//   sum_out[r]    = sum in double of x[r][j] over the columns with col_group[j] == sel (every column with a null col_group)
// which replaces the reference's torch.max, its one .item() per predicted label, its one (wrong == i).sum().item() per class of the
// comparison set, and its column gather with mean().item(): the counts are taken on the host from argmax_out, the class score of a batch
// is sum(sum_out) / (n * k).
//
// The shape of distill.hip and icarl.hip: one wave per row, reductions by wave shuffles, no atomics, no scratch, a fixed order of
// summation.  A row of up to RS_REG * 64 columns has all its loads issued before the arithmetic and sits in registers (lane l holds columns
// l, l + 64, ...), a longer row takes a strided loop; either way lane l adds its columns in ascending order, then wave_sum_d.  There is
// no cross-row reduction, so the rows spread over workgroups: four waves, four rows per workgroup, and a row's two results depend
// neither on n nor on which wave or workgroup computed it.
//
// Columns outside the group are left out by a select on the column's group, never multiplied by 0: a NaN or Inf there leaves the sum's
// bits alone.  An empty group gives +0.0 (the accumulators start there and -0.0 + +0.0 = +0.0).  Nothing in this file may be built with
// fast-math: the NaN order is spelled out with x != x.
#include <climits>
#include <cmath>

#include "common.h"

using namespace ocl;

static constexpr int RS_REG = 4;       // registers per lane: rows of up to 256 columns stay in registers
static constexpr int RS_ROWS = 4;      // rows (= waves) per workgroup

// (av, ai) comes before (bv, bi) in the order of the arg-max: a NaN above every number, equal values (two NaNs; -0.0 and +0.0) by the
// smaller index.  A total order on pairs with distinct indices, so a butterfly over the wave leaves the same pair in every lane.
__device__ __forceinline__ bool rs_before(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

template <bool REG>
__global__ void __launch_bounds__(64 * RS_ROWS) row_argmax_groupsum_kernel(const float* __restrict__ x, int n, int c,
                                                                           const int32_t* __restrict__ col_group, int sel,
                                                                           int64_t* __restrict__ argmax_out, double* __restrict__ sum_out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * RS_ROWS + wid;
    if (r >= n) return;   // (a whole wave leaves: the shuffles below see all 64 lanes of the waves that stay)
    const float* __restrict__ row = x + r * c;
    // a lane without a column holds (-inf, INT_MAX): it loses against every column, a column of -inf included (the index decides)
    float bv = -INFINITY;
    int bi = INT_MAX;
    double acc = 0.0;
    auto f = [&](int j, float v, bool in) {
        if (rs_before(v, j, bv, bi)) {
            bv = v;
            bi = j;
        }
        acc += in ? (double)v : 0.0;
    };
    if (REG) {
        float xv[RS_REG];
        int gv[RS_REG];
#pragma unroll
        for (int k = 0; k < RS_REG; ++k) {
            const int j = lane + 64 * k;
            xv[k] = j < c ? row[j] : 0.f;
            gv[k] = (col_group && j < c) ? col_group[j] : sel;
        }
#pragma unroll
        for (int k = 0; k < RS_REG; ++k) {
            const int j = lane + 64 * k;
            if (j < c) f(j, xv[k], gv[k] == sel);
        }
    } else {
        for (int j = lane; j < c; j += 64) f(j, row[j], col_group ? col_group[j] == sel : true);
    }
    if (argmax_out) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (rs_before(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) argmax_out[r] = (int64_t)bi;
    }
    if (sum_out) {
        acc = wave_sum_d(acc);
        if (lane == 0) sum_out[r] = acc;
    }
}

int ocl_row_argmax_groupsum(const float* x, int n, int c, const int32_t* col_group, int sel, int64_t* argmax_out, double* sum_out,
                            void* stream) {
    OCL_REQUIRE(x, "row_argmax_groupsum: null pointer (x is required)");
    OCL_REQUIRE(argmax_out || sum_out, "row_argmax_groupsum: null pointer (at least one of argmax_out and sum_out is required)");
    OCL_REQUIRE(n >= 1 && c >= 1, "row_argmax_groupsum: n=%d c=%d (both must be >= 1)", n, c);
    const size_t x_bytes = (size_t)n * (size_t)c * sizeof(float), g_bytes = (size_t)c * sizeof(int32_t);
    const size_t a_bytes = (size_t)n * sizeof(int64_t), s_bytes = (size_t)n * sizeof(double);
    if (argmax_out) {
        OCL_REQUIRE(!ranges_overlap(argmax_out, a_bytes, x, x_bytes), "row_argmax_groupsum: argmax_out overlaps x");
        OCL_REQUIRE(!(col_group && ranges_overlap(argmax_out, a_bytes, col_group, g_bytes)), "row_argmax_groupsum: argmax_out overlaps col_group");
    }
    if (sum_out) {
        OCL_REQUIRE(!ranges_overlap(sum_out, s_bytes, x, x_bytes), "row_argmax_groupsum: sum_out overlaps x");
        OCL_REQUIRE(!(col_group && ranges_overlap(sum_out, s_bytes, col_group, g_bytes)), "row_argmax_groupsum: sum_out overlaps col_group");
    }
    OCL_REQUIRE(!(argmax_out && sum_out && ranges_overlap(argmax_out, a_bytes, sum_out, s_bytes)), "row_argmax_groupsum: argmax_out overlaps sum_out");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    auto k = c <= RS_REG * 64 ? row_argmax_groupsum_kernel<true> : row_argmax_groupsum_kernel<false>;
    hipLaunchKernelGGL(k, dim3(cdiv(n, RS_ROWS)), dim3(64 * RS_ROWS), 0, s, x, n, c, col_group, sel, argmax_out, sum_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
