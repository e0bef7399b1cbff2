// K6d: the two per-row statistics evaluate()'s error analysis needs of a batch of logits (agents/base.py:179-203 of the reference) and of
// the last layer's weight (:217-218), in ONE launch.  With x [n, c] row-major, per row r:
//   argmax_out[r] = the smallest column index among the row's maxima, under the order of torch.max(x, 1) on the CPU: a NaN is larger than
//                   everything and the first NaN wins; -0.0 and +0.0 are equal
//   sum_out[r]    = sum in double of x[r][j] over the columns with col_group[j] == sel (every column with a null col_group)
// which replaces the reference's torch.max, its one .item() per predicted label, its one (wrong == i).sum().item() per class of the
// comparison set, and its column gather with mean().item(): the counts are taken on the host from argmax_out, the class score of a batch
// is sum(sum_out) / (n * k).
//
// The row iterator of the loss family (row_dev.h; the second operand is the columns' group, `sel` where there is none): one wave per
// row, reductions by wave shuffles, no atomics, no scratch, a fixed order of summation.  Lane l adds its columns in ascending order, then
// wave_sum_d.  There is no cross-row reduction, so the rows spread over workgroups: four waves, four rows per workgroup, and a row's two
// results depend neither on n nor on which wave or workgroup computed it.
//
// Columns outside the group are left out by a select on the column's group, never multiplied by 0: a NaN or Inf there leaves the sum's
// bits alone.  An empty group gives +0.0 (the accumulators start there and -0.0 + +0.0 = +0.0).  Nothing in this file may be built with
// fast-math: the NaN order is spelled out with x != x.
#include <climits>
#include <cmath>

#include "row_dev.h"

using namespace ocl;

// (av, ai) comes before (bv, bi) in the order of the arg-max: a NaN above every number, equal values (two NaNs; -0.0 and +0.0) by the
// smaller index.  A total order on pairs with distinct indices, so a butterfly over the wave leaves the same pair in every lane.
__device__ __forceinline__ bool rs_before(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

template <bool REG>
__global__ void __launch_bounds__(64 * ROW_WAVES) row_argmax_groupsum_kernel(const float* __restrict__ x, int n, int c,
                                                                           const int32_t* __restrict__ col_group, int sel,
                                                                           int64_t* __restrict__ argmax_out, double* __restrict__ sum_out) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * ROW_WAVES + wid;
    if (r >= n) return;   // (a whole wave leaves: the shuffles below see all 64 lanes of the waves that stay)
    // a lane without a column holds (-inf, INT_MAX): it loses against every column, a column of -inf included (the index decides)
    float bv = -INFINITY;
    int bi = INT_MAX;
    double acc = 0.0;
    RowCols<REG, int32_t>(x + r * c, col_group, lane, c, col_group ? c : 0, sel).each([&](int j, float v, int32_t g) {
        if (rs_before(v, j, bv, bi)) {
            bv = v;
            bi = j;
        }
        acc += g == sel ? (double)v : 0.0;
    });
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
    const RowArg am = {argmax_out, a_bytes, "argmax_out"}, sm = {sum_out, s_bytes, "sum_out"};
    const RowArg in[2] = {{x, x_bytes, "x"}, {col_group, g_bytes, "col_group"}};
    if (int rc = row_check_output("row_argmax_groupsum", am, in)) return rc;
    if (int rc = row_check_output("row_argmax_groupsum", sm, in)) return rc;
    if (int rc = row_check_output("row_argmax_groupsum", am, {sm})) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    auto k = row_in_regs(c) ? row_argmax_groupsum_kernel<true> : row_argmax_groupsum_kernel<false>;
    hipLaunchKernelGGL(k, dim3(cdiv(n, ROW_WAVES)), dim3(64 * ROW_WAVES), 0, s, x, n, c, col_group, sel, argmax_out, sum_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
