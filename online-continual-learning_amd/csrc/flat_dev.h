// The one streaming skeleton of the flat-array kernels (K8 SGD and K8b Adam in optim.hip, K8c A-GEM, K8d EWC++, K8e clip): every kernel over the flat
// parameter or gradient array is this loop, these two reduction stages and this argument check, plus its own per-element mathematics.
//
// What is fixed here, and why the code has this shape:
//   * 256 threads per block; a grid-stride loop over float4 groups (one dwordx4 access per array), then a scalar tail that starts at
//     (n >> 2 << 2) + the thread's global index.  A body sees a 4-wide and then a 1-wide accessor and writes its arithmetic once, as a
//     loop over k < W: lanes are taken in the order x, y, z, w, so an accumulator gets its addends in element order within a thread.
//   * a sum is reduced in double, without atomics, in an order that is a function of n alone: per thread in loop order, per wave by
//     wave_sum_d's shuffle tree, per block by thread 0 adding the waves' LDS slots in index order (flat_block_partial), over the grid by
//     the first wave of every block, lane l adding partials l, l + 64, ... in index order, then the shuffle tree (flat_grid_fold).
//     flat_reduce_blocks(n) fixes the number of partials and so the order: it must stay this function of n alone.
//   * K accumulators are interleaved in the workspace: partial[K * block + k].
//   * a body decides what it loads and stores: a path that must not touch an array (a bit copy, a skip range, "g is not written when
//     nothing is added") simply does not call load / store for it.
//   * nothing that includes this header may be built with fast-math.
// What is not shared: the min / max reduction of the Fisher normalisation (one user: ewc.hip keeps it), ewc_penalty_kernel's serial
// fold, the cosine kernels' (r0 + r1) + (r2 + r3) block stage (cosine.hip), and every grid formula but the reduction grid's.
#pragma once
#include "common.h"
#include <algorithm>

namespace ocl {

static constexpr int FLAT_THREADS = 256;
static constexpr int FLAT_MAX_BLOCKS = 512;

// the grid of a flat-array reduction (and of the EWC++ passes): a function of n alone, so that the partial sums, and with them the
// result, do not depend on the device or on the launch
static inline int flat_reduce_blocks(int64_t n) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(FLAT_MAX_BLOCKS, ((n >> 2) + FLAT_THREADS - 1) / FLAT_THREADS));
}

// ---- device: the streaming loop ----------------------------------------------------------------------------------------------------
template <int W>
struct FlatVals {
    float v[W];
    __device__ __forceinline__ float& operator[](int k) { return v[k]; }
    __device__ __forceinline__ float operator[](int k) const { return v[k]; }
};

// W consecutive elements from element index `e` on (W == 4: e is a multiple of 4 and the arrays are 16-byte aligned)
template <int W_>
struct FlatAccess {
    static constexpr int W = W_;
    int64_t e;
    __device__ __forceinline__ FlatVals<W> load(const float* p) const {
        if constexpr (W == 4) {
            const float4 t = *(const float4*)(p + e);
            return {{t.x, t.y, t.z, t.w}};
        } else {
            return {{p[e]}};
        }
    }
    __device__ __forceinline__ void store(float* p, const FlatVals<W>& a) const {
        if constexpr (W == 4) *(float4*)(p + e) = make_float4(a[0], a[1], a[2], a[3]);
        else p[e] = a[0];
    }
};

// body(FlatAccess<4>) for this thread's float4 groups, then body(FlatAccess<1>) for its tail elements; `body` is a generic lambda
template <class Body>
__device__ __forceinline__ void flat_for_each(int64_t n, Body&& body) {
    const int64_t n4 = n >> 2;
    // (the builtin, not blockDim.x: inside a device function blockDim.x is lowered for a grid whose last block may be partial, a
    // vector load and a select at the head of every wave, which the kernels' own loops did not pay)
    const int64_t threads = __builtin_amdgcn_workgroup_size_x();
    const int64_t stride = (int64_t)gridDim.x * threads;
    const int64_t first = (int64_t)blockIdx.x * threads + threadIdx.x;
    for (int64_t i = first; i < n4; i += stride) body(FlatAccess<4>{i << 2});
    for (int64_t i = (n4 << 2) + first; i < n; i += stride) body(FlatAccess<1>{i});
}

// ---- device: the two stages of a sum over the grid ---------------------------------------------------------------------------------
// block stage: every thread's K accumulators -> partial[K * blockIdx.x + k]
template <int K>
__device__ __forceinline__ void flat_block_partial(double (&acc)[K], double* __restrict__ partial) {
    __shared__ double red[K][FLAT_THREADS / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        acc[k] = wave_sum_d(acc[k]);
        if (lane == 0) red[k][wid] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = red[k][0];
            for (int w = 1; w < FLAT_THREADS / 64; ++w) s += red[k][w];
            partial[K * blockIdx.x + k] = s;
        }
    }
}

// grid stage: the nb blocks' partials -> tot[k], the same K doubles in every thread of every block.  At most 8 dependent adds per lane
// and the shuffle tree, not nb adds on one thread while 255 wait.
template <int K>
__device__ __forceinline__ void flat_grid_fold(const double* __restrict__ partial, int nb, double (&tot)[K]) {
    __shared__ double bc[K];
    if (threadIdx.x < 64) {
        double a[K] = {};
        for (int b = threadIdx.x; b < nb; b += 64) {
#pragma unroll
            for (int k = 0; k < K; ++k) a[k] += partial[K * b + k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            a[k] = wave_sum_d(a[k]);
            if (threadIdx.x == 0) bc[k] = a[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) tot[k] = bc[k];
}

// ---- host: the argument check of an entry point ------------------------------------------------------------------------------------
struct FlatArg {
    const void* ptr;
    const char* name;
};

// n float32 elements behind each of the first `count` pointers: none null, 0 < n <= UINTPTR_MAX / 8, all 16-byte aligned, pairwise
// disjoint.  Sets the error text "<op>: ..." and returns OCL_ERR_ARG, or returns OCL_OK.
template <int N>
static inline int flat_check_args(const char* op, int64_t n, const FlatArg (&args)[N], int count = N) {
    for (int i = 0; i < count; ++i) OCL_REQUIRE(args[i].ptr != nullptr, "%s: null pointer (%s)", op, args[i].name);
    OCL_REQUIRE(n > 0, "%s: n=%lld (must be > 0)", op, (long long)n);
    OCL_REQUIRE(n <= (int64_t)(UINTPTR_MAX / 8), "%s: n=%lld is too large", op, (long long)n);
    for (int i = 0; i < count; ++i) OCL_REQUIRE(((uintptr_t)args[i].ptr % 16) == 0, "%s: %s must be 16-B aligned", op, args[i].name);
    const size_t bytes = (size_t)n * 4;
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            OCL_REQUIRE(!ranges_overlap(args[i].ptr, bytes, args[j].ptr, bytes), "%s: %s and %s overlap", op, args[i].name, args[j].name);
    return OCL_OK;
}

}  // namespace ocl
