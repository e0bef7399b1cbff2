// K9: gather / scatter of replay-buffer rows by an int64 index vector.  HBM-bound copies: 16-byte units where the row size and the
// pointers allow, 4-byte units otherwise, a long row spread over grid.y.
#include "small_ops.h"

using namespace ocl;

static unsigned rows_grid_y(int64_t units) { return (unsigned)max((int64_t)1, min((int64_t)8, (units + 1023) / 1024)); }

namespace ocl {
SPlan plan_rows(const void* src, const void* dst, int64_t row_bytes, int64_t n) {
    const bool v16 = (row_bytes % 16) == 0 && aligned16(src, dst);
    const unsigned gy = rows_grid_y(row_bytes / (v16 ? 16 : 4));
    const int path = v16 ? (gy == 8 ? OCL_PATH_ROWS_COPY16_YCAP : OCL_PATH_ROWS_COPY16) : (gy == 8 ? OCL_PATH_ROWS_COPY4_YCAP : OCL_PATH_ROWS_COPY4);
    return splan(path, (unsigned)n, gy, 256);
}
SPlan plan_pair(const void* src_a, const void* dst_a, int64_t row_bytes_a, int64_t row_bytes_b, int64_t n) {
    const bool v16 = (row_bytes_a % 16) == 0 && aligned16(src_a, dst_a);
    if (!v16) {   // two rows_copy launches (each planned by plan_rows from its own pointers)
        SPlan p = splan(OCL_PATH_PAIR_FALLBACK, (unsigned)n, rows_grid_y(row_bytes_a / 4), 256);
        p.grid2_x = (unsigned)n; p.block2 = 256;
        return p;
    }
    return splan(row_bytes_b / 4 > 256 ? OCL_PATH_PAIR_FUSED_BLOOP : OCL_PATH_PAIR_FUSED, (unsigned)n, rows_grid_y(row_bytes_a / 16), 256);
}
}  // namespace ocl

// =====================================================================================================
// K9 gather / scatter of replay-buffer rows
// =====================================================================================================
template <bool SCATTER>
__global__ void __launch_bounds__(256) rows_copy16(const uint4* __restrict__ src, const int64_t* __restrict__ idx,
                                                   uint4* __restrict__ dst, int64_t units) {
    const int64_t r = blockIdx.x;
    const int64_t row = idx[r];
    const uint4* s = SCATTER ? src + r * units : src + row * units;
    uint4* d = SCATTER ? dst + row * units : dst + r * units;
    for (int64_t u = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.y * blockDim.x)
        d[u] = s[u];
}
template <bool SCATTER>
__global__ void __launch_bounds__(256) rows_copy4(const uint32_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                  uint32_t* __restrict__ dst, int64_t units) {
    const int64_t r = blockIdx.x;
    const int64_t row = idx[r];
    const uint32_t* s = SCATTER ? src + r * units : src + row * units;
    uint32_t* d = SCATTER ? dst + row * units : dst + r * units;
    for (int64_t u = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.y * blockDim.x)
        d[u] = s[u];
}

template <bool SCATTER>
static int rows_copy(const void* src, const int64_t* idx, int64_t n, int64_t row_bytes, void* dst, void* stream) {
    OCL_REQUIRE(n >= 0 && row_bytes > 0 && (row_bytes % 4) == 0, "rows_copy: n=%lld row_bytes=%lld (must be >0, %%4)",
                (long long)n, (long long)row_bytes);
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(src && idx && dst, "rows_copy: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_rows(src, dst, row_bytes, n);
    const dim3 grid(pl.grid_x, pl.grid_y);
    if (pl.path == OCL_PATH_ROWS_COPY16 || pl.path == OCL_PATH_ROWS_COPY16_YCAP)
        hipLaunchKernelGGL(rows_copy16<SCATTER>, grid, dim3(pl.block), 0, s, (const uint4*)src, idx, (uint4*)dst, row_bytes / 16);
    else
        hipLaunchKernelGGL(rows_copy4<SCATTER>, grid, dim3(pl.block), 0, s, (const uint32_t*)src, idx, (uint32_t*)dst, row_bytes / 4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// rows of TWO arrays by one index vector in one launch (replay-buffer images + their labels: every retrieval of the reference is the
// pair buffer_img[indices], buffer_label[indices]): a in 16-byte units over grid.y, b (a few bytes per row) by the first block of the row
__global__ void __launch_bounds__(256) rows_gather_pair(const uint4* __restrict__ a, uint4* __restrict__ da, int64_t units_a,
                                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ db, int64_t units_b,
                                                        const int64_t* __restrict__ idx) {
    const int64_t r = blockIdx.x;
    const int64_t row = idx[r];
    for (int64_t u = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; u < units_a; u += (int64_t)gridDim.y * blockDim.x)
        da[r * units_a + u] = a[row * units_a + u];
    if (blockIdx.y == 0)
        for (int64_t u = threadIdx.x; u < units_b; u += blockDim.x) db[r * units_b + u] = b[row * units_b + u];
}

int ocl_gather_rows(const void* src, const int64_t* idx, int64_t n, int64_t row_bytes, void* dst, void* stream) {
    return rows_copy<false>(src, idx, n, row_bytes, dst, stream);
}
int ocl_scatter_rows(void* dst, const int64_t* idx, int64_t n, int64_t row_bytes, const void* src, void* stream) {
    return rows_copy<true>(src, idx, n, row_bytes, dst, stream);
}

int ocl_gather_rows_pair(const void* src_a, int64_t row_bytes_a, void* dst_a, const void* src_b, int64_t row_bytes_b, void* dst_b,
                         const int64_t* idx_host, int64_t* idx_dev, int64_t n, void* stream) {
    OCL_REQUIRE(n >= 0 && row_bytes_a > 0 && row_bytes_b > 0 && (row_bytes_a % 4) == 0 && (row_bytes_b % 4) == 0,
                "gather_rows_pair: n=%lld row bytes %lld / %lld (must be > 0, %%4)", (long long)n, (long long)row_bytes_a, (long long)row_bytes_b);
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(src_a && dst_a && src_b && dst_b && idx_dev, "gather_rows_pair: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (idx_host) {   // the index vector was built on the host (numpy / torch-CPU RNG draws): upload it here, through the staging ring
        int rc = ocl::upload_small(idx_host, (size_t)n * sizeof(int64_t), idx_dev, s);
        if (rc != OCL_OK) return rc;
    }
    const SPlan pl = plan_pair(src_a, dst_a, row_bytes_a, row_bytes_b, n);
    if (pl.path == OCL_PATH_PAIR_FALLBACK) {
        int rc = rows_copy<false>(src_a, idx_dev, n, row_bytes_a, dst_a, stream);
        if (rc != OCL_OK) return rc;
        return rows_copy<false>(src_b, idx_dev, n, row_bytes_b, dst_b, stream);
    }
    ProfScope ps(PROF_KNN, s);
    hipLaunchKernelGGL(rows_gather_pair, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), 0, s, (const uint4*)src_a, (uint4*)dst_a, row_bytes_a / 16,
                       (const uint32_t*)src_b, (uint32_t*)dst_b, row_bytes_b / 4, idx_dev);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
