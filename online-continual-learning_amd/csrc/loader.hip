// K9b: the mini-batch of a task whose images are already float (the reference's new-instance streams, continuum/non_stationary.py: HWC
// arrays divided by 255 on the host).  dataset_transform.__getitem__ on such an array (continuum/data_utils.py:47-54) is ToTensor's
// transpose HWC -> CHW and nothing else, so the kernel moves bits: rows of a device-resident float32 [N, H, W, C] task chosen by an int64
// index vector, written as [n, C, H, W].  The sibling of gather_u8_hwc_f32_chw (at the end of this file), without its division.
//
// Two forms, chosen on the host:
//   tile    a row's float count is a multiple of 4, the task's base is 16-byte aligned (so every row is) and C <= LD_MAX_C: a workgroup
//           takes 256 pixels at a time, reads their 256 * C interleaved floats with 16-byte loads into LDS (a tile starts at a multiple
//           of 256 * C floats and ends at the row's end, both multiples of 4), and writes channel after channel from there, one
//           pixel per lane: loads and stores both run over consecutive addresses.
//   scalar  anything else: output-linear, one 4-byte load per element at stride C (the u8 kernel's form).
// The values travel as 32-bit words, never through a floating-point instruction: NaN payloads, -0.0 and denormals keep their bits.
#include "small_ops.h"

using namespace ocl;

static constexpr int LD_TILE = 256;     // pixels per tile = threads per workgroup
static constexpr int LD_MAX_C = 16;     // channels the tile form holds in LDS (16 KB)
static constexpr int LD_MAX_Y = 16;     // workgroups per row (each loops over its tiles)

__global__ void __launch_bounds__(LD_TILE) gather_f32_hwc_f32_chw_kernel(const uint32_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                                         int64_t hw, int c, uint32_t* __restrict__ dst) {
    extern __shared__ uint4 ld_tile4[];
    uint32_t* tile = (uint32_t*)ld_tile4;
    const int64_t r = blockIdx.x, per = hw * c;
    const uint32_t* s = src + idx[r] * per;
    uint32_t* d = dst + r * per;
    const int64_t n_tiles = (hw + LD_TILE - 1) / LD_TILE;
    for (int64_t t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        const int64_t p0 = t * LD_TILE;
        const int np = (int)min((int64_t)LD_TILE, hw - p0);
        const int nf4 = (np * c) >> 2;   // (np * c is a multiple of 4: see the header)
        const uint4* s4 = (const uint4*)(s + p0 * c);
        for (int u = threadIdx.x; u < nf4; u += LD_TILE) ld_tile4[u] = s4[u];
        __syncthreads();
        if ((int)threadIdx.x < np)
            for (int ch = 0; ch < c; ++ch) d[ch * hw + p0 + threadIdx.x] = tile[threadIdx.x * c + ch];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) gather_f32_hwc_f32_chw_scalar_kernel(const uint32_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                                            int64_t hw, int c, uint32_t* __restrict__ dst) {
    const int64_t r = blockIdx.x, per = hw * c;
    const uint32_t* s = src + idx[r] * per;
    uint32_t* d = dst + r * per;
    for (int64_t o = threadIdx.x + (int64_t)blockIdx.y * blockDim.x; o < per; o += (int64_t)blockDim.x * gridDim.y) {
        const int64_t ch = o / hw, p = o - ch * hw;
        d[o] = s[p * c + ch];
    }
}

int ocl_gather_f32_hwc_to_f32_chw(const float* src, const int64_t* idx, int64_t n, int h, int w, int c, float* dst, void* stream) {
    OCL_REQUIRE(n >= 0 && n <= 0x7fffffff && h > 0 && w > 0 && c > 0, "gather_f32: bad shape (n=%lld h=%d w=%d c=%d)", (long long)n, h, w, c);
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(src && idx && dst, "gather_f32: null pointer");
    OCL_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "gather_f32: src and dst must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const int64_t hw = (int64_t)h * w, per = hw * c;
    const bool tiled = (per & 3) == 0 && ((uintptr_t)src & 15) == 0 && c <= LD_MAX_C;
    if (tiled) {
        const unsigned gy = (unsigned)min((int64_t)LD_MAX_Y, (hw + LD_TILE - 1) / LD_TILE);
        hipLaunchKernelGGL(gather_f32_hwc_f32_chw_kernel, dim3((unsigned)n, gy), dim3(LD_TILE), (size_t)LD_TILE * c * sizeof(uint32_t), s,
                           (const uint32_t*)src, idx, hw, c, (uint32_t*)dst);
    } else {
        const unsigned gy = (unsigned)max((int64_t)1, min((int64_t)LD_MAX_Y, (per + 2047) / 2048));
        hipLaunchKernelGGL(gather_f32_hwc_f32_chw_scalar_kernel, dim3((unsigned)n, gy), dim3(256), 0, s, (const uint32_t*)src, idx, hw, c,
                           (uint32_t*)dst);
    }
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// The uint8 sibling: rows of a device-resident uint8 [N, H, W, C] task, ToTensor's transpose and its division by 255
namespace ocl {
SPlan plan_u8(int64_t n, int h, int w, int c) {
    const int64_t per = (int64_t)h * w * c;
    return splan(OCL_PATH_U8_GATHER, (unsigned)n, (unsigned)max((int64_t)1, min((int64_t)16, (per + 2047) / 2048)), 256);
}
}  // namespace ocl

__global__ void __launch_bounds__(256) gather_u8_hwc_f32_chw(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                             int h, int w, int c, float* __restrict__ dst) {
    const int64_t r = blockIdx.x;
    const int64_t hw = (int64_t)h * w, per = hw * c;
    const uint8_t* s = src + idx[r] * per;
    float* d = dst + r * per;
    // output-linear so stores coalesce; the u8 reads hit L1/L2 (3 KB / 21 KB per image)
    for (int64_t o = threadIdx.x + (int64_t)blockIdx.y * blockDim.x; o < per; o += (int64_t)blockDim.x * gridDim.y) {
        const int64_t ch = o / hw, p = o - ch * hw;
        d[o] = (float)s[p * c + ch] / 255.0f;  // ToTensor: .float().div(255)
    }
}

int ocl_gather_u8_hwc_to_f32_chw(const uint8_t* src, const int64_t* idx, int64_t n, int h, int w, int c, float* dst,
                                 void* stream) {
    OCL_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "gather_u8: bad shape");
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(src && idx && dst, "gather_u8: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_u8(n, h, w, c);
    hipLaunchKernelGGL(gather_u8_hwc_f32_chw, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), 0, s, src, idx, h, w, c, dst);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
