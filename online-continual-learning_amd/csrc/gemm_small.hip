// The small exact-fp32 MFMA GEMM of the head (net.hip calls it through the C entry point) and of ops.py.
#include "small_ops.h"

using namespace ocl;

// =====================================================================================================
// small exact-fp32 MFMA GEMM: one wave per 16x16 tile of C, arbitrary strides
// lane l: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; D: col=l&15, row=(l>>4)*4+reg  (v_mfma_f32_16x16x4_f32)
// =====================================================================================================
namespace ocl {
SPlan plan_gemm(int m, int n, int k) {
    return splan(k % 16 == 0 ? OCL_PATH_GEMM_K16 : k < 16 ? OCL_PATH_GEMM_KTAIL : OCL_PATH_GEMM_KBOTH, (unsigned)cdiv(n, 16), (unsigned)cdiv(m, 16), 64);
}
}  // namespace ocl

__global__ void __launch_bounds__(64) gemm_small_kernel(const float* __restrict__ a, int64_t a_rs, int64_t a_cs,
                                                        const float* __restrict__ b, int64_t b_rs, int64_t b_cs,
                                                        float* __restrict__ c, int64_t c_rs, int m, int n, int k,
                                                        const float* __restrict__ bias, int relu, int accumulate) {
    const int lane = threadIdx.x;
    const int r16 = lane & 15, g = lane >> 4;
    const int row0 = blockIdx.y * 16, col0 = blockIdx.x * 16;
    const int ar = row0 + r16, bc = col0 + r16;
    const bool av = ar < m, bv = bc < n;
    const float* ap = a + (int64_t)(av ? ar : 0) * a_rs;
    const float* bp = b + (int64_t)(bv ? bc : 0) * b_cs;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 16 <= k; k0 += 16) {
        float av4[4], bv4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kk = k0 + u * 4 + g;
            av4[u] = av ? ap[(int64_t)kk * a_cs] : 0.f;
            bv4[u] = bv ? bp[(int64_t)kk * b_rs] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av4[u], bv4[u], acc, 0, 0, 0);
    }
    for (; k0 < k; k0 += 4) {
        const int kk = k0 + g;
        const float x = (av && kk < k) ? ap[(int64_t)kk * a_cs] : 0.f;
        const float y = (bv && kk < k) ? bp[(int64_t)kk * b_rs] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0);
    }
    const int col = col0 + r16;
    if (col < n) {
        const float bs = bias ? bias[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + g * 4 + r;
            if (row < m) {
                float v = acc[r] + bs;
                float* cp = c + (int64_t)row * c_rs + col;
                if (accumulate) v += *cp;
                if (relu) v = fmaxf(v, 0.f);
                *cp = v;
            }
        }
    }
}

int ocl_gemm_small(const float* a, int64_t a_rs, int64_t a_cs, const float* b, int64_t b_rs, int64_t b_cs, float* c,
                   int64_t c_rs, int m, int n, int k, const float* bias, int relu, int accumulate, void* stream) {
    OCL_REQUIRE(a && b && c && m > 0 && n > 0 && k > 0, "gemm_small: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const SPlan pl = plan_gemm(m, n, k);
    hipLaunchKernelGGL(gemm_small_kernel, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), 0, s, a, a_rs, a_cs, b, b_rs, b_cs, c, c_rs, m,
                       n, k, bias, relu, accumulate);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
