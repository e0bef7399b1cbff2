// The small kernels around the convolutions: weight packing, NCHW -> NHWC input conversion, average pool, L2 normalisation, ReLU backward,
// column sum, fill -- and their launchers.
#include "conv_dev.h"
#include <algorithm>
#include <cmath>

namespace ocl {

// =====================================================================================================
// weight packing (all conv layers in one launch)
// =====================================================================================================
__global__ void __launch_bounds__(256) pack_weights_kernel(const float* __restrict__ params, float* __restrict__ arena,
                                                           const PackDesc* __restrict__ descs, int mask, int n_layers, StatCell* __restrict__ zero_a,
                                                           int64_t zero_a_n, StatCell* __restrict__ zero_b, int64_t zero_b_n) {
    if ((int)blockIdx.y >= n_layers) {   // the last grid row clears the statistics arenas of the pass (saves two memset launches)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < zero_a_n + zero_b_n; i += (int64_t)gridDim.x * blockDim.x) {
            StatCell z;
            z.lo = 0ull; z.hi = 0ll;
            if (i < zero_a_n) zero_a[i] = z;
            else zero_b[i - zero_a_n] = z;
        }
        return;
    }
    PackDesc d = descs[blockIdx.y];
    // a pass writes only the packs it reads (PACK_* bits).  The threads walk the PACKS in storage order -- rows of Cout x 4 (forward) /
    // Cin x 4 (data gradient) consecutive floats, coalesced stores -- and gather from the OIHW tensor (read-only, 36-byte strides: served by
    // L2); walking the tensor and scattering 4-byte stores into both packs was 13 us at the head of every step's chain.  Padding rows /
    // columns of a pack are never written (zero since the arena was created).
    if (!(mask & PACK_TF)) d.tf_off = -1;
    if (!(mask & PACK_TD)) d.td_off = -1;
    const int ci4n = (d.Cin + 3) >> 2;
    const int nF = d.tf_off >= 0 ? d.ntaps * ci4n * d.Cout * 4 : 0;
    const int nD = d.td_off >= 0 ? d.ntaps * d.Cout * d.Cin : 0;   // (Cout is a multiple of 4)
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nF + nD; e += gridDim.x * blockDim.x) {
        if (e < nF) {   // [t][ci >> 2][co][ci & 3]
            const int k = e & 3, r = e >> 2;
            const int co = r % d.Cout, r2 = r / d.Cout;
            const int c4 = r2 % ci4n, t = r2 / ci4n;
            const int ci = c4 * 4 + k;
            if (ci < d.Cin)
                arena[d.tf_off + ((((int64_t)t * (d.CinP >> 2) + c4) * d.CoutP + co) << 2) + k] = params[d.w_off + ((int64_t)co * d.Cin + ci) * d.ntaps + t];
        } else {        // [t][co >> 2][ci][co & 3]
            const int f = e - nF;
            const int k = f & 3, r = f >> 2;
            const int ci = r % d.Cin, r2 = r / d.Cin;
            const int o4 = r2 % (d.Cout >> 2), t = r2 / (d.Cout >> 2);
            const int co = o4 * 4 + k;
            arena[d.td_off + ((((int64_t)t * (d.Cout >> 2) + o4) * d.CiP + ci) << 2) + k] = params[d.w_off + ((int64_t)co * d.Cin + ci) * d.ntaps + t];
        }
    }
}

int launch_pack_weights(const float* params, float* arena, const PackDesc* descs_dev, int n_layers, int max_elems, hipStream_t s,
                        int mask, StatCell* zero_a, int64_t zero_a_n, StatCell* zero_b, int64_t zero_b_n) {
    ProfScope ps(PROF_BN, s);
    const int extra = (zero_a_n + zero_b_n) > 0 ? 1 : 0;
    // (up to 256 workgroups per layer: layer 4's 230 k weights in 4 passes per thread instead of 14)
    hipLaunchKernelGGL(pack_weights_kernel, dim3(std::min(512, cdiv(2 * max_elems, 256)), n_layers + extra), dim3(256), 0, s, params, arena,
                       descs_dev, mask, n_layers, zero_a, zero_a_n, zero_b, zero_b_n);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// =====================================================================================================
// layout
// =====================================================================================================
__global__ void __launch_bounds__(256) nchw3_to_nhwc4_kernel(const float* __restrict__ x, float4* __restrict__ out, int HW,
                                                             int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / HW;
        const int p = (int)(i - n * HW);
        const float* b = x + n * 3 * HW + p;
        out[i] = make_float4(b[0], b[HW], b[2 * (int64_t)HW], 0.f);
    }
}
int launch_nchw3_to_nhwc4(const float* x, float* out, int N, int H, int W, hipStream_t s) {
    const int64_t total = (int64_t)N * H * W;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3((unsigned)std::min<int64_t>(2048, (total + 255) / 256)), dim3(256), 0, s, x,
                       (float4*)out, H * W, total);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
// the same from up to kMaxInputSegments separate [n_i, 3, H, W] tensors that together form the batch (memory rows + stream batch +
// augmented views: the reference's torch.cat((mem_x, batch_x)) and the per-view forward calls, without materialising the concatenation)
__global__ void __launch_bounds__(256) nchw3_to_nhwc4_seg_kernel(const InputSegments sg, float4* __restrict__ out, int HW, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / HW);
        const int p = (int)(i - (int64_t)n * HW);
        int k = 0;
#pragma unroll
        for (int j = 1; j < kMaxInputSegments; ++j) k = (j < sg.n && n >= sg.first[j]) ? j : k;
        const float* xs = sg.x[0];
#pragma unroll
        for (int j = 1; j < kMaxInputSegments; ++j) xs = k == j ? sg.x[j] : xs;
        int f = sg.first[0];
#pragma unroll
        for (int j = 1; j < kMaxInputSegments; ++j) f = k == j ? sg.first[j] : f;
        const float* b = xs + (int64_t)(n - f) * 3 * HW + p;
        out[i] = make_float4(b[0], b[HW], b[2 * (int64_t)HW], 0.f);
    }
}
int launch_nchw3_to_nhwc4_segments(const InputSegments& sg, float* out, int N, int H, int W, hipStream_t s) {
    if (sg.n == 1) return launch_nchw3_to_nhwc4(sg.x[0], out, N, H, W, s);
    const int64_t total = (int64_t)N * H * W;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(nchw3_to_nhwc4_seg_kernel, dim3((unsigned)std::min<int64_t>(2048, (total + 255) / 256)), dim3(256), 0, s, sg,
                       (float4*)out, H * W, total);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// =====================================================================================================
// avg_pool2d(4) + flatten (C,ph,pw order), l2-normalise, misc
// =====================================================================================================
__global__ void __launch_bounds__(256) avgpool_fwd_kernel(const float* __restrict__ z, float* __restrict__ feat, int H, int W, int C,
                                                          int PH, int PW) {
    const int n = blockIdx.x;
    const int D = C * PH * PW;
    for (int o = threadIdx.x; o < D; o += blockDim.x) {
        const int c = o / (PH * PW), r = o - c * PH * PW;
        const int ph = r / PW, pw = r - ph * PW;
        float s = 0.f;
        for (int dy = 0; dy < 4; ++dy)
            for (int dx = 0; dx < 4; ++dx) s += z[(((int64_t)n * H + ph * 4 + dy) * W + pw * 4 + dx) * C + c];
        feat[(int64_t)n * D + o] = s * (1.0f / 16.0f);
    }
}
__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ dfeat, float* __restrict__ dz, int H, int W, int C,
                                                          int PH, int PW) {
    const int n = blockIdx.x;
    const int D = C * PH * PW;
    const int total = H * W * C;
    for (int e = threadIdx.x + blockIdx.y * blockDim.x; e < total; e += blockDim.x * gridDim.y) {
        const int c = e % C, p = e / C;
        const int y = p / W, x = p - y * W;
        float v = 0.f;
        if (y < PH * 4 && x < PW * 4) v = dfeat[(int64_t)n * D + c * PH * PW + (y >> 2) * PW + (x >> 2)] * (1.0f / 16.0f);
        dz[(int64_t)n * total + e] = v;
    }
}
int launch_avgpool_fwd(const float* z, float* feat, int N, int H, int W, int C, hipStream_t s) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(N), dim3(256), 0, s, z, feat, H, W, C, H / 4, W / 4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
int launch_avgpool_bwd(const float* dfeat, float* dz, int N, int H, int W, int C, hipStream_t s) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(N, std::max(1, std::min(8, cdiv(H * W * C, 2048)))), dim3(256), 0, s, dfeat, dz, H,
                       W, C, H / 4, W / 4);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

__global__ void __launch_bounds__(64) l2norm_fwd_kernel(const float* __restrict__ v, float* __restrict__ out, float* __restrict__ norms,
                                                        int d, float* __restrict__ out2) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* p = v + (int64_t)n * d;
    float ss = 0.f;
    for (int j = lane; j < d; j += 64) ss = fmaf(p[j], p[j], ss);
    ss = wave_sum(ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize eps
    if (lane == 0) norms[n] = nrm;
    for (int j = lane; j < d; j += 64) {
        const float q = p[j] / nrm;
        out[(int64_t)n * d + j] = q;
        if (out2) out2[(int64_t)n * d + j] = q;   // the caller's tensor (saves a device-to-device copy launch)
    }
}
__global__ void __launch_bounds__(64) l2norm_bwd_kernel(const float* __restrict__ out, const float* __restrict__ norms,
                                                        const float* __restrict__ dout, float* __restrict__ dv, int d) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* o = out + (int64_t)n * d;
    const float* g = dout + (int64_t)n * d;
    float dot = 0.f;
    for (int j = lane; j < d; j += 64) dot = fmaf(o[j], g[j], dot);
    dot = wave_sum(dot);
    const float inv = 1.0f / norms[n];
    for (int j = lane; j < d; j += 64) dv[(int64_t)n * d + j] = (g[j] - o[j] * dot) * inv;
}
int launch_l2norm_fwd(const float* v, float* out, float* norms, int n, int d, hipStream_t s, float* out2) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(n), dim3(64), 0, s, v, out, norms, d, out2);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
int launch_l2norm_bwd(const float* out, const float* norms, const float* dout, float* dv, int n, int d, hipStream_t s) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(n), dim3(64), 0, s, out, norms, dout, dv, d);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

__global__ void __launch_bounds__(256) relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a, float* __restrict__ dx,
                                                       int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dx[i] = a[i] > 0.f ? dy[i] : 0.f;
}
int launch_relu_bwd(const float* dy, const float* a, float* dx, int64_t n, hipStream_t s) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, s, dy, a, dx, n);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

// out[c] (+)= sum_r m[r][c]: 32 columns x 8 row lanes per workgroup, lane sums combined through LDS in a fixed order
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ m, int rows, int cols, float* __restrict__ out,
                                                     int accumulate) {
    __shared__ float red[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s = 0.f;
    if (c < cols)
        for (int r = rl; r < rows; r += 8) s += m[(int64_t)r * cols + c];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < cols) {
        const float v = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
        out[c] = accumulate ? out[c] + v : v;
    }
}
int launch_colsum(const float* m, int rows, int cols, float* out, int accumulate, hipStream_t s) {
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 32)), dim3(256), 0, s, m, rows, cols, out, accumulate);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

__global__ void __launch_bounds__(256) fill_kernel(float* __restrict__ p, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}
int launch_fill(float* p, int64_t n, float v, hipStream_t s) {
    if (n <= 0) return OCL_OK;
    ProfScope ps(PROF_HEAD, s);
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, s, p, n, v);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

}  // namespace ocl
