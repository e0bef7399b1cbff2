// K11: the nearest-class-mean classifier: class means of the normalised buffer features, then the nearest mean of each test feature.
#include "small_ops.h"
#include <math.h>

using namespace ocl;

// =====================================================================================================
// K11 NCM (agents/base.py:121-142, 159-176)
// =====================================================================================================
namespace ocl {
SPlan plan_ncm_means(int d, int n_cls) { return splan(OCL_PATH_NCM_MEANS, (unsigned)n_cls, 1, 256, (int64_t)d * 8 + 64); }
SPlan plan_ncm_predict(int n, int d, int n_cls) { return splan(OCL_PATH_NCM_PREDICT, (unsigned)n, 1, 256, (int64_t)(d + n_cls + 16) * 4); }
}  // namespace ocl

__global__ void __launch_bounds__(256) ncm_means_kernel(const float* __restrict__ feat, const int64_t* __restrict__ labels, int n,
                                                        int d, const int64_t* __restrict__ class_ids, float* __restrict__ means,
                                                        int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw3[];
    double* acc = (double*)smraw3;      // d
    float* red = (float*)(acc + d);     // 16
    const int c = blockIdx.x;
    const int64_t cls = class_ids[c];
    for (int j = threadIdx.x; j < d; j += blockDim.x) acc[j] = 0.0;
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        if (labels[i] != cls) continue;  // uniform across the workgroup
        const float* f = feat + (int64_t)i * d;
        float ss = 0.f;
        for (int j = threadIdx.x; j < d; j += blockDim.x) ss = fmaf(f[j], f[j], ss);
        ss = block_sum(ss, red);
        const float nrm = sqrtf(ss);
        for (int j = threadIdx.x; j < d; j += blockDim.x) acc[j] += (double)(f[j] / nrm);
        ++cnt;
    }
    if (threadIdx.x == 0 && counts) counts[c] = cnt;
    if (cnt == 0) return;
    __syncthreads();
    float ss = 0.f;
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
        const float mu = (float)(acc[j] / (double)cnt);
        ss = fmaf(mu, mu, ss);
    }
    ss = block_sum(ss, red);
    const float nrm = sqrtf(ss);
    for (int j = threadIdx.x; j < d; j += blockDim.x) means[(int64_t)c * d + j] = (float)(acc[j] / (double)cnt) / nrm;
}

__global__ void __launch_bounds__(256) ncm_predict_kernel(const float* __restrict__ feat, int d, const float* __restrict__ means,
                                                          int n_cls, int64_t* __restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* fn = smf;            // d
    float* dist = smf + d;      // n_cls
    float* red = dist + n_cls;  // 16
    const int i = blockIdx.x;
    const float* f = feat + (int64_t)i * d;
    float ss = 0.f;
    for (int j = threadIdx.x; j < d; j += blockDim.x) ss = fmaf(f[j], f[j], ss);
    ss = block_sum(ss, red);
    const float nrm = sqrtf(ss);
    for (int j = threadIdx.x; j < d; j += blockDim.x) fn[j] = f[j] / nrm;
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int c = wid; c < n_cls; c += nw) {
        const float* mu = means + (int64_t)c * d;
        float s = 0.f;
        for (int j = lane; j < d; j += 64) {
            const float t = fn[j] - mu[j];
            s = fmaf(t, t, s);
        }
        s = wave_sum(s);
        if (lane == 0) dist[c] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        float bv = dist[0];
        for (int c = 1; c < n_cls; ++c)
            if (dist[c] < bv || (dist[c] != dist[c] && bv == bv)) {   // the first NaN wins and stays (torch.min), else the first minimum
                bv = dist[c];
                best = c;
            }
        pred[i] = best;
    }
}

int ocl_ncm_class_means(const float* feat, const int64_t* labels, int n, int d, const int64_t* class_ids, int n_cls,
                        float* means_out, int32_t* counts_out, void* stream) {
    OCL_REQUIRE(feat && labels && class_ids && means_out && n >= 0 && d > 0 && n_cls > 0, "ncm_means: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_ncm_means(d, n_cls);
    hipLaunchKernelGGL(ncm_means_kernel, dim3(pl.grid_x), dim3(pl.block), (size_t)pl.lds_bytes, s, feat, labels, n, d, class_ids, means_out,
                       counts_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_ncm_predict(const float* feat, int n, int d, const float* means, int n_cls, int64_t* pred_out, void* stream) {
    OCL_REQUIRE(n >= 0 && d > 0 && n_cls > 0, "ncm_predict: bad sizes");
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(feat && means && pred_out, "ncm_predict: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_ncm_predict(n, d, n_cls);
    hipLaunchKernelGGL(ncm_predict_kernel, dim3(pl.grid_x), dim3(pl.block), (size_t)pl.lds_bytes, s, feat, d, means, n_cls, pred_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
