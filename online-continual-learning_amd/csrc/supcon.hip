// K7: the supervised contrastive loss of SCR and its gradient w.r.t. the features, in two launches: one workgroup per anchor row, then
// the symmetrised sum over the coefficient matrix.
#include "small_ops.h"
#include <math.h>
#include <algorithm>

using namespace ocl;

// the in-kernel predicate of supcon_rows' 16-byte dot product (plan_supcon answers from the same expression)
__host__ __device__ __forceinline__ bool supcon_vec(const float* feat, int dim) { return (dim & 3) == 0 && (((uintptr_t)feat) & 15) == 0; }
// (the size and form variants of a path are consecutive codes: plan_cosine and plan_supcon add an offset to the first)
static_assert(OCL_PATH_SUPCON_VEC_NOTAIL == OCL_PATH_SUPCON_VEC_TAIL + 1 && OCL_PATH_SUPCON_VEC_LOSS == OCL_PATH_SUPCON_VEC_TAIL + 2 &&
              OCL_PATH_SUPCON_SCALAR_NOTAIL == OCL_PATH_SUPCON_SCALAR_TAIL + 1 && OCL_PATH_SUPCON_SCALAR_LOSS == OCL_PATH_SUPCON_SCALAR_TAIL + 2, "supcon path codes");
namespace ocl {
SPlan plan_supcon(const float* feat, int bsz, int n_views, int dim, bool want_grad) {
    const int64_t A = (int64_t)bsz * n_views;
    if (A > 8192 || dim > 4096) return splan(OCL_PATH_SUPCON_REFUSED);
    const int form = !want_grad ? 2 : (A % 16) ? 0 : 1;
    SPlan p = splan((supcon_vec(feat, dim) ? OCL_PATH_SUPCON_VEC_TAIL : OCL_PATH_SUPCON_SCALAR_TAIL) + form, (unsigned)A, 1, 256,
                    (int64_t)(dim + A + 16) * (int64_t)sizeof(float));
    p.grid2_x = want_grad ? (unsigned)A : 1u; p.block2 = 128;
    p.lds2_bytes = (int64_t)std::max<int64_t>(A, 128) * (int64_t)sizeof(float);
    return p;
}
}  // namespace ocl

// =====================================================================================================
// K7 SupCon (utils/loss.py:19-96), contrast_mode 'all'
// =====================================================================================================
// pass 1: one workgroup per anchor i. G[i][j] = d(mean loss)/d(logit_ij); rowloss[i] = loss_i.
__global__ void __launch_bounds__(256) supcon_rows(const float* __restrict__ feat, const int64_t* __restrict__ y, int bsz, int A,
                                                   int dim, float T, float* __restrict__ G, float* __restrict__ rowloss) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* fi = sm;            // dim
    float* lg = sm + dim;      // A logits
    float* red = lg + A;       // 16
    const int i = blockIdx.x;
    for (int d = threadIdx.x; d < dim; d += blockDim.x) fi[d] = feat[(int64_t)i * dim + d];
    __syncthreads();
    float m = -INFINITY;
    const bool vec = supcon_vec(feat, dim);
    for (int j = threadIdx.x; j < A; j += blockDim.x) {
        const float* fj = feat + (int64_t)j * dim;
        float dot = 0.f;
        if (vec) {   // 16-byte loads, four independent chains (one chain of `dim` FMAs behind 4-byte loads was most of this kernel's 10 us)
            const float4* fj4 = (const float4*)fj;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
            for (int d4 = 0; d4 < (dim >> 2); ++d4) {
                const float4 v = fj4[d4];
                const float4 e = *(const float4*)(fi + 4 * d4);
                a0 = fmaf(e.x, v.x, a0); a1 = fmaf(e.y, v.y, a1); a2 = fmaf(e.z, v.z, a2); a3 = fmaf(e.w, v.w, a3);
            }
            dot = (a0 + a1) + (a2 + a3);
        } else {
            for (int d = 0; d < dim; ++d) dot = fmaf(fi[d], fj[d], dot);
        }
        const float l = dot / T;
        lg[j] = l;
        m = fmaxf(m, l);  // reference takes the max over the full row, diagonal included (loss.py:71)
    }
    m = block_max(m, red);
    float se = 0.f;
    for (int j = threadIdx.x; j < A; j += blockDim.x)
        if (j != i) se += expf(lg[j] - m);
    se = block_sum(se, red);
    const float logden = logf(se);
    const int64_t yi = y[i % bsz];
    float sp = 0.f, np = 0.f;
    for (int j = threadIdx.x; j < A; j += blockDim.x) {
        if (j != i && y[j % bsz] == yi) {
            sp += (lg[j] - m) - logden;
            np += 1.f;
        }
    }
    sp = block_sum(sp, red);
    np = block_sum(np, red);
    if (threadIdx.x == 0) rowloss[i] = -(sp / np);  // 0/0 -> NaN like the reference (loss.py:90)
    if (G) {
        const float invA = 1.0f / (float)A, invden = 1.0f / se, invnp = 1.0f / np;
        // an anchor without a positive: the reference's autograd sends the 1/0 of loss.py:90 through the zero mask (0 * inf) into every
        // logit of the row, diagonal included; supcon_grad's symmetrised sum then spreads the NaN to every feature row, as autograd does
        const bool nopos = np == 0.f;
        for (int j = threadIdx.x; j < A; j += blockDim.x) {
            float g = nopos ? NAN : 0.f;
            if (j != i && !nopos) {
                const float p = expf(lg[j] - m) * invden;
                const float pos = (y[j % bsz] == yi) ? invnp : 0.f;
                g = (p - pos) * invA;
            }
            G[(int64_t)i * A + j] = g;
        }
    }
}
// pass 2: dfeat_i = (1/T) * sum_j (G[i][j] + G[j][i]) f_j ; block 0 also reduces the loss.
// The symmetrised coefficient row is staged in LDS first (the column read G[j][i] is strided: done once, in parallel),
// then threads run over the feature dimension with coalesced reads of f_j.
__global__ void __launch_bounds__(128) supcon_grad(const float* __restrict__ feat, int A, int dim, float T,
                                                   const float* __restrict__ G, const float* __restrict__ rowloss,
                                                   float* __restrict__ loss_out, float* __restrict__ dfeat) {
    extern __shared__ __attribute__((aligned(16))) float cf[];   // A coefficients
    const int i = blockIdx.x;
    if (dfeat) {
        for (int j = threadIdx.x; j < A; j += blockDim.x) cf[j] = G[(int64_t)i * A + j] + G[(int64_t)j * A + i];
        __syncthreads();
        for (int d = threadIdx.x; d < dim; d += blockDim.x) {
            // sixteen independent chains, sixteen loads in flight (a single chain of A = 220 dependent FMAs behind their loads was 18 us of
            // the SCR step's chain; four chains = 55 dependent L2 round trips: 17 us)
            float acc[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = 0.f;
            int j = 0;
            for (; j + 16 <= A; j += 16) {
                float v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = feat[(int64_t)(j + k) * dim + d];
#pragma unroll
                for (int k = 0; k < 16; ++k) acc[k] = fmaf(cf[j + k], v[k], acc[k]);
            }
            for (; j < A; ++j) acc[j & 15] = fmaf(cf[j], feat[(int64_t)j * dim + d], acc[j & 15]);
#pragma unroll
            for (int st = 8; st > 0; st >>= 1)
#pragma unroll
                for (int k = 0; k < st; ++k) acc[k] += acc[k + st];
            dfeat[(int64_t)i * dim + d] = acc[0] / T;
        }
    }
    if (i == 0) {   // mean of the row losses: every thread a strided share, then a tree over the workgroup (was one thread, A dependent steps)
        __syncthreads();   // (cf is free again)
        float t = 0.f;
        for (int j = threadIdx.x; j < A; j += blockDim.x) t += rowloss[j];
        cf[threadIdx.x] = t;
        __syncthreads();
        for (int st = blockDim.x >> 1; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) cf[threadIdx.x] += cf[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) loss_out[0] = cf[0] / (float)A;
    }
}

int64_t ocl_supcon_workspace_bytes(int n_anchor) {
    return ((int64_t)n_anchor * n_anchor + n_anchor + 64) * (int64_t)sizeof(float);
}

int ocl_supcon_fwd_bwd(const float* feat, const int64_t* y, int bsz, int n_views, int dim, float temperature, float* loss_out,
                       float* dfeat, void* workspace, void* stream) {
    OCL_REQUIRE(feat && y && loss_out && workspace, "supcon: null pointer");
    OCL_REQUIRE(bsz > 0 && n_views > 0 && dim > 0 && temperature > 0.f, "supcon: bad shape/temperature");
    const SPlan pl = plan_supcon(feat, bsz, n_views, dim, dfeat != nullptr);
    OCL_REQUIRE(pl.path != OCL_PATH_SUPCON_REFUSED, "supcon: A=%lld dim=%d too large", (long long)bsz * n_views, dim);
    const int A = bsz * n_views;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    float* G = (float*)workspace;
    float* rowloss = G + (int64_t)A * A;
    hipLaunchKernelGGL(supcon_rows, dim3(pl.grid_x), dim3(pl.block), (size_t)pl.lds_bytes, s, feat, y, bsz, A, dim, temperature, G, rowloss);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(supcon_grad, dim3(pl.grid2_x), dim3(pl.block2), (size_t)pl.lds2_bytes, s, feat, A, dim, temperature, G, rowloss,
                       loss_out, dfeat);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
