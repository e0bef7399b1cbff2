// K10: ASER's retrieval and update scores: kNN-Shapley values (distances -> LDS bitonic sort -> fp64 suffix scan -> scatter), column
// reductions over the evaluation rows, the ASER score, and the descending argsort that picks the candidates.
#include "small_ops.h"
#include <math.h>
#include <vector>

using namespace ocl;

// =====================================================================================================
// K10 kNN Shapley (utils/buffer/aser_utils.py:7-61,94-116)
// =====================================================================================================
// A bitonic network sorts only under a total order: with a comparator that answers "no" both ways for two different entries (every float
// comparison against a NaN does) the network leaves an arbitrary arrangement, padding among the first n entries included.  Both orders
// below are total over everything the arrays can hold; they are host functions too, so that ocl_test_knn_order replays the kernel's very
// expressions on the CPU (tests/test_cpu_small_ops.py).
__host__ __device__ __forceinline__ bool key_less(float ka, int ia, float kb, int ib) {
    return (ka < kb) || (ka == kb && ia < ib);
}

// kNN (K10): numbers ascending, ties by index (+inf is a number); then the NaN keys in index order; then the padding, known by its index
// (idx >= n_real), never by its key -- a candidate at distance +inf ties with the padding's key and still sorts before it
__host__ __device__ __forceinline__ bool key_less_nan_last(float ka, int ia, float kb, int ib, int n_real) {
    // without a branch (every lane of the sort evaluates all of it).  Two numbers: the first line; a comparison against a NaN is false, so with
    // a NaN the first line is false and the second decides: a < b if b is a NaN and a is a number or a NaN of lower index.  A real entry
    // before the padding, and two padding entries are equal
    const bool pa = ia >= n_real, pb = ib >= n_real, na = ka != ka, nb = kb != kb, il = ia < ib;
    const bool num = (ka < kb) | ((ka == kb) & il);
    const bool real = num | (nb & (!na | il));
    return !pa & (pb | real);
}

// argsort: NaN keys before every number (index order among themselves), torch's descending NaN-first rule; the padding (+inf with the
// largest index) is never a NaN and loses every tie, so it stays last
__host__ __device__ __forceinline__ bool key_less_nan_first(float ka, int ia, float kb, int ib) {
    const bool na = ka != ka, nb = kb != kb;
    if (na || nb) return na && (!nb || ia < ib);
    return key_less(ka, ia, kb, ib);
}

__host__ __device__ __forceinline__ void bitonic_pad(float* key, int* idx, int c) {
    key[c] = INFINITY;
    idx[c] = 0x7fffffff;
}

// compare-exchange number t (of P / 2) of the network's stage (k, j); the pairs of one stage are disjoint
template <bool NAN_FIRST>
__host__ __device__ __forceinline__ void bitonic_exchange(float* key, int* idx, int t, int j, int k, int n_real) {
    const int lo = 2 * t - (t & (j - 1));      // j is a power of two: (t / j) * 2 j + t % j
    const int hi = lo + j;
    const bool up = ((lo & k) == 0);
    const float ka = key[lo], kb = key[hi];
    const int ia = idx[lo], ib = idx[hi];
    const bool lt = NAN_FIRST ? key_less_nan_first(kb, ib, ka, ia) : key_less_nan_last(kb, ib, ka, ia, n_real);  // hi < lo
    if (lt == up) {
        key[lo] = kb; key[hi] = ka;
        idx[lo] = ib; idx[hi] = ia;
    }
}

// in-LDS bitonic sort of P (pow2) (key, idx) pairs, the first n_real real and the others padding, ascending in the order chosen
template <bool NAN_FIRST>
__device__ __forceinline__ void bitonic_sort_lds(float* key, int* idx, int P, int n_real) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) bitonic_exchange<NAN_FIRST>(key, idx, t, j, k, n_real);
        }
    }
    __syncthreads();
}

// the in-kernel predicate of knn_sv_kernel's one-thread-per-candidate distance loop
__host__ __device__ __forceinline__ bool knn_vec(const float* cand_f, int dim) { return (dim & 3) == 0 && (((uintptr_t)cand_f) & 15) == 0; }
namespace ocl {
SPlan plan_knn(const float* cand_f, int n_eval, int n_cand, int dim) {
    if (n_cand > OCL_KNN_MAX_CAND) return splan(OCL_PATH_KNN_REFUSED);
    const int P = next_pow2(n_cand), d4n = dim >> 2;
    const int path = !knn_vec(cand_f, dim) ? OCL_PATH_KNN_WAVE : d4n < 4 ? OCL_PATH_KNN_VEC_REM : (d4n % 4) ? OCL_PATH_KNN_VEC_BOTH : OCL_PATH_KNN_VEC_UNROLL;
    SPlan p = splan(path, (unsigned)n_eval, 1, 256, (int64_t)P * (8 + 4 + 4) + (int64_t)dim * 4);
    p.aux = P;
    return p;
}
SPlan plan_argsort(int n) {
    if (n > OCL_SORT_MAX) return splan(OCL_PATH_ARGSORT_REFUSED);
    const int P = next_pow2(n);
    SPlan p = splan(P == n ? OCL_PATH_ARGSORT_FULL : OCL_PATH_ARGSORT_PADDED, 1, 1, 256, (int64_t)P * 8);
    p.aux = P;
    return p;
}
SPlan plan_cols(int path, int cols) { return splan(path, (unsigned)cdiv(cols, 32), 1, 256); }
}  // namespace ocl

__global__ void __launch_bounds__(256) knn_sv_kernel(const float* __restrict__ eval_f, const int64_t* __restrict__ eval_y,
                                                     const float* __restrict__ cand_f, const int64_t* __restrict__ cand_y,
                                                     int n_cand, int dim, int k, int P, float* __restrict__ sv_out,
                                                     int64_t* __restrict__ sorted_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    double* scan = (double*)smraw;              // P doubles (first: 8-B aligned)
    float* key = (float*)(scan + P);            // P
    int* idx = (int*)(key + P);                 // P
    float* ef = (float*)(idx + P);              // dim
    const int e = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = threadIdx.x; d < dim; d += blockDim.x) ef[d] = eval_f[(int64_t)e * dim + d];
    for (int c = n_cand + threadIdx.x; c < P; c += blockDim.x) bitonic_pad(key, idx, c);
    __syncthreads();
    // squared Euclidean distance sum((u-v)^2) (utils/utils.py:93-95): one THREAD per candidate, its feature row streamed with four
    // independent 16-byte loads in flight (rows are L2-resident: every workgroup reads the same candidates), the evaluation row
    // broadcast from LDS.  (One wave per candidate with a shuffle reduction made every step a dependent ~0.5 us L2 round trip.)
    if (knn_vec(cand_f, dim)) {
        const int d4n = dim >> 2;
        for (int c = threadIdx.x; c < n_cand; c += blockDim.x) {
            const float4* cf = (const float4*)(cand_f + (int64_t)c * dim);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            int d4 = 0;
            for (; d4 + 4 <= d4n; d4 += 4) {
                const float4 v0 = cf[d4], v1 = cf[d4 + 1], v2 = cf[d4 + 2], v3 = cf[d4 + 3];
                const float4 e0 = *(const float4*)(ef + 4 * d4), e1 = *(const float4*)(ef + 4 * d4 + 4);
                const float4 e2 = *(const float4*)(ef + 4 * d4 + 8), e3 = *(const float4*)(ef + 4 * d4 + 12);
                float t;
                t = e0.x - v0.x; s0 = fmaf(t, t, s0); t = e0.y - v0.y; s1 = fmaf(t, t, s1); t = e0.z - v0.z; s2 = fmaf(t, t, s2); t = e0.w - v0.w; s3 = fmaf(t, t, s3);
                t = e1.x - v1.x; s0 = fmaf(t, t, s0); t = e1.y - v1.y; s1 = fmaf(t, t, s1); t = e1.z - v1.z; s2 = fmaf(t, t, s2); t = e1.w - v1.w; s3 = fmaf(t, t, s3);
                t = e2.x - v2.x; s0 = fmaf(t, t, s0); t = e2.y - v2.y; s1 = fmaf(t, t, s1); t = e2.z - v2.z; s2 = fmaf(t, t, s2); t = e2.w - v2.w; s3 = fmaf(t, t, s3);
                t = e3.x - v3.x; s0 = fmaf(t, t, s0); t = e3.y - v3.y; s1 = fmaf(t, t, s1); t = e3.z - v3.z; s2 = fmaf(t, t, s2); t = e3.w - v3.w; s3 = fmaf(t, t, s3);
            }
            for (; d4 < d4n; ++d4) {
                const float4 v0 = cf[d4];
                const float4 e0 = *(const float4*)(ef + 4 * d4);
                float t;
                t = e0.x - v0.x; s0 = fmaf(t, t, s0); t = e0.y - v0.y; s1 = fmaf(t, t, s1); t = e0.z - v0.z; s2 = fmaf(t, t, s2); t = e0.w - v0.w; s3 = fmaf(t, t, s3);
            }
            key[c] = (s0 + s1) + (s2 + s3);
            idx[c] = c;
        }
    } else {
        for (int c = wid; c < n_cand; c += nw) {
            const float* cf = cand_f + (int64_t)c * dim;
            float s = 0.f;
            for (int d = lane; d < dim; d += 64) {
                const float t = ef[d] - cf[d];
                s = fmaf(t, t, s);
            }
            s = wave_sum(s);
            if (lane == 0) {
                key[c] = s;
                idx[c] = c;
            }
        }
    }
    bitonic_sort_lds<false>(key, idx, P, n_cand);   // a total order: idx[0 .. n_cand) is a permutation of the candidates for every input
    // indicator difference x factor (aser_utils.py:33-50), then reverse cumulative sum (:51-52)
    const int64_t ye = eval_y[e];
    const int N = n_cand;
    for (int j = threadIdx.x; j < P; j += blockDim.x) {
        double v = 0.0;
        if (j < N) {
            const float ind = (cand_y[idx[j]] == ye) ? 1.f : 0.f;
            const float nxt = (j + 1 < N) ? ((cand_y[idx[j + 1]] == ye) ? 1.f : 0.f) : 0.f;
            float numer = (float)(j + 1), denom = (float)(j + 1);
            if (j < N - 1) denom = denom * (float)k;
            if (j >= k && j < N - 1) numer = (float)k;
            if (j == N - 1) numer = 1.f;
            const float factor = numer / denom;
            v = (double)((ind - nxt) * factor);
        }
        scan[j] = v;
    }
    __syncthreads();
    // inclusive suffix scan in double (torch's CPU cumsum accumulates float in double)
    for (int off = 1; off < P; off <<= 1) {
        double add[8];  // P <= 2048, 256 threads: statically indexed so it stays in registers
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = threadIdx.x + q * 256;
            add[q] = (j < P && j + off < P) ? scan[j + off] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = threadIdx.x + q * 256;
            if (j < P) scan[j] += add[q];
        }
        __syncthreads();
    }
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        sv_out[(int64_t)e * N + idx[j]] = (float)scan[j];
        if (sorted_idx) sorted_idx[(int64_t)e * N + j] = (int64_t)idx[j];
    }
}

// column reductions over evaluation rows: 32 columns x 8 row lanes per workgroup; the fp64 lane sums are combined in a
// fixed order (deterministic)
__global__ void __launch_bounds__(256) col_reduce_kernel(const float* __restrict__ m, int rows, int cols, int mode,
                                                         float* __restrict__ out) {
    __shared__ double red[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    double s = 0.0;
    float v = mode == 2 ? -INFINITY : INFINITY;
    if (c < cols)
        for (int r = rl; r < rows; r += 8) {
            const float t = m[(int64_t)r * cols + c];
            s += (double)t;
            v = mode == 2 ? fmaxf(v, t) : fminf(v, t);
        }
    red[rl][cl] = mode <= 1 ? s : (double)v;
    __syncthreads();
    if (rl == 0 && c < cols) {
        if (mode <= 1) {
            const double t = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
            out[c] = mode == 1 ? (float)(t / (double)rows) : (float)t;
        } else {
            double t = red[0][cl];
            for (int k = 1; k < 8; ++k) t = mode == 2 ? fmax(t, red[k][cl]) : fmin(t, red[k][cl]);
            out[c] = (float)t;
        }
    }
}

__global__ void __launch_bounds__(256) aser_score_kernel(const float* __restrict__ adv, int n_adv, const float* __restrict__ coop,
                                                         int n_coop, int n_cand, int type, float* __restrict__ out) {
    __shared__ double ra[8][33], rc[8][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    double sa = 0.0, sc = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    if (c < n_cand) {
        for (int r = rl; r < n_adv; r += 8) {
            const float t = adv[(int64_t)r * n_cand + c];
            sa += (double)t;
            mn = fminf(mn, t);
        }
        if (type != 2)
            for (int r = rl; r < n_coop; r += 8) {
                const float t = coop[(int64_t)r * n_cand + c];
                sc += (double)t;
                mx = fmaxf(mx, t);
            }
    }
    ra[rl][cl] = type == 1 ? (double)mn : sa;
    rc[rl][cl] = type == 1 ? (double)mx : sc;
    __syncthreads();
    if (rl == 0 && c < n_cand) {
        if (type == 1) {
            double a = ra[0][cl], b = rc[0][cl];
            for (int k = 1; k < 8; ++k) { a = fmin(a, ra[k][cl]); b = fmax(b, rc[k][cl]); }
            out[c] = (float)b - (float)a;
        } else {
            const double ta = ((ra[0][cl] + ra[1][cl]) + (ra[2][cl] + ra[3][cl])) + ((ra[4][cl] + ra[5][cl]) + (ra[6][cl] + ra[7][cl]));
            const double tc = ((rc[0][cl] + rc[1][cl]) + (rc[2][cl] + rc[3][cl])) + ((rc[4][cl] + rc[5][cl]) + (rc[6][cl] + rc[7][cl]));
            if (type == 0) out[c] = (float)(tc / (double)n_coop) - (float)(ta / (double)n_adv);
            else out[c] = (float)ta * -1.0f;
        }
    }
}

// descending argsort, single workgroup; ties keep ascending index
__global__ void __launch_bounds__(256) argsort_desc_kernel(const float* __restrict__ v, int n, int P, int64_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw2[];
    float* key = (float*)smraw2;
    int* idx = (int*)(key + P);
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
        if (i < n) {
            key[i] = -v[i];  // NaN stays NaN: first in torch's descending order, before +inf (key_less_nan_first)
            idx[i] = i;
        } else {
            bitonic_pad(key, idx, i);
        }
    }
    bitonic_sort_lds<true>(key, idx, P, n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) out[i] = (int64_t)idx[i];
}

int ocl_knn_sv(const float* eval_f, const int64_t* eval_y, int n_eval, const float* cand_f, const int64_t* cand_y, int n_cand,
               int dim, int k, float* sv_out, int64_t* sorted_idx, void* stream) {
    OCL_REQUIRE(n_eval >= 0 && n_cand >= 0 && dim > 0 && k > 0, "knn_sv: bad sizes n_eval=%d n_cand=%d dim=%d k=%d", n_eval,
                n_cand, dim, k);
    if (n_eval == 0 || n_cand == 0) return OCL_OK;
    OCL_REQUIRE(eval_f && eval_y && cand_f && cand_y && sv_out, "knn_sv: null pointer");
    const SPlan pl = plan_knn(cand_f, n_eval, n_cand, dim);
    OCL_REQUIRE(pl.path != OCL_PATH_KNN_REFUSED, "knn_sv: n_cand=%d exceeds OCL_KNN_MAX_CAND=%d", n_cand, OCL_KNN_MAX_CAND);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    hipLaunchKernelGGL(knn_sv_kernel, dim3(pl.grid_x), dim3(pl.block), (size_t)pl.lds_bytes, s, eval_f, eval_y, cand_f, cand_y, n_cand, dim, k, pl.aux, sv_out,
                       sorted_idx);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_col_reduce(const float* m, int rows, int cols, int mode, float* out, void* stream) {
    OCL_REQUIRE(m && out && rows > 0 && cols > 0 && mode >= 0 && mode <= 3, "col_reduce: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_cols(OCL_PATH_COL_REDUCE, cols);
    hipLaunchKernelGGL(col_reduce_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, m, rows, cols, mode, out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_aser_score(const float* sv_adv, int n_adv, const float* sv_coop, int n_coop, int n_cand, int type, float* out,
                   void* stream) {
    OCL_REQUIRE(sv_adv && out && n_adv > 0 && n_cand > 0 && type >= 0 && type <= 2, "aser_score: bad arguments");
    OCL_REQUIRE(type == 2 || (sv_coop && n_coop > 0), "aser_score: cooperative matrix required for type %d", type);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    const SPlan pl = plan_cols(OCL_PATH_ASER_SCORE, n_cand);
    hipLaunchKernelGGL(aser_score_kernel, dim3(pl.grid_x), dim3(pl.block), 0, s, sv_adv, n_adv, sv_coop, n_coop, n_cand, type,
                       out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_argsort_desc(const float* v, int n, int64_t* idx_out, void* stream) {
    OCL_REQUIRE(n >= 0, "argsort: n<0");
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(v && idx_out, "argsort: null pointer");
    const SPlan pl = plan_argsort(n);
    OCL_REQUIRE(pl.path != OCL_PATH_ARGSORT_REFUSED, "argsort: n=%d exceeds OCL_SORT_MAX=%d", n, OCL_SORT_MAX);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_KNN, s);
    hipLaunchKernelGGL(argsort_desc_kernel, dim3(pl.grid_x), dim3(pl.block), (size_t)pl.lds_bytes, s, v, n, pl.aux, idx_out);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_test_knn_order(const float* keys, int n_cand, int64_t* order_out) {
    OCL_REQUIRE(keys && order_out && n_cand >= 1 && n_cand <= OCL_KNN_MAX_CAND, "knn_order: bad arguments");
    const int P = next_pow2(n_cand);
    std::vector<float> key(P);
    std::vector<int> idx(P);
    for (int c = 0; c < n_cand; ++c) {
        key[c] = keys[c];
        idx[c] = c;
    }
    for (int c = n_cand; c < P; ++c) bitonic_pad(key.data(), idx.data(), c);
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int t = 0; t < (P >> 1); ++t) bitonic_exchange<false>(key.data(), idx.data(), t, j, k, n_cand);
    for (int c = 0; c < n_cand; ++c) order_out[c] = (int64_t)idx[c];
    return OCL_OK;
}
