// Internal interface of the small-op files (buffer_rows.hip, loader.hip, optim.hip, cosine.hip, row_losses.hip, supcon.hip, aser.hip,
// ncm.hip, augment.hip, gemm_small.hip): the launch plan -- which kernel variant, grid and LDS size an entry point takes for given sizes
// and pointer alignments -- and one plan function per launch.  Host-only.  Each plan function is defined in its family's file, above the
// kernels and the entry points that launch from it; ocl_test_small_op_path (small_ops.hip) reports the same functions' answers
// (tests/test_cpu_small_ops.py).
#pragma once
#include "common.h"

namespace ocl {

typedef ocl_small_op_plan SPlan;
static SPlan splan(int path, unsigned gx = 0, unsigned gy = 0, unsigned block = 0, int64_t lds = 0) {
    SPlan p = {};
    p.path = path;
    p.grid_x = gx; p.grid_y = gy; p.block = block; p.lds_bytes = lds;
    return p;
}
static int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16) == 0;
}

// buffer_rows.hip
SPlan plan_rows(const void* src, const void* dst, int64_t row_bytes, int64_t n);
SPlan plan_pair(const void* src_a, const void* dst_a, int64_t row_bytes_a, int64_t row_bytes_b, int64_t n);
// loader.hip
SPlan plan_u8(int64_t n, int h, int w, int c);
// optim.hip
SPlan plan_sgd(const void* params, const void* grads, const void* out, int64_t n);
// cosine.hip
SPlan plan_cosine(const void* mem, const void* g, int k, int64_t n);
// row_losses.hip
SPlan plan_ce(int path);
SPlan plan_mir(int n);
// supcon.hip
SPlan plan_supcon(const float* feat, int bsz, int n_views, int dim, bool want_grad);
// aser.hip
SPlan plan_knn(const float* cand_f, int n_eval, int n_cand, int dim);
SPlan plan_argsort(int n);
SPlan plan_cols(int path, int cols);
// ncm.hip
SPlan plan_ncm_means(int d, int n_cls);
SPlan plan_ncm_predict(int n, int d, int n_cls);
// augment.hip
SPlan plan_augment(int64_t n, int64_t h, int64_t w);
SPlan plan_aug_params(int64_t n);
// gemm_small.hip
SPlan plan_gemm(int m, int n, int k);

}  // namespace ocl
