// Which path a small-op entry point takes (tests): ocl_test_small_op_path answers from the plan functions the entry points launch from
// (small_ops.h; each is defined beside its kernels and entry points, in its family's file).  Host-only, no launch.
#include "small_ops.h"

using namespace ocl;

static const void* P(int64_t v) { return (const void*)(uintptr_t)v; }

// One row per OCL_SOP_* code, in code order: the op, how many arguments it takes and its plan call (the argument lists: include/ocl_hip.h)
struct SopRow {
    int op, n_args;
    SPlan (*plan)(const int64_t* a);
};
static constexpr SopRow kSops[] = {
    {OCL_SOP_ROWS, 4, [](const int64_t* a) { return plan_rows(P(a[0]), P(a[1]), a[2], a[3]); }},
    {OCL_SOP_PAIR, 5, [](const int64_t* a) { return plan_pair(P(a[0]), P(a[1]), a[2], a[3], a[4]); }},
    {OCL_SOP_U8, 4, [](const int64_t* a) { return plan_u8(a[0], (int)a[1], (int)a[2], (int)a[3]); }},
    {OCL_SOP_SGD, 4, [](const int64_t* a) { return plan_sgd(P(a[0]), P(a[1]), P(a[2]), a[3]); }},
    {OCL_SOP_COSINE, 4, [](const int64_t* a) { return plan_cosine(P(a[0]), P(a[1]), (int)a[2], a[3]); }},
    {OCL_SOP_CE, 3, [](const int64_t* a) { return plan_ce(a[2] ? OCL_PATH_CE_MEAN : OCL_PATH_CE_NONE); }},
    {OCL_SOP_CE_SEG, 2, [](const int64_t*) { return plan_ce(OCL_PATH_CE_SEG); }},
    {OCL_SOP_KD, 2, [](const int64_t*) { return plan_ce(OCL_PATH_KD); }},
    {OCL_SOP_MIR, 2, [](const int64_t* a) { return plan_mir((int)a[0]); }},
    {OCL_SOP_SUPCON, 5, [](const int64_t* a) { return plan_supcon((const float*)P(a[0]), (int)a[1], (int)a[2], (int)a[3], a[4] != 0); }},
    {OCL_SOP_KNN, 5, [](const int64_t* a) { return plan_knn((const float*)P(a[0]), (int)a[1], (int)a[2], (int)a[3]); }},
    {OCL_SOP_COL_REDUCE, 2, [](const int64_t* a) { return plan_cols(OCL_PATH_COL_REDUCE, (int)a[1]); }},
    {OCL_SOP_ASER, 1, [](const int64_t* a) { return plan_cols(OCL_PATH_ASER_SCORE, (int)a[0]); }},
    {OCL_SOP_ARGSORT, 1, [](const int64_t* a) { return plan_argsort((int)a[0]); }},
    {OCL_SOP_NCM_MEANS, 2, [](const int64_t* a) { return plan_ncm_means((int)a[0], (int)a[1]); }},
    {OCL_SOP_NCM_PREDICT, 3, [](const int64_t* a) { return plan_ncm_predict((int)a[0], (int)a[1], (int)a[2]); }},
    {OCL_SOP_GEMM, 3, [](const int64_t* a) { return plan_gemm((int)a[0], (int)a[1], (int)a[2]); }},
    {OCL_SOP_AUGMENT, 3, [](const int64_t* a) { return plan_augment(a[0], a[1], a[2]); }},
    {OCL_SOP_AUG_PARAMS, 1, [](const int64_t* a) { return plan_aug_params(a[0]); }},
};
constexpr int kNumSops = (int)(sizeof(kSops) / sizeof(kSops[0]));
constexpr bool sops_in_code_order() {
    for (int i = 0; i < kNumSops; ++i)
        if (kSops[i].op != i) return false;
    return true;
}
static_assert(kNumSops == OCL_SOP_AUG_PARAMS + 1 && sops_in_code_order(), "kSops: one row per OCL_SOP_* code, indexed by the code");

int ocl_test_small_op_path(int op, const int64_t* a, int na, ocl_small_op_plan* plan) {
    if (op < 0 || op >= kNumSops || !a || na != kSops[op].n_args) {
        ocl::set_error("small_op_path: op %d takes %d arguments, got %d", op, op >= 0 && op < kNumSops ? kSops[op].n_args : -1, na);
        return 0;
    }
    const SPlan p = kSops[op].plan(a);
    if (plan) *plan = p;
    return p.path;
}
