// The EPI_BNB instantiations of conv_t_kernel (data gradients that feed a BatchNorm backward) and their selector.
#include "conv_t_kernel.h"

namespace ocl {

conv_fn_t convt_bnb_fn(int MT, int NT, int PF, int res, int cls, int pipe) {   // the EPI_BNB epilogue: stride-1 data gradients only (no output classes)
    if (cls) return nullptr;
    if (pipe) {
        if (res || NT != 1) return nullptr;
#define OCL_CASE(M)                                                                                     \
    if (MT == M) {                                                                                      \
        if (PF == 4) return conv_t_kernel<M, 1, 4, false, false, true, true>;                           \
        if (PF == 8) return conv_t_kernel<M, 1, 8, false, false, true, true>;                           \
    }
        OCL_CASE(1) OCL_CASE(2) OCL_CASE(3) OCL_CASE(4) OCL_CASE(5)
#undef OCL_CASE
        return nullptr;
    }
#define OCL_CASE(M, N)                                                                                                              \
    if (MT == M && NT == N) {                                                                                                       \
        if (PF == 4) return res ? conv_t_kernel<M, N, 4, true, false, false, true> : conv_t_kernel<M, N, 4, false, false, false, true>;   \
        if (PF == 8) return res ? conv_t_kernel<M, N, 8, true, false, false, true> : conv_t_kernel<M, N, 8, false, false, false, true>;   \
    }
    OCL_CONVT_TILINGS(OCL_CASE)
#undef OCL_CASE
    return nullptr;
}

}  // namespace ocl
