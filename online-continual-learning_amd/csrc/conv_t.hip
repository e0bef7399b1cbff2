// The conv_t_kernel instantiations without the EPI_BNB epilogue (forward, shortcut, data gradients) and their selector.
#include "conv_t_kernel.h"

namespace ocl {

conv_fn_t convt_plain_fn(int MT, int NT, int PF, int res, int cls, int pipe) {
    if (pipe) {   // staged weights through the ring: one pixel tile per wave
        if (res || NT != 1) return nullptr;
#define OCL_CASE(M)                                                                                                                  \
    if (MT == M) {                                                                                                                   \
        if (PF == 4) return cls ? conv_t_kernel<M, 1, 4, false, true, true> : conv_t_kernel<M, 1, 4, false, false, true>;            \
        if (PF == 8) return cls ? conv_t_kernel<M, 1, 8, false, true, true> : conv_t_kernel<M, 1, 8, false, false, true>;            \
    }
        OCL_CASE(1) OCL_CASE(2) OCL_CASE(3) OCL_CASE(4) OCL_CASE(5)
#undef OCL_CASE
        return nullptr;
    }
    if (cls) {   // output classes: one pixel tile per wave (the class lattices are the small ones)
#define OCL_CASE(M)                                                                                              \
    if (MT == M && NT == 1) {                                                                                    \
        if (PF == 4) return res ? conv_t_kernel<M, 1, 4, true, true> : conv_t_kernel<M, 1, 4, false, true>;      \
        if (PF == 8) return res ? conv_t_kernel<M, 1, 8, true, true> : conv_t_kernel<M, 1, 8, false, true>;      \
    }
        OCL_CASE(1) OCL_CASE(2) OCL_CASE(3) OCL_CASE(4) OCL_CASE(5)
#undef OCL_CASE
        return nullptr;
    }
#define OCL_CASE(M, N)                                                                              \
    if (MT == M && NT == N) {                                                                       \
        if (PF == 4) return res ? conv_t_kernel<M, N, 4, true> : conv_t_kernel<M, N, 4, false>;     \
        if (PF == 8) return res ? conv_t_kernel<M, N, 8, true> : conv_t_kernel<M, N, 8, false>;     \
    }
    OCL_CONVT_TILINGS(OCL_CASE)
#undef OCL_CASE
    return nullptr;
}

}  // namespace ocl
