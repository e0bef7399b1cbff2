// K6e: Dark Experience Replay's loss (DER / DER++, Buzzega et al., NeurIPS 2020) -- the cross-entropy of the stream batch, alpha times the
// mean squared error between today's logits of replayed images and the logits those images had when they entered the memory, and beta
// times the cross-entropy of a second replayed batch -- and its gradient with respect to the logits, in ONE launch.  The logits are one
// contiguous block of n0 + n1 + n2 rows, as a taped pass over the three batches returns it:
//   ce    = mean_{r < n0}( lse(s_r) - s_r[y0_r] )
//   mse   = sum_{r in block 1, j} (s_rj - z_rj)^2 / (n1 * c)            z_r = stored[slots[r]]  (slots null: stored[r])
//   ce_m  = mean_{r in block 2}( lse(s_r) - s_r[y2_r] )
//   loss_out = { ce + alpha * mse + beta * ce_m, ce, mse, ce_m }
//   dlogits:  block 0 (softmax - onehot) / n0;   block 1 alpha * 2 * (s - z) / (n1 * c);   block 2 beta * (softmax - onehot) / n2
// A member of the row family (row_dev.h): a single workgroup of ROW_WAVES waves, wave w takes rows w, w + 4, ... of the whole block, lane
// l owns columns l, l + 64, ...; a row of up to ROW_REG * 64 columns is read once and kept in registers.  The cross-entropy rows are
// ce_row as it is: block 0's rows fall to the waves ce_kernel gives them to and are summed in its order, so with n1 = n2 = 0 the loss and
// the gradient are ocl_ce_fwd_bwd's bits.  The squared error's element, row and cross-row sums are in double (the square of a float
// difference is exact there), as icarl.hip carries its sums, and so are block 2's row losses (ce_row's `exact`) and their sum; the total
// is formed in double from the three terms and rounded once.  The difference s - z is formed once and feeds both the loss and the
// gradient: a stored row that equals today's row bit for bit gives exactly 0 for both.  Sums in a fixed order, no atomics: two runs give
// the same bits.
//
// Addresses: a label outside [0, c) is no address (ce_row: that row's loss is NaN, no one-hot is subtracted); a slot outside [0, m) is no
// address (that row's z is NaN in every column and nothing is read); block 1 never reads a label; an empty block reads nothing.
// Nothing in this file may be built with fast-math.
#include <cmath>

#include "row_dev.h"

using namespace ocl;

// REPLAY: a block 1 or a block 2 is present (false: the stream rows alone, ce_kernel's statements)
template <bool REG, bool REPLAY>
__global__ void __launch_bounds__(256) der_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ y0,
                                                       const int64_t* __restrict__ y2, const float* __restrict__ stored,
                                                       const int64_t* __restrict__ slots, int n0, int n1, int n2, int c, int m, float alpha,
                                                       float beta, float* __restrict__ loss_out, float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const int n = REPLAY ? n0 + n1 + n2 : n0;
    const float scale0 = 1.0f / (float)n0;                                   // ce_kernel's scale
    const float scale2 = REPLAY && n2 > 0 ? beta * (1.0f / (float)n2) : 0.f;
    const float scale1 = REPLAY && n1 > 0 ? alpha * 2.0f / ((float)n1 * (float)c) : 0.f;
    float ce[1] = {0.f};          // the wave's rows of block 0: ce_kernel's sum
    double mem[2] = {0.0, 0.0};   // [0] the lane's columns of the wave's rows of block 1; [1] the wave's rows of block 2
    ROW_FOR_EACH(r, n) {
        const float* s = logits + (int64_t)r * c;
        float* dx = dlogits ? dlogits + (int64_t)r * c : nullptr;
        if (REPLAY && r >= n0 && r < n0 + n1) {
            const int64_t slot = slots ? slots[r - n0] : (int64_t)(r - n0);
            const bool held = (uint64_t)slot < (uint64_t)m;
            RowCols<REG>(s, held ? stored + slot * c : nullptr, lane, c, held ? c : 0, NAN).each([&](int j, float sj, float zj) {
                const float d = sj - zj;
                mem[0] += (double)d * (double)d;
                if (dx) dx[j] = d * scale1;
            });
        } else {
            // a replayed row's loss is ce_row's `exact` one (log of the sum, the max and the label's logit combined in double): a block of
            // one row whose loss is small beside its logits is not averaged with larger ones, and lse - x[y] in float would leave it with the
            // rounding of the lse.  Block 0 keeps the float one: it is ce_kernel's.
            const bool rep = REPLAY && r >= n0;
            double exact = 0.0;
            // (&exact on every row: a pointer chosen by `rep` puts the double in scratch; an unread one costs nothing)
            const float l = ce_row(RowCols<REG>(s, nullptr, lane, c, 0, 0.f), c, rep ? y2[r - n0 - n1] : y0[r], dx, rep ? scale2 : scale0, &exact);
            ce[0] += rep ? 0.f : l;   // (two selects, as in icarl.hip: an indexed sum would sit in scratch)
            mem[1] += rep ? exact : 0.0;
        }
    }
    if (REPLAY) mem[0] = wave_sum_d(mem[0]);
    row_fold(ce);
    if (REPLAY) row_fold(mem);
    if (threadIdx.x == 0) {
        const float ce0 = ce[0] / (float)n0;                                 // ce_kernel's mean
        const double ce2 = REPLAY && n2 > 0 ? mem[1] / (double)n2 : 0.0;
        const double mse = REPLAY && n1 > 0 ? mem[0] / ((double)n1 * (double)c) : 0.0;
        loss_out[0] = REPLAY ? (float)((double)ce0 + (double)alpha * mse + (double)beta * ce2) : ce0;
        loss_out[1] = ce0;
        loss_out[2] = (float)mse;
        loss_out[3] = (float)ce2;
    }
}

int ocl_der_fwd_bwd(const float* logits, const int64_t* y0, const int64_t* y2, const float* stored, const int64_t* slots, int n0, int n1,
                    int n2, int c, int m, float alpha, float beta, float* loss_out, float* dlogits, void* stream) {
    OCL_REQUIRE(logits && y0 && loss_out, "der_loss: null pointer (logits, y0 and loss_out are required)");
    OCL_REQUIRE(n0 >= 1 && n1 >= 0 && n2 >= 0 && c >= 1, "der_loss: n0=%d n1=%d n2=%d c=%d (n0 >= 1, n1 >= 0, n2 >= 0, c >= 1)", n0, n1, n2, c);
    OCL_REQUIRE((int64_t)n0 + n1 + n2 <= INT32_MAX, "der_loss: n0 + n1 + n2 = %lld rows (at most 2^31 - 1)", (long long)n0 + n1 + n2);
    OCL_REQUIRE(n1 == 0 || (stored && m >= 1), "der_loss: n1=%d with stored %s and m=%d (a logit-replay block needs the table and m >= 1)", n1,
                stored ? "given" : "null", m);
    OCL_REQUIRE(n2 == 0 || y2, "der_loss: n2=%d without y2", n2);
    OCL_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "der_loss: alpha=%g beta=%g (must be finite)", (double)alpha, (double)beta);
    const size_t bytes = (size_t)((int64_t)n0 + n1 + n2) * (size_t)c * sizeof(float);
    const size_t table = n1 > 0 ? (size_t)m * (size_t)c * sizeof(float) : 0;
    if (int rc = row_check_output("der_loss", {dlogits, bytes, "dlogits"}, {{logits, bytes, "logits"}, {n1 > 0 ? stored : nullptr, table, "stored"}}))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_HEAD, s);
    const bool reg = row_in_regs(c), replay = n1 > 0 || n2 > 0;
    auto k = replay ? (reg ? der_loss_kernel<true, true> : der_loss_kernel<false, true>)
                    : (reg ? der_loss_kernel<true, false> : der_loss_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, s, logits, y0, y2, stored, slots, n0, n1, n2, c, m, alpha, beta, loss_out, dlogits);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
