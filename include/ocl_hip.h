/*
 * ocl_hip.h — C-ABI of libocl_hip.so: the MI355X (gfx950) replay-step hot path of
 * RaptorMai/online-continual-learning, hand-written HIP.
 *
 * The reference is pure Python on PyTorch and defines no FFI; every entry point
 * here replaces an ATen op *sequence* inside the reference and cites the file:line it stands in
 * for.  The reference-side binding (a ctypes stub) is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain C: raw device pointers + sizes, no torch types.  `stream` is a hipStream_t passed as
 *     void* (NULL = the null stream).  Calls are stream-ordered and never synchronise the host.
 *   - caller owns all memory (PyTorch tensors on the Python side); the library allocates nothing on
 *     the device.  Scratch comes from caller-provided workspaces whose sizes are queried first.
 *   - return 0 on success, <0 on error; ocl_last_error() returns a thread-local message.  The Python
 *     wrapper turns non-zero into RuntimeError (the reference's error convention is exceptions:
 *     utils/loss.py:36-50, utils/buffer/reservoir_update.py:46-51).
 *   - labels / indices are int64 (PyTorch LongTensor) everywhere; floats are fp32 (exact-fp32 MFMA,
 *     no reduced precision anywhere).
 */
#ifndef OCL_HIP_H
#define OCL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCL_OK 0
#define OCL_ERR_ARG (-1)
#define OCL_ERR_HIP (-2)
#define OCL_ERR_STATE (-3)
#define OCL_ERR_UNSUPPORTED (-4)

/* ---- library ---------------------------------------------------------------------------------- */
int ocl_version(void);
const char* ocl_last_error(void);
/* Selects the device and verifies it is gfx950; fails loudly otherwise. */
int ocl_init(int device);

/* ---- K9: replay-buffer row gather / scatter ----------------------------------------------------
 * replaces buffer.buffer_img[indices] / buffer_label[indices] (utils/buffer/buffer_utils.py:19-21,
 * 115-116) and the slot overwrite buffer_img[idx] = x (utils/buffer/reservoir_update.py:59-60,
 * utils/buffer/aser_update.py:111-112).  row_bytes must be a multiple of 4.  Duplicate indices in a
 * scatter are the caller's problem (the reference de-duplicates with a dict first). */
int ocl_gather_rows(const void* src, const int64_t* idx, int64_t n, int64_t row_bytes, void* dst,
                    void* stream);
int ocl_scatter_rows(void* dst, const int64_t* idx, int64_t n, int64_t row_bytes, const void* src,
                     void* stream);
/* The pair buffer.buffer_img[indices], buffer.buffer_label[indices] of every retrieval (utils/buffer/buffer_utils.py:19-21,115-116;
 * utils/buffer/aser_utils.py:152-155) as ONE call and one launch: rows of two arrays by the same index vector.  idx_host != NULL:
 * the indices were drawn on the host (numpy / torch-CPU generators); they are uploaded into idx_dev (n int64, caller-owned) first,
 * asynchronously.  idx_host == NULL: idx_dev already holds them (e.g. the ranking of ocl_argsort_desc). */
int ocl_gather_rows_pair(const void* src_a, int64_t row_bytes_a, void* dst_a, const void* src_b, int64_t row_bytes_b, void* dst_b,
                         const int64_t* idx_host, int64_t* idx_dev, int64_t n, void* stream);
/* Host -> device upload of a small host array (index vectors the reference builds with torch.tensor(...) / torch.from_numpy(...)
 * and moves with maybe_cuda: utils/buffer/buffer_utils.py:17-21, reservoir_update.py:52-60).  Asynchronous on `stream`; `host`
 * may be reused as soon as the call returns (payloads <= 64 KB are staged through pinned memory). */
int ocl_upload(const void* host, int64_t nbytes, void* dev, void* stream);
/* dataset_transform + ToTensor for a whole minibatch (continuum/data_utils.py:38-54,
 * utils/setup_elements.py:29-43): gathers n HWC uint8 images by index from a device-resident task
 * tensor and writes CHW fp32 / 255. */
int ocl_gather_u8_hwc_to_f32_chw(const uint8_t* src, const int64_t* idx, int64_t n, int h, int w,
                                 int c, float* dst, void* stream);
/* The same for a task whose images are already float (the new-instance streams of continuum/non_stationary.py hand
 * over HWC arrays divided by 255): dataset_transform.__getitem__ on a non-uint8 array is ToTensor's transpose HWC ->
 * CHW and .float(), nothing else.  The float32 rounding is done once per task on the host; this gathers n HWC float32
 * images by index from the device-resident task and writes them CHW, bit for bit (NaN payloads, -0.0 and denormals
 * included).  16-byte loads when h*w*c is a multiple of 4, src is 16-byte aligned and c <= 16; 4-byte loads otherwise.
 * src and dst must be 4-byte aligned. */
int ocl_gather_f32_hwc_to_f32_chw(const float* src, const int64_t* idx, int64_t n, int h, int w, int c,
                                  float* dst, void* stream);

/* ---- K8: SGD -------------------------------------------------------------------------------------
 * torch.optim.SGD.step with momentum 0 (utils/setup_elements.py:73-75): p <- p - lr*(g + wd*p).
 * With out != NULL the result goes to `out` and p is untouched: that is MIR's virtual step on a
 * deepcopy (utils/buffer/mir_retrieve.py:34-47) without the copy. grad_scale multiplies g first
 * (review trick divides grads by 10, agents/base.py:84-87). */
int ocl_sgd_step(float* params, const float* grads, int64_t n, float lr, float weight_decay,
                 float grad_scale, float* out, void* stream);

/* ---- K8b: Adam -----------------------------------------------------------------------------------
 * torch.optim.Adam.step (utils/setup_elements.py:76-79: betas (0.9, 0.999), eps 1e-8, amsgrad off) over the
 * flat parameter, gradient and moment arrays, one launch, in the order of torch's _single_tensor_adam:
 *   g' = wd*p + g*grad_scale;  m <- m + (1-beta1)*(g'-m);  v <- beta2*v + (1-beta2)*g'*g';
 *   p <- p - step_size * (m / (sqrt(v)/bc2_sqrt + eps)),  step_size = lr/(1-beta1^step), bc2_sqrt = sqrt(1-beta2^step).
 * `step` is this step's 1-based number; step_size, bc2_sqrt and 1-beta are formed in double on the host from
 * the float arguments (no device-side counter, no synchronisation).  Elements [skip_begin, skip_end) keep p, m
 * and v: parameters that never get a gradient, which torch skips entirely (SupConResNet's encoder.linear.*).
 * All four arrays 16-byte aligned; OCL_ERR_ARG before any launch for a null or misaligned pointer, n <= 0,
 * step < 1, a beta outside [0, 1), eps < 0, or a skip range that is not 0 <= begin <= end <= n. */
int ocl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float grad_scale, int64_t step,
                  int64_t skip_begin, int64_t skip_end, void* stream);

/* ---- K8c: A-GEM gradient projection ----------------------------------------------------------------
 * agents/agem.py:72-80 on the flat gradient array, between backward and the optimiser step:
 *   prod = sum g*g_ref;  prod_ref = sum g_ref*g_ref;
 *   out = prod < 0 ? g - (prod / prod_ref) * g_ref : g        (out is written over g_ref_inout)
 * Two launches on `stream`, no host synchronisation, no atomics.  Products and sums are formed in double in a
 * fixed order (block count a function of n alone): two runs give the same bits.  prod < 0 is false for NaN and
 * for g_ref == 0; a not-projected output is a bit copy of g.  coef = (float)(prod / prod_ref).  info4 (may be
 * NULL) receives {(float)prod, (float)prod_ref, projected ? coef : 0, projected ? 1 : 0}.
 * `workspace`: at least ocl_agem_workspace_doubles(n) doubles of device memory, 8-byte aligned (the per-block
 * partial pairs; at most 1024).  g and g_ref_inout 16-byte aligned and disjoint; OCL_ERR_ARG before any launch
 * for a null or misaligned pointer, n <= 0, overlapping arrays or a workspace that is too small. */
int64_t ocl_agem_workspace_doubles(int64_t n);
int ocl_agem_project(const float* g, float* g_ref_inout, int64_t n, double* workspace,
                     int64_t workspace_doubles, float* info4, void* stream);

/* ---- K8d: EWC++ bookkeeping -------------------------------------------------------------------------
 * agents/ewc_pp.py on flat arrays of n floats, all 16-byte aligned and pairwise disjoint; no host
 * synchronisation, no atomics; OCL_ERR_ARG ("ewc: ...") before any launch for a null or misaligned pointer,
 * n <= 0, overlapping arrays or a workspace that is too small.
 *
 * ocl_ewc_accumulate (:83-92, :104-106), once per step between backward and the optimiser step, one launch:
 *   d = p - p_prev;  g' = g + scale * f_hat * d;  tmp += g' * g'       (g' over g, the sum over tmp)
 * scale = 2 * lambda * w, w the weight the KD tricks put on the loss (1 without them).  prev_params and
 * fisher_hat both NULL (first task): tmp += g * g alone, g is not written.  scale == 0 does not write g either.
 * One of the two NULL is an argument error.  With penalty_out != NULL every block also writes a double partial
 * of sum f_hat * d * d (d formed in double) to `workspace` (at least ocl_ewc_workspace_doubles(n) doubles, at
 * most 512, 8-byte aligned) and a second one-block launch adds them in index order: penalty_out[0] = (float)sum
 * (0 without prev_params).  With penalty_out == NULL the workspace is neither needed nor touched.
 *
 * ocl_ewc_fisher_ema (:97-102), one launch: running = keep * running + gain * tmp with both products and the
 * sum rounded separately (no fma: the bits of the float32 statement), then tmp = 0.
 *
 * ocl_ewc_fisher_normalize (:76-80), two launches: fisher_hat = (running - min) / (max - min + 1e-32f) in IEEE
 * float32, min and max over the whole array; a NaN anywhere makes min, max and every output NaN.  `workspace`:
 * 2 * ocl_ewc_workspace_doubles(n) floats (the same workspace serves both calls).  minmax_out2 (may be NULL)
 * receives {min, max}. */
int64_t ocl_ewc_workspace_doubles(int64_t n);
int ocl_ewc_accumulate(float* grads_inout, float* tmp_fisher_inout, const float* params, const float* prev_params,
                       const float* fisher_hat, int64_t n, float scale, double* workspace, int64_t workspace_doubles,
                       float* penalty_out, void* stream);
int ocl_ewc_fisher_ema(float* running_inout, float* tmp_inout, int64_t n, float keep, float gain, void* stream);
int ocl_ewc_fisher_normalize(const float* running, float* fisher_hat_out, int64_t n, float* workspace,
                             int64_t workspace_floats, float* minmax_out2, void* stream);

/* ---- K8e: global L2-norm gradient clip ---------------------------------------------------------------
 * torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite off; agents/gdumb.py:82) on the flat gradient
 * array, between backward and the optimiser step:
 *   total = sqrt(sum g*g);  coef = max_norm / (total + 1e-6);  g *= min(coef, 1)
 * Two launches on `stream`, no host synchronisation, no atomics.  Squares and sums are formed in double in a
 * fixed order (block count a function of n alone): two runs give the same bits.  sqrt and the IEEE divide are
 * done in double, coef = (float)(that quotient).  Where the quotient is >= 1 (or rounds to 1.0f) no element is
 * read or written; otherwise every element becomes g * coef, one rounded float multiply.  A NaN norm multiplies
 * through (every element NaN); an infinite norm gives coef = 0 (finite elements 0, infinite ones NaN).  info4
 * (may be NULL) receives {(float)total, clipped ? coef : 1, clipped ? 1 : 0, (float)sum g*g}.
 * `workspace`: at least ocl_clip_workspace_doubles(n) doubles of device memory, 8-byte aligned (the per-block
 * partials; at most 512).  grads_inout 16-byte aligned; OCL_ERR_ARG ("clip: ...") before any launch for a null
 * or misaligned pointer, n <= 0, max_norm negative or NaN, or a workspace that is too small. */
int64_t ocl_clip_workspace_doubles(int64_t n);
int ocl_clip_grad_norm(float* grads_inout, int64_t n, float max_norm, double* workspace, int64_t workspace_doubles,
                       float* info4, void* stream);

/* ---- K6: softmax cross-entropy ---------------------------------------------------------------------
 * torch.nn.CrossEntropyLoss(reduction='mean') (agents/base.py:95,113) and
 * F.cross_entropy(reduction='none') (utils/buffer/mir_retrieve.py:26-27).
 * reduction: 0 = none (loss_out[n]), 1 = mean (loss_out[1]).  dlogits (may be NULL) receives
 * d(loss)/d(logits) for reduction=mean, or d(loss_i)/d(logits_i) per row for reduction=none.
 * A label outside [0, c) (the reference raises) is never used as an address: that row's loss is NaN, so
 * the mean is NaN; its dlogits row is written inside the row only (the softmax, no -1 anywhere); every
 * other row's loss and dlogits have the bits of the same call with a valid label in that row's place.
 * The same holds for the segmented form below (the row's softmax is then empty: its dlogits are 0). */
int ocl_ce_fwd_bwd(const float* logits, const int64_t* y, int n, int c, int reduction,
                   float* loss_out, float* dlogits, void* stream);

/* Cross-entropy (mean) over a column segment: the labels trick (agents/base.py:96-101: softmax over the classes present in
 * the batch) and the separated softmax (:102-108: old and new classes normalised separately) as ONE kernel.  seg[c] assigns
 * every logit column to a segment id >= 0, or -1 (column takes no part); row r is a softmax over the columns j with
 * seg[j] == seg[y[r]] (seg[y[r]] must be >= 0: checked by the caller, the labels live on the host).  dlogits (may be NULL)
 * receives d(mean loss)/d(logits): zero outside the row's segment. */
int ocl_ce_segmented_fwd_bwd(const float* logits, const int64_t* y, const int32_t* seg, int n, int c, float* loss_out,
                             float* dlogits, void* stream);

/* Knowledge-distillation loss of the KD tricks (utils/kd_manager.py:6-11, loss_fn_kd):
 * mean_r(-sum_j softmax(target_r/T)_j * log_softmax(scores_r/T)_j) * T^2; dscores (may be NULL) = d(loss)/d(scores). */
int ocl_kd_fwd_bwd(const float* scores, const float* target_scores, int n, int c, float T, float* loss_out, float* dscores,
                   void* stream);

/* ---- K6b: cross-entropy blended with distillation (Learning without Forgetting) ------------------------
 * agents/lwf.py:36-39 with utils/kd_manager.py:6-11 and agents/base.py:113, loss and gradient in ONE launch:
 *   ce = mean_r(lse(s_r) - s_r[y_r])
 *   kd = mean_r(-sum_j softmax(t_r/T)_j * log_softmax(s_r/T)_j) * T^2          (s = logits, t = teacher)
 *   loss_out[3] = {w_new * ce + w_old * kd, ce, kd}
 *   dlogits[r][j] = w_new * (softmax(s_r)_j - [j == y_r]) / n + w_old * (softmax(s_r/T)_j - softmax(t_r/T)_j) * T / n
 * x / T is a true division, as in ocl_kd_fwd_bwd.  teacher == NULL (LwF's first task, where the reference
 * computes 1 * loss_new + 0 * 0): kd = 0 and the gradient is the CE term alone; with w_new == 1 the
 * cross-entropy and dlogits are then the bits of ocl_ce_fwd_bwd(reduction = mean).  A teacher that equals the
 * logits bit for bit adds exactly 0 to the gradient.  dlogits may be NULL (losses only: the same three values).
 * One workgroup, one wave per row, sums in a fixed order without atomics: two runs give the same bits.  A row
 * of up to 256 columns is read once and held in registers; a longer one is re-read by strided loops.  Ordered
 * on `stream`, no host synchronisation.  OCL_ERR_ARG ("ce_kd_blend: ...") before any launch, nothing written,
 * for n < 1, c < 1, T <= 0, a non-finite T, w_new or w_old, a null logits, y or loss_out, or a dlogits that
 * overlaps logits or teacher. */
int ocl_ce_kd_blend_fwd_bwd(const float* logits, const int64_t* y, const float* teacher, int n, int c, float T, float w_new,
                            float w_old, float* loss_out, float* dlogits, void* stream);

/* ---- K6c: binary cross-entropy against a distilled target (iCaRL) ----------------------------------------
 * agents/icarl.py:42-62, loss and gradient in ONE launch.  s = logits [n, c], t = teacher [n, c],
 * sig(x) = 1 / (1 + exp(-x)); the first n_stream rows are the stream batch, the others memory rows:
 *   z[r][j] = sig(t[r][j])                                   for j <  n_old          (every row)
 *           = 1 if r < n_stream and j == pos[r], else 0      for n_old <= j < n_cls
 *   l[r][j] = max(s, 0) - s * z + log1p(exp(-|s|))
 *   old = (1/n) sum_r sum_{j < n_old} l       new = (1/n) sum_r sum_{n_old <= j < n_cls} l
 *   loss_out[3] = {old + new, old, new}
 *   dlogits[r][j] = (sig(s[r][j]) - z[r][j]) / n  for j < n_cls;  +0.0 for n_cls <= j < c
 * = F.binary_cross_entropy_with_logits(logits[:, :n_cls], target, reduction='none').sum(1).mean() with the
 * reference's target.  pos is int64 [n_stream]; a pos[r] below n_old is overwritten by the teacher's value, one
 * outside [0, n_cls) sets no target.  Logit and teacher columns j >= n_cls and teacher columns j >= n_old are
 * never read (a NaN there changes nothing).  sig(s) and sig(t) come from one function and are rounded before
 * they are subtracted: a teacher that equals the logits bit for bit gives exactly 0 on the old columns.
 * teacher == NULL requires n_old == 0 (iCaRL's first task).  dlogits may be NULL (losses only: the same three
 * values).  One workgroup, one wave per row, element, row and cross-row sums in double and in a fixed order
 * without atomics: two runs give the same bits.  A row of up to 256 columns is held in registers; a longer
 * one takes a strided loop.  Ordered on `stream`, no host synchronisation.  OCL_ERR_ARG ("bce_distill: ...")
 * before any launch, nothing written, for a null logits, pos or loss_out, n < 1, c < 1, n_stream outside
 * [1, n], anything but 0 <= n_old <= n_cls <= c, n_old > 0 without a teacher, or a dlogits that overlaps
 * logits, teacher or pos. */
int ocl_bce_distill_fwd_bwd(const float* logits, const float* teacher, const int64_t* pos, int n, int n_stream, int c, int n_cls,
                            int n_old, float* loss_out, float* dlogits, void* stream);

/* ---- K6e: Dark Experience Replay's loss (DER / DER++) ---------------------------------------------------
 * Buzzega et al., NeurIPS 2020, loss and gradient in ONE launch.  logits is one contiguous block of
 * n0 + n1 + n2 rows of c columns: the stream batch, the logit-replay batch, the label-replay batch.
 *   ce    = mean_{r < n0}(lse(s_r) - s_r[y0_r])
 *   mse   = sum_{r in block 1, j} (s_rj - z_rj)^2 / (n1 * c)        z_r = stored[slots[r]]
 *   ce_m  = mean_{r in block 2}(lse(s_r) - s_r[y2_r])
 *   loss_out[4] = {ce + alpha * mse + beta * ce_m, ce, mse, ce_m}
 *   dlogits: block 0 (softmax - onehot) / n0;  block 1 alpha * 2 * (s - z) / (n1 * c);
 *            block 2 beta * (softmax - onehot) / n2
 * y0 is int64 [n0], y2 int64 [n2], stored float [m, c] (the memory's logit table), slots int64 [n1] or NULL
 * (rows 0 .. n1 - 1 of stored).  n1 == 0 or n2 == 0 is allowed: the term is 0, nothing of it is read, and
 * stored, slots and y2 may then be NULL.  With n1 == n2 == 0 the loss and dlogits are the bits of
 * ocl_ce_fwd_bwd(reduction = mean).  s - z is formed once for the loss and the gradient: a stored row that
 * equals today's row bit for bit gives exactly 0 for both.  A label outside [0, c) is no address: that row's
 * loss is NaN and no one-hot is subtracted.  A slot outside [0, m) is no address: that row's z is NaN and
 * nothing is read.  Block 1 never reads a label.  dlogits may be NULL (losses only: the same four values).
 * One workgroup, one wave per row; the squared error's element, row and cross-row sums and block 2's row
 * losses and their sum in double (block 0's in float: they are ocl_ce_fwd_bwd's); every sum in a fixed order
 * without atomics: two runs give the same bits.  A row of up to 256 columns is held in
 * registers; a longer one takes strided loops.  Ordered on `stream`, no host synchronisation.  OCL_ERR_ARG
 * ("der_loss: ...") before any launch, nothing written, for a null logits, y0 or loss_out, n0 < 1, n1 < 0,
 * n2 < 0, c < 1, n1 > 0 with a null stored or m < 1, n2 > 0 with a null y2, a non-finite alpha or beta, or a
 * dlogits that overlaps logits or stored. */
int ocl_der_fwd_bwd(const float* logits, const int64_t* y0, const int64_t* y2, const float* stored, const int64_t* slots, int n0,
                    int n1, int n2, int c, int m, float alpha, float beta, float* loss_out, float* dlogits, void* stream);

/* ---- K6d: per-row arg-max and group sum (evaluate()'s error analysis) -----------------------------------
 * agents/base.py:179-203 and :217-218.  x is [n, c], row-major and contiguous.  Per row r, in ONE launch:
 *   argmax_out[r] = the smallest column index among the row's maxima; a NaN compares as larger than everything
 *                   and the first NaN wins (torch.max(x, 1) on the CPU); -0.0 and +0.0 are equal
 *   sum_out[r]    = the sum in double of x[r][j] over the columns with col_group[j] == sel
 * col_group is int32 [c]; NULL sums every column.  Columns outside the group are left out by a select, not
 * multiplied by 0: a NaN or Inf there leaves the sum's bits alone; an empty group gives +0.0.  Either output
 * may be NULL (not computed), not both; the one that is computed has the bits it has when both are.  Outputs
 * may point into the middle of larger buffers.  One wave per row, four rows per workgroup; a row of up to 256
 * columns is held in registers, a longer one takes a strided loop; lane l adds its columns l, l + 64, ... in
 * order, then a shuffle tree: no atomics, two runs give the same bits, and a row's results depend neither on n
 * nor on where in the grid it was computed.  Ordered on `stream`, no host synchronisation.  OCL_ERR_ARG
 * ("row_argmax_groupsum: ...") before any launch, nothing written, for a null x, both outputs null, n < 1,
 * c < 1, an output that overlaps x or col_group, or outputs that overlap each other. */
int ocl_row_argmax_groupsum(const float* x, int n, int c, const int32_t* col_group, int sel, int64_t* argmax_out,
                            double* sum_out, void* stream);

/* ---- K7: supervised contrastive loss ---------------------------------------------------------------
 * SupConLoss.forward with contrast_mode='all' (utils/loss.py:19-96).  feat is VIEW-MAJOR
 * [n_views*bsz, dim] (= torch.cat(torch.unbind(features,1)), loss.py:56).  workspace: at least
 * ocl_supcon_workspace_bytes(bsz*n_views).  dfeat may be NULL (loss only). An anchor without any
 * positive (n_views = 1 and a label that occurs once) yields what the reference's 0/0 yields (loss.py:90) under autograd: a NaN
 * loss AND a NaN in every element of dfeat (the 1/0 of that anchor's mean meets the zero mask, 0 * inf, in every logit of its
 * row, and every feature row takes part in that row's logits). */
int64_t ocl_supcon_workspace_bytes(int n_anchor);
int ocl_supcon_fwd_bwd(const float* feat, const int64_t* y, int bsz, int n_views, int dim,
                       float temperature, float* loss_out, float* dfeat, void* workspace,
                       void* stream);

/* ---- K10: kNN Shapley values -----------------------------------------------------------------------
 * sorted_cand_ind + compute_knn_sv on precomputed deep features (utils/buffer/aser_utils.py:7-61,
 * 94-116; distance = sum((u-v)^2), utils/utils.py:93-95).  One workgroup per evaluation row:
 * distances -> LDS bitonic sort (ties broken by ascending candidate index) -> label indicator ->
 * closed-form suffix recursion -> scatter to candidate order.  n_cand <= OCL_KNN_MAX_CAND.
 * sorted_idx (may be NULL) receives the per-row ascending-distance candidate order.
 * The per-row order is total: ascending distance, ties by ascending candidate index (+inf is an ordinary
 * distance); then every candidate whose distance is NaN (a NaN in either row, or +inf in the same dimension
 * of both), in index order; then, unseen by the caller, the sort's padding, which is known by its index and
 * not by its key.  That is torch.argsort(distance, stable=True) on the CPU.  So for EVERY input sorted_idx[e]
 * is a permutation of 0 .. n_cand - 1 and every cell of sv_out is written; the recursion reads labels and
 * ranks only, so every value is finite whatever the features hold. */
#define OCL_KNN_MAX_CAND 2048
int ocl_knn_sv(const float* eval_f, const int64_t* eval_y, int n_eval, const float* cand_f,
               const int64_t* cand_y, int n_cand, int dim, int k, float* sv_out,
               int64_t* sorted_idx, void* stream);
/* column reduction over the evaluation rows: mode 0 sum, 1 mean, 2 max, 3 min
 * (aser_retrieve.py:79-86, aser_update.py:80). */
int ocl_col_reduce(const float* m, int rows, int cols, int mode, float* out, void* stream);
/* ASER score (aser_retrieve.py:77-86): type 0 "asvm": coop.mean(0) - adv.mean(0); 1 "asv":
 * coop.max(0) - adv.min(0); 2 "neg_sv": -adv.sum(0) (coop ignored, may be NULL). */
int ocl_aser_score(const float* sv_adv, int n_adv, const float* sv_coop, int n_coop, int n_cand,
                   int type, float* out, void* stream);
/* sv.argsort(descending=True) (aser_retrieve.py:88, aser_update.py:88; scores.sort(descending)
 * mir_retrieve.py:29).  Deterministic: ties keep ascending index (-0.0 and +0.0 are a tie).  NaN sorts first, before +inf, in
 * index order among NaNs: torch.argsort(descending=True, stable=True).  n <= OCL_SORT_MAX. */
#define OCL_SORT_MAX 4096
int ocl_argsort_desc(const float* v, int n, int64_t* idx_out, void* stream);

/* ---- K11: nearest-class-mean classifier ------------------------------------------------------------
 * agents/base.py:121-142 (means) and :159-176 (predict).  feat rows are L2-normalised, averaged per
 * class, the mean re-normalised.  class_ids[n_cls] lists the labels in `old_labels` order; a class
 * with no exemplar gets count 0 and its mean row is left untouched (the caller fills it the way the
 * reference does, base.py:135-137).  predict returns argmin_j ||f/|f| - mean_j||^2 as an index
 * into class_ids (first minimum wins, like torch.min; a NaN distance counts as smaller than every
 * number and the first NaN wins, as dists.min(1) has it on the CPU). */
int ocl_ncm_class_means(const float* feat, const int64_t* labels, int n, int d,
                        const int64_t* class_ids, int n_cls, float* means_out, int32_t* counts_out,
                        void* stream);
int ocl_ncm_predict(const float* feat, int n, int d, const float* means, int n_cls,
                    int64_t* pred_out, void* stream);

/* ---- K12: MIR interference score -------------------------------------------------------------------
 * post_loss - pre_loss with per-sample CE (utils/buffer/mir_retrieve.py:26-28).  A label outside
 * [0, c) is never used as an address: that row's score is NaN, every other row's bits are unchanged (K6). */
int ocl_mir_scores(const float* logits_pre, const float* logits_post, const int64_t* y, int n,
                   int c, float* scores_out, void* stream);

/* ---- GSS-Greedy: gradient-direction similarity ------------------------------------------------------
 * max_i cosine_similarity(mem[i], g) over k stored flat gradient vectors of n floats (utils/buffer/buffer_utils.py:51-56:
 * x1.x2 / max(|x1||x2|, eps); call sites utils/buffer/gss_greedy_update.py:79,121 `max(cosine_similarity(mem_grads, grad))`).
 * workspace: ocl_cosine_max_workspace_bytes(k) bytes. out: one float. */
int64_t ocl_cosine_max_workspace_bytes(int k);
int ocl_cosine_max(const float* mem, int k, int64_t n, const float* g, float eps, float* out, void* workspace, void* stream);

/* ---- K13: SCR view augmentation --------------------------------------------------------------------
 * stands in for the kornia pipeline of agents/scr.py:18-24 (RandomResizedCrop -> HorizontalFlip ->
 * ColorJitter -> RandomGrayscale); kornia 0.4.1's RNG parameterisation is unpinned, so
 * the per-sample parameters are drawn on the host and passed in.  params: n rows of
 * OCL_AUG_NPARAM floats: [y0,x0,crop_h,crop_w (input pixels, fractional), flip(0/1),
 * jitter_on(0/1), brightness, contrast, saturation, hue (fraction of a turn), order (0..23 index
 * of the permutation of the four jitter ops), gray(0/1)]. x, out: [n,3,h,w] fp32 in [0,1].
 * Given the parameters the result is fully determined (tests/augment_ref.py states it in float64).  Output pixel (oy, ox), in order:
 *   1. flip: the column read is ox' = w - 1 - ox if flip, else ox (the flip comes BEFORE the source coordinate: the crop box keeps
 *      its place in the input, its content is mirrored);
 *   2. crop + resize, half-pixel centres: sy = y0 + (oy + 0.5) * crop_h / h - 0.5, sx = x0 + (ox' + 0.5) * crop_w / w - 0.5, each
 *      clamped to the IMAGE, [0, h - 1] and [0, w - 1] (not to the crop box: near the box's edge the neighbours outside it are
 *      read), then bilinear between floor(s) and min(floor(s) + 1, size - 1), per channel;
 *   3. if jitter_on: the four operations 0 brightness, 1 contrast, 2 saturation, 3 hue in the order given by `order`, the index
 *      into the 24 permutations of (0, 1, 2, 3) in lexicographic order (0: 0123, 1: 0132, ... 23: 3210).  brightness:
 *      clamp01(c + (brightness - 1)); contrast: clamp01(c * contrast); saturation: to HSV, s = clamp01(s * saturation), back;
 *      hue: to HSV, h = h + hue (a fraction of a turn, any real number), back.  HSV is the usual hexcone: v = max, s = (max - min) /
 *      max (0 for black), h in [0, 1) from the channel that is the maximum (r first, then g, on ties), 0 for a gray; the way back
 *      takes the fractional part of h;
 *   4. if gray: all three channels become 0.299 r + 0.587 g + 0.114 b.
 * n <= 65535 (one grid row per image) and h * w <= 2^31 - 256 (pixel indices are int): anything larger is refused with OCL_ERR_ARG
 * before a launch. */
#define OCL_AUG_NPARAM 12
int ocl_scr_augment(const float* x, float* out, int n, int h, int w, const float* params,
                    void* stream);
/* Same, with the parameter arithmetic on the device: u holds n rows of OCL_AUG_NUNIFORM raw U[0,1) draws (host generator,
 * one torch.rand call as before): [0,10) crop areas, [10,20) crop log-ratios of the 10 attempts RandomResizedCrop makes,
 * [20,30) position y / x, flip, jitter-on, brightness, contrast, saturation, hue, order, gray.  cfg12 (HOST array):
 * scale_lo, scale_hi, ratio_lo, ratio_hi, brightness, contrast, saturation, hue, p_jitter, p_gray, fallback crop w, h.
 * params [n, OCL_AUG_NPARAM] (device) receives the derived per-image parameters (the layout ocl_scr_augment takes). */
#define OCL_AUG_NUNIFORM 30
int ocl_scr_augment_uniform(const float* x, float* out, int n, int h, int w, const float* u, const double* cfg12,
                            float* params, void* stream);

/* ---- small dense GEMM (K5 helper; exposed for tests) ----------------------------------------------
 * C[m,n] = A(m,k) * B(k,n) (+ bias[n]) (relu) with arbitrary element strides, exact-fp32 MFMA
 * 16x16x4.  Used for nn.Linear fwd/bwd (models/resnet.py:79,103,148-152). */
int ocl_gemm_small(const float* a, int64_t a_rs, int64_t a_cs, const float* b, int64_t b_rs,
                   int64_t b_cs, float* c, int64_t c_rs, int m, int n, int k, const float* bias,
                   int relu, int accumulate, void* stream);

/* ---- K1-K5: Reduced-ResNet18 engine ----------------------------------------------------------------
 * One object per model (models/resnet.py:69-116 Reduced_ResNet18; :140-168 SupConResNet).  The
 * parameter order/layout is exactly PyTorch's named_parameters() order of the reference module, as
 * one flat fp32 array (so the flat gradient IS the vector get_grad_vector builds,
 * utils/buffer/buffer_utils.py:58-71).  All BatchNorm running statistics live in one flat array:
 * per BN, running_mean[C] then running_var[C], in module order; num_batches_tracked is int64[n_bn].
 */
typedef struct ocl_net ocl_net;

typedef struct {
    int32_t in_h, in_w;     /* 32x32 (CIFAR) or 84x84 (Mini-ImageNet), utils/setup_elements.py:11-17 */
    int32_t nf;             /* 20 (Reduced_ResNet18, models/resnet.py:112-116) */
    int32_t n_classes;      /* size of the encoder's `linear` (always present as parameters) */
    int32_t head;           /* 0: logits = linear(features)           (ResNet.forward, :106-109)
                               1: normalize(mlp(features))            (SupConResNet head='mlp')
                               2: normalize(linear_head(features))    (head='linear')
                               3: normalize(features)                 (head='None') */
    int32_t feat_dim;       /* 128: SupCon projection size (head 1,2) */
    int32_t max_batch;      /* largest n ever passed to forward */
    int32_t n_slots;        /* activation tapes kept alive for backward (>=1) */
} ocl_net_desc;

int ocl_net_create(const ocl_net_desc* desc, ocl_net** out);
void ocl_net_destroy(ocl_net* net);

int64_t ocl_net_param_count(const ocl_net* net);       /* floats in the flat parameter array */
int32_t ocl_net_num_tensors(const ocl_net* net);       /* parameter tensors, named_parameters() order */
/* name (<=63 chars + NUL), flat offset, ndim<=4, shape */
int ocl_net_tensor_info(const ocl_net* net, int i, char* name64, int64_t* offset, int32_t* ndim,
                        int64_t* shape4);
int32_t ocl_net_num_bn(const ocl_net* net);
int64_t ocl_net_bn_stat_count(const ocl_net* net);     /* floats in the flat running-stat array */
int ocl_net_bn_info(const ocl_net* net, int i, char* name64, int64_t* offset, int32_t* channels);
int32_t ocl_net_feature_dim(const ocl_net* net);        /* 160 (32x32) / 640 (84x84) */
int32_t ocl_net_out_dim(const ocl_net* net);            /* n_classes, feat_dim or feature_dim */
int64_t ocl_net_workspace_bytes(const ocl_net* net);

/* Binds caller-owned storage. params/grads: param_count floats; running: bn_stat_count floats;
 * nbt: int64[num_bn]; workspace: workspace_bytes, 256-B aligned. */
int ocl_net_bind(ocl_net* net, float* params, float* grads, float* running, int64_t* nbt,
                 void* workspace, int64_t workspace_bytes);

#define OCL_FWD_TRAIN 1u          /* BatchNorm uses batch statistics (model.train()) */
#define OCL_FWD_SAVE_TAPE 2u      /* keep activations in `slot` for ocl_net_backward */
#define OCL_FWD_UPDATE_RUNNING 4u /* momentum-0.1 running-stat update (nn.BatchNorm2d default);
                                     applied once per group, in group order */
#define OCL_FWD_FROZEN_BN 8u      /* with OCL_FWD_SAVE_TAPE and without OCL_FWD_TRAIN: eval-mode BatchNorm (running statistics) but
                                     the activations are kept, so that ocl_net_backward gives the gradients of an eval-mode
                                     forward: model.eval() followed by loss.backward(), utils/buffer/gss_greedy_update.py:16,
                                     77-79,97-100,116-118 */
#define OCL_FWD_SAME_WEIGHTS 16u  /* the caller asserts that the parameter array of this call has not been written since this net's
                                     previous forward read it (several forwards between two optimiser steps: the ASER retrieval's
                                     feature pass, the memory pass and the combined pass of agents/exp_replay.py:49-84): the engine
                                     reuses the weight packs it made then instead of re-packing (it still re-packs when its arena
                                     holds another array's packs, e.g. after a params_override call) */
#define OCL_FWD_PACK_ALL 32u      /* with a pass that packs (no OCL_FWD_SAME_WEIGHTS, or refused): also write the data-gradient packs
                                     although this pass keeps no tape -- a taped pass on the same weights will follow */
/* x: [n,3,H,W] fp32 NCHW (what the reference's agents hand to model.forward).
 * groups: the batch is `groups` equal consecutive sub-batches that the reference would have run as
 * separate forward calls (SCR's two views, agents/scr.py:55): BatchNorm statistics are per group.
 * params_override: NULL = bound params; else another flat parameter array (MIR's virtual model,
 * mir_retrieve.py:21,25).  feat_out [n,feature_dim] and out [n,out_dim] may each be NULL. */
int ocl_net_forward(ocl_net* net, const float* x, int n, int groups, uint32_t flags,
                    const float* params_override, float* feat_out, float* out, int slot,
                    void* stream);
/* The same pass over a batch given as `nseg` (1..8) separate tensors xs[i] of ns[i] images each, in batch order: the reference's
 * torch.cat((mem_x, batch_x)) (agents/exp_replay.py:78, agents/scr.py:52) and its one-forward-call-per-view (agents/scr.py:55),
 * torch.cat((eval_x, cand_x)) of utils/buffer/aser_utils.py:73 -- without materialising the concatenation: the engine's layout
 * conversion reads the segments where they are. */
int ocl_net_forward_segments(ocl_net* net, const float* const* xs, const int32_t* ns, int nseg, int groups, uint32_t flags,
                             const float* params_override, float* feat_out, float* out, int slot, void* stream);
/* Backward of the forward recorded in `slot`. dout: [n,out_dim] = d(loss)/d(out).
 * accumulate=0 overwrites the bound flat gradient, 1 adds to it (loss.backward() twice,
 * agents/exp_replay.py:55,77).  Tensors that take no part in the forward (SupConResNet's
 * encoder.linear) get zero / are left untouched respectively. */
int ocl_net_backward(ocl_net* net, int slot, const float* dout, int accumulate, void* stream);

/* Test hooks. debug_stop: make ocl_net_backward return right after stage block*10+step (step 1: bn2 backward,
 * 2: conv2 data gradient, 3: bn1 backward, 4: conv1 data gradient, 5: block input gradient complete; -1: off).
 * debug_copy what: 0 raw conv output (NHWC) of conv `index`; 1 output of block `index`; 2 gradient scratch buffer
 * `index`; 3 gradient buffer by role (0..4 = gA..gE) at the last stop; 4 activation a1 of block `index`; 5 stem output. */
int ocl_net_debug_stop(ocl_net* net, int stage);
int ocl_net_debug_copy(ocl_net* net, int slot, int what, int index, float* dst, int64_t max_floats,
                       int64_t* n_written, void* stream);

/* ---- kernel-level entry points (single layers; tests and micro-benchmarks) ------------------------------
 * BatchNorm2d backward (train mode) fused with the ReLU mask that follows it: dpre = dz * (zmask > 0) (zmask NULL =
 * no ReLU); dy = gamma*invstd*(dpre - mean(dpre) - xhat*mean(dpre*xhat)); dgamma = sum(dpre*xhat), dbeta = sum(dpre).
 * Tensors are NHWC [groups*m_per_group, c]; mean/invstd are [groups, c]. scratch: groups*2*c accumulator cells of 16 bytes
 * (= groups*4*c doubles, 16-byte aligned).  The batch sums follow ocl_set_deterministic (fp64 atomics, or fixed-point integers);
 * no arrival scratch is passed, so the one-pass kernel is never taken here (ocl_test_bn_bwd reaches it). */
int ocl_bn_bwd_nhwc(const float* dz, const float* zmask, const float* y, const float* mean, const float* invstd,
                    const float* gamma, int64_t m_per_group, int groups, int c, float* dy, float* dgamma,
                    float* dbeta, int accumulate, double* scratch, void* stream);

/* Single-layer test hooks (tests/test_gpu_layers.py, tests/test_cpu_forms.py).  They plan, finalize, pack and launch through the
 * engine's own functions and add no kernel.  Device scratch (weight packs, plan tables, split-K slabs, arrival counters) is allocated
 * and freed inside; every call synchronises `stream`.  Accumulator cells ("stats") are the engine's 16-byte cells, laid out
 * [8 replicas][groups][2][C] with replica stride groups*2*C cells; the caller zeroes them. */
#define OCL_EPI_STATS 1      /* + per-(group, channel) sum / sum of squares into stats */
#define OCL_EPI_AFFINE 2     /* out = acc*scale[c] + shift[c] */
#define OCL_EPI_RES 4        /* out += res */
#define OCL_EPI_RESMASK 8    /* out += res * (resmask > 0) */
#define OCL_EPI_RELU 16      /* out = max(out, 0) */
#define OCL_EPI_ACCUM 32     /* out = out_old + value */
#define OCL_EPI_BNB 64       /* data gradient feeding a BatchNorm backward: ReLU mask + that BatchNorm's two sums into stats */

/* One convolution layer of Reduced-ResNet18 and the pass it is planned for.  cin = 3: the stem (input tensor NHWC with 4 channels,
 * the fourth zero).  dir 0: forward (in = x [n,hin,win,cinT], out = y [n,ho,wo,cout]); dir 1: data gradient (in = dy, out = dx).
 * merge (dir 1, 3x3 stride 2): 1 = the four parity classes as one launch where it plans (the engine's choice), 0 = four launches.
 * xf / bnb: the LDS reservations of the input transform / the EPI_BNB epilogue (ConvGeomDesc); bnb also makes the data-gradient tiles
 * follow the groups.  force_*: ConvGeomDesc's overrides (0 = planner). */
typedef struct {
    int32_t cin, cout, k, stride, hin, win;
    int32_t n, groups, dir, merge, xf, bnb;
    int32_t force_mt, force_nt, force_pipe, force_q4, force_cs, force_cw;
} ocl_test_conv_desc;
/* family: 0 conv_t_kernel, 1 conv_q_kernel, 2 conv_s_kernel, 3 conv_w_kernel, 4 conv_wx_kernel.  pipe: 1 three-buffer ring; wres: 1
 * resident weights (else two buffers); ncls: output classes of the launch; pf: patch prefetch units per thread of the instantiation;
 * bnb_room: the plan reserved the EPI_BNB table. */
typedef struct {
    int32_t family, mt, nt, q4, pipe, wres, ncls, pf, bnb_room, grid_x, grid_y, reserved;
} ocl_test_conv_form;
/* The launches of a layer (1, or the 4 parity classes): returns their count (<= cap forms written) or < 0.  Host only. */
int ocl_test_conv_plan(const ocl_test_conv_desc* desc, ocl_test_conv_form* forms, int cap);
typedef struct {
    const float* in;
    const float* w;          /* OIHW [cout, cin, k, k] (packed here by the engine's pack kernel) */
    float* out;
    int32_t flags;           /* OCL_EPI_* */
    int32_t xf;              /* apply the input transform (needs desc->xf) */
    const float *scale, *shift, *res, *resmask;
    void* stats;             /* EPI_STATS / EPI_BNB cells over the output channels */
    const void* xf_stats;    /* producer's cells over the input channels (filled by its EPI_STATS launch) */
    const float *xf_gamma, *xf_beta;
    float *xf_save_mean, *xf_save_invstd, *xf_running_mean, *xf_running_var;
    int64_t* xf_nbt;
    const float *bnb_y, *bnb_z, *bnb_mean, *bnb_invstd, *bnb_gamma, *bnb_beta;
} ocl_test_conv_ops;
/* Runs every launch of the layer (forms: <= cap written); returns the launch count or < 0. */
int ocl_test_conv(const ocl_test_conv_desc* desc, const ocl_test_conv_ops* ops, ocl_test_conv_form* forms, int cap, void* stream);

/* Weight gradient of one layer (plan_wgrad's inputs): x [n,hin,win,cinT], dy [n,ho,wo,cout] -> grad OIHW. */
typedef struct {
    int32_t cin, cout, k, stride, hin, win, n, xf_groups, wg_target, reserved;
} ocl_test_wgrad_desc;
/* q_rgw > 0: the 4x4x1 form; multi: form index inside conv_wgrad_multi_kernel (-1: none); s: pixel splits */
typedef struct {
    int32_t mtw, ntw, q_rgw, pf, multi, s, grid_x, grid_y;
} ocl_test_wgrad_form;
typedef struct {
    const float* x;
    const float* dy;
    float* grad;             /* multi: every layer's grad inside ONE array, the first layer's first */
    int32_t xf;              /* x is a raw conv output: apply max(fma(x, scale, shift), 0) of its BatchNorm while staging */
    int32_t reserved;
    const float *xf_mean, *xf_invstd, *xf_gamma, *xf_beta;
} ocl_test_wgrad_ops;
/* multi 0: per layer launch_wgrad + launch_wgrad_reduce; 1: the layers in one conv_wgrad_multi_kernel launch (all of one form set) +
 * one launch_wgrad_reduce_multi.  ops may be NULL (plan only, host).  Returns 0 or < 0. */
int ocl_test_wgrad(const ocl_test_wgrad_desc* descs, const ocl_test_wgrad_ops* ops, int n_layers, int multi, int accumulate,
                   ocl_test_wgrad_form* forms, void* stream);

/* BatchNorm forward from the cells of the producing conv (launch_bn_fwd): every BnFwdArgs field the engine uses, the second set (_b:
 * the projection shortcut's BatchNorm, z = relu(bn(y) + bn_b(yb))) included; yb NULL = none, frozen_* NULL = batch statistics. */
typedef struct {
    const float* y; float* z; const float* res; const void* stats;
    const float *gamma, *beta; float *running_mean, *running_var; int64_t* nbt; float *save_mean, *save_invstd;
    const float *frozen_mean, *frozen_var;
    const float* yb; const void* stats_b; const float *gamma_b, *beta_b; float *running_mean_b, *running_var_b; int64_t* nbt_b;
    float *save_mean_b, *save_invstd_b; const float *frozen_mean_b, *frozen_var_b;
    int64_t m_per_group; int32_t groups, c, relu; float momentum, eps; int32_t reserved;
} ocl_test_bn_fwd_args;
int ocl_test_bn_fwd(const ocl_test_bn_fwd_args* a, void* stream);
/* BatchNorm backward (launch_bn_bwd): nsets 1 or 2, frozen, mask_from_y (needs beta).  one_pass = 1 allocates the arrival counter and
 * the replicated accumulators so that the one-pass kernel can be chosen.  Returns the path that ran (>= 0) or < 0:
 * 1000 + 10*U + nsets: bn_bwd_chan_kernel<U, nsets>; 2000 + 10*U + nsets: bn_bwd_fused_kernel<U, nsets>; 3000 + nsets: reduce + apply. */
typedef struct {
    const float* dz; const float* z;
    const float* y[2]; const float* mean[2]; const float* invstd[2]; const float* gamma[2]; const float* beta[2];
    float* dy[2]; float* dgamma[2]; float* dbeta[2];
    int64_t m_per_group; int32_t groups, c, nsets, accumulate, frozen, mask_from_y, one_pass, reserved;
} ocl_test_bn_bwd_args;
int ocl_test_bn_bwd(const ocl_test_bn_bwd_args* a, void* stream);
/* Apply half after an EPI_BNB data gradient (launch_bn_apply_e): d = the masked gradient that launch wrote, esums = its cells. */
int ocl_test_bn_apply_e(const float* d, const float* y, const float* mean, const float* invstd, const float* gamma, const void* esums,
                        int64_t m_per_group, int groups, int c, float* dy, float* dgamma, float* dbeta, int accumulate, void* stream);

/* Every form the network engine plans for one pass of Reduced-ResNet18 (hw x hw input, nf filters): n images in `groups` BatchNorm
 * groups, train (forward + data gradients + weight gradients) or eval (forward only; n as the engine plans it, i.e. already rounded).
 * Made by the function the engine's own plan cache calls.  One entry per launch geometry; returns the entry count (<= cap written). */
typedef struct {
    int32_t layer, dir, wg_merged, reserved;   /* conv index in module order; dir 0 fwd, 1 data gradient, 2 weight gradient */
    ocl_test_conv_desc desc;                   /* dir 0 / 1 */
    ocl_test_conv_form form;
    ocl_test_wgrad_desc wdesc;                 /* dir 2 */
    ocl_test_wgrad_form wform;
} ocl_test_net_form;
int ocl_test_net_forms(int hw, int nf, int n, int groups, int train, ocl_test_net_form* out, int cap);

/* ---- the glue kernels and the head chain on their own (tests/test_gpu_aux.py) ------------------------
 * Like the hooks above: no kernel of their own, the engine's launch_* functions, device scratch allocated and freed inside, the stream
 * synchronised before they return.
 *
 * ocl_test_aux: one launcher of csrc/conv_aux.hip / csrc/bn.hip per op code.  Operands in p[], sizes in i[], scalars in f[]:
 *   LAYOUT          p0 = const float* const xs[i0] (host list of device tensors [ns[k],3,i1,i2]), p1 = const int32_t ns[i0] (host),
 *                   p2 = out [sum ns, i1, i2, 4]; 1 <= i0 <= 8 segments (one segment: the plain kernel, as in the engine)
 *   AVGPOOL_FWD     p0 = z [i0,i1,i2,i3] (N,H,W,C), p1 = feat [N, C*(H/4)*(W/4)]
 *   AVGPOOL_BWD     p0 = dfeat, p1 = dz, sizes as above
 *   L2NORM_FWD      p0 = v [i0,i1], p1 = out, p2 = norms [i0], p3 = out2 (may be null)
 *   L2NORM_BWD      p0 = out, p1 = norms, p2 = dout, p3 = dv; i0 rows of i1
 *   RELU_BWD        p0 = dy, p1 = a, p2 = dx (may be dy: in place); i0 elements
 *   COLSUM          p0 = m [i0,i1], p1 = out [i1]; i2 = accumulate
 *   FILL            p0 = p, i0 elements of f0 (i0 == 0: returns before launching)
 *   BN_FOLD         the whole network's BatchNorm table (i0 = hw, i1 = nf): p0 = params (ocl_net_param_count floats), p1 = running
 *                   (ocl_net_bn_stat_count floats), p2 = out (same layout as running: scale[C], shift[C] per BatchNorm); f0 = eps
 *   BN_APPLY_SAVED  p0 = y [i1 groups][i0 = m_per_group][i2 = C], p1 = mean [groups][C], p2 = invstd, p3 = gamma [C], p4 = beta, p5 = z */
enum { OCL_AUX_LAYOUT = 0, OCL_AUX_AVGPOOL_FWD = 1, OCL_AUX_AVGPOOL_BWD = 2, OCL_AUX_L2NORM_FWD = 3, OCL_AUX_L2NORM_BWD = 4,
       OCL_AUX_RELU_BWD = 5, OCL_AUX_COLSUM = 6, OCL_AUX_FILL = 7, OCL_AUX_BN_FOLD = 8, OCL_AUX_BN_APPLY_SAVED = 9 };
typedef struct {
    const void* p[8];
    int64_t i[8];
    float f[2];
} ocl_test_aux_args;
int ocl_test_aux(int op, const ocl_test_aux_args* a, void* stream);

/* The engine's single multi-layer weight-pack launch for the whole network (hw x hw input, nf filters), with the engine's own PackDesc
 * table.  mask: 1 forward packs, 2 data-gradient packs, 3 both.  zero_a / zero_b: two arrays of 16-byte accumulator cells the same launch
 * clears (may be null / 0 cells: the launch has no clearing row then).  table (may be null): per layer, in module order, the 9 values
 * w_off, tf_off, td_off, Cout, Cin, ntaps, CinP, CoutP, CiP (offsets in floats into params / arena; -1: no such pack), at most table_cap
 * layers.  sizes (may be null): [0] floats of the parameter array, [1] floats of the arena.  arena == NULL: only fills table / sizes.
 * The launch writes pack elements only: padding rows / columns and unselected packs keep what the caller put there.
 * Returns the number of layers, or an error code (< 0). */
int ocl_test_pack_all(int hw, int nf, int mask, const float* params, float* arena, void* zero_a, int64_t zero_a_cells, void* zero_b,
                      int64_t zero_b_cells, int64_t* table, int table_cap, int64_t* sizes, void* stream);

/* head_forward on a caller-supplied feature batch, then the head half of ocl_net_backward (the very function that entry point calls),
 * for a net of the given head kind (0 linear classifier, 1 MLP, 2 linear projection, 3 none), input size and class / projection counts.
 * params / grads: flat arrays in the net's tensor layout (ocl_net_tensor_info; n_params floats); only the head's tensors are touched.
 * feat [n, FD], dout [n, out_dim] in; every stage tensor out: h1 [n, FD] (kind 1), h2 [n, out_dim] before normalisation (kinds 1, 2),
 * norms [n] (kinds 1-3), out [n, out_dim], dh2 [n, out_dim] (kinds 1, 2), dh1 [n, FD] after the ReLU mask (kind 1), dfeat [n, FD]; tensors a
 * kind does not have may be null.  The head's weight / bias gradients go to grads (accumulate as ocl_net_backward).  The stream decision
 * is the engine's: side_stream reports whether the weight / bias gradients ran on the side stream (ocl_test_head_side_min_batch: the
 * smallest n of an hw x hw input for which they do; 0: never in this process). */
typedef struct {
    int32_t head, hw, nf, n, n_classes, feat_dim, accumulate, side_stream;
    int64_t n_params;
    const float* params; float* grads; const float* feat; const float* dout;
    float* h1; float* h2; float* norms; float* out; float* dh2; float* dh1; float* dfeat;
} ocl_test_head_args;
int ocl_test_head(ocl_test_head_args* a, void* stream);
int ocl_test_head_side_min_batch(int hw);

/* ---- which path a small-op entry point takes (tests) ------------------------------------------------
 * Host-only (no launch, no GPU): the kernel variant, grid and LDS size that the small-op entry points (one file of csrc/ per kernel family) choose for the
 * given sizes and pointer VALUES (only their alignment is looked at; nothing is dereferenced).  The entry points call the same
 * functions (csrc/small_ops.h) to launch, so the answer cannot drift from what runs.  tests/test_cpu_small_ops.py requires a parity case in
 * tests/small_op_cases.py for every OCL_PATH_* below.  args (int64 each), by op:
 *   ROWS        src, dst, row_bytes, n                  (ocl_gather_rows / ocl_scatter_rows)
 *   PAIR        src_a, dst_a, row_bytes_a, row_bytes_b, n
 *   U8          n, h, w, c
 *   SGD         params, grads, out, n
 *   COSINE      mem, g, k, n
 *   CE          n, c, reduction      CE_SEG / KD / MIR: n, c
 *   SUPCON      feat, bsz, n_views, dim, want_grad
 *   KNN         cand_f, n_eval, n_cand, dim, k
 *   COL_REDUCE  rows, cols           ASER: n_cand
 *   ARGSORT     n
 *   NCM_MEANS   d, n_cls             NCM_PREDICT: n, d, n_cls
 *   GEMM        m, n, k
 *   AUGMENT     n, h, w              (ocl_scr_augment, and the image launch of ocl_scr_augment_uniform)
 *   AUG_PARAMS  n                    (the parameter launch of ocl_scr_augment_uniform)
 * Returns the OCL_PATH_* code (> 0) and fills *plan (may be NULL); 0 for an unknown op or a wrong argument count.  A *_REFUSED code
 * means the entry point returns OCL_ERR_ARG on the host before any launch. */
enum {
    OCL_SOP_ROWS = 0, OCL_SOP_PAIR = 1, OCL_SOP_U8 = 2, OCL_SOP_SGD = 3, OCL_SOP_COSINE = 4, OCL_SOP_CE = 5, OCL_SOP_CE_SEG = 6,
    OCL_SOP_KD = 7, OCL_SOP_MIR = 8, OCL_SOP_SUPCON = 9, OCL_SOP_KNN = 10, OCL_SOP_COL_REDUCE = 11, OCL_SOP_ASER = 12,
    OCL_SOP_ARGSORT = 13, OCL_SOP_NCM_MEANS = 14, OCL_SOP_NCM_PREDICT = 15, OCL_SOP_GEMM = 16,
    OCL_SOP_AUGMENT = 17, OCL_SOP_AUG_PARAMS = 18
};
enum {
    OCL_PATH_ROWS_COPY16 = 1,          /* 16-byte units (row_bytes % 16 == 0, src and dst 16-byte aligned), grid.y < 8 */
    OCL_PATH_ROWS_COPY16_YCAP = 2,     /* ... grid.y at its cap of 8 (rows > 112 KB) */
    OCL_PATH_ROWS_COPY4 = 3,           /* 4-byte units */
    OCL_PATH_ROWS_COPY4_YCAP = 4,      /* ... grid.y = 8 (rows > 28 KB) */
    OCL_PATH_PAIR_FUSED = 5,           /* one rows_gather_pair launch, b's row in one trip (<= 256 units of 4 bytes) */
    OCL_PATH_PAIR_FUSED_BLOOP = 6,     /* ... b's row takes several trips */
    OCL_PATH_PAIR_FALLBACK = 7,        /* a not 16-byte copyable: two rows_copy launches */
    OCL_PATH_U8_GATHER = 8,
    OCL_PATH_SGD_VEC = 9,              /* n % 4 == 0 */
    OCL_PATH_SGD_TAIL = 10,            /* scalar tail of 1 - 3 elements */
    OCL_PATH_SGD_GRID_CAP = 11,        /* 2048 workgroups: the grid-stride loop takes more than one trip */
    OCL_PATH_SGD_REFUSED = 12,         /* a pointer that is not 16-byte aligned */
    OCL_PATH_COS_VEC_ONE = 13,         /* float4 loads; one workgroup */
    OCL_PATH_COS_VEC_MULTI = 14,
    OCL_PATH_COS_VEC_CAP = 15,         /* 512 workgroups */
    OCL_PATH_COS_SCALAR_ONE = 16,      /* n % 4 != 0, or mem / g not 16-byte aligned */
    OCL_PATH_COS_SCALAR_MULTI = 17,
    OCL_PATH_COS_SCALAR_CAP = 18,
    OCL_PATH_CE_NONE = 19,
    OCL_PATH_CE_MEAN = 20,
    OCL_PATH_CE_SEG = 21,
    OCL_PATH_KD = 22,
    OCL_PATH_MIR = 23,
    OCL_PATH_SUPCON_VEC_TAIL = 24,     /* supcon_rows: 16-byte dot product (dim % 4 == 0, feat aligned); supcon_grad: A % 16 != 0 */
    OCL_PATH_SUPCON_VEC_NOTAIL = 25,
    OCL_PATH_SUPCON_VEC_LOSS = 26,     /* dfeat == NULL: supcon_grad is one workgroup that reduces the loss */
    OCL_PATH_SUPCON_SCALAR_TAIL = 27,
    OCL_PATH_SUPCON_SCALAR_NOTAIL = 28,
    OCL_PATH_SUPCON_SCALAR_LOSS = 29,
    OCL_PATH_SUPCON_REFUSED = 30,      /* A > 8192 or dim > 4096 */
    OCL_PATH_KNN_VEC_UNROLL = 31,      /* one thread per candidate, 16-byte loads: dim / 4 a multiple of 4 (unrolled loop only) */
    OCL_PATH_KNN_VEC_REM = 32,         /* dim / 4 < 4 (remainder loop only) */
    OCL_PATH_KNN_VEC_BOTH = 33,        /* both loops in one row */
    OCL_PATH_KNN_WAVE = 34,            /* dim % 4 != 0 or cand_f misaligned: one wave per candidate */
    OCL_PATH_KNN_REFUSED = 35,         /* n_cand > OCL_KNN_MAX_CAND */
    OCL_PATH_COL_REDUCE = 36,
    OCL_PATH_ASER_SCORE = 37,
    OCL_PATH_ARGSORT_FULL = 38,        /* n a power of two: no padding entries */
    OCL_PATH_ARGSORT_PADDED = 39,
    OCL_PATH_ARGSORT_REFUSED = 40,     /* n > OCL_SORT_MAX */
    OCL_PATH_NCM_MEANS = 41,
    OCL_PATH_NCM_PREDICT = 42,
    OCL_PATH_GEMM_K16 = 43,            /* k % 16 == 0: the unrolled loop only */
    OCL_PATH_GEMM_KTAIL = 44,          /* k < 16: the 4-wide tail loop only */
    OCL_PATH_GEMM_KBOTH = 45,
    OCL_PATH_AUGMENT = 46,             /* augment_kernel: ceil(h w / 256) x n workgroups of 256, one thread per output pixel */
    OCL_PATH_AUGMENT_REFUSED = 47,     /* n > 65535 (grid.y) or h w > 2^31 - 256 (int pixel index) */
    OCL_PATH_AUG_PARAMS = 48           /* aug_params_kernel: ceil(n / 64) workgroups of 64, one thread per image */
};
typedef struct {
    int32_t path;                      /* OCL_PATH_* */
    int32_t aux;                       /* cosine: workgroups; knn / argsort: the padded power of two; otherwise 0 */
    uint32_t grid_x, grid_y, block;    /* first (or only) launch; all 0 for a refusal */
    uint32_t grid2_x, block2;          /* second launch (cosine finish, supcon_grad, the pair fallback's b copy); 0 if none */
    uint32_t reserved;
    int64_t lds_bytes, lds2_bytes;     /* dynamic LDS of the two launches */
} ocl_small_op_plan;
int ocl_test_small_op_path(int op, const int64_t* args, int n_args, ocl_small_op_plan* plan);
/* The sort of ocl_knn_sv (K10) replayed on the host, no GPU: n_cand (1 .. OCL_KNN_MAX_CAND) float keys are padded to the next
 * power of two as the kernel pads them and sent through the kernel's network -- the same compare-exchange function, comparator
 * and index arithmetic, one stage after the other -- and order_out receives the first n_cand indices.  For every input that is
 * torch.argsort(keys, stable=True) (tests/test_cpu_small_ops.py). */
int ocl_test_knn_order(const float* keys, int n_cand, int64_t* order_out);

/* Run-to-run reproducibility.  The BatchNorm batch sums (forward statistics, backward reductions) are the only accumulations of a
 * step whose order depends on scheduling.  on = 1: they are accumulated as fixed-point integers (associative): every weight is
 * bit-identical from run to run, as the reference's CPU path is at a fixed thread count; costs ~12 % per step (two atomics per
 * partial sum).  on = 0 (default; OCL_DETERMINISTIC=1 in the environment starts with 1): fp64 atomics.  Synchronises the device;
 * call it between steps, not inside one. */
int ocl_set_deterministic(int on);

/* ---- measurement helpers --------------------------------------------------------------------------
 * HIP-event timing on the caller's stream (bench.py's roofline leg: torch.cuda.Event only sees
 * torch's current stream).  Kernel-class accumulators are filled when profiling is enabled. */
int ocl_prof_enable(int on);
int ocl_prof_reset(void);
/* cls: 0 conv fwd/dgrad GEMM, 1 conv wgrad, 2 batchnorm/elementwise, 3 head/loss, 4 kNN/buffer.
 * Returns accumulated milliseconds and launch count since reset (synchronises the device). */
int ocl_prof_query(int cls, double* ms, int64_t* launches);
/* What the fp32 MFMA pipe of THIS box delivers right now: a register-only stream of v_mfma_f32_16x16x4_f32 (four independent
 * accumulators per wave, one wave per SIMD on every CU, `iters` rounds; no memory traffic), timed with HIP events on `stream`
 * (synchronises the host).  `scratch` receives 256 * n_cu floats (n_cu <= 1024).  bench.py reports it as `roofline.calibrated_peak`
 * next to the nominal peak so that a clock- or power-limited box shows in the record (boxes of this pool differ by up to ~19 % on the
 * MFMA-dense kernels).  There is no reference counterpart: measurement only. */
int ocl_mfma_calibrate(int iters, float* scratch, double* tflops, double* us, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OCL_HIP_H */
