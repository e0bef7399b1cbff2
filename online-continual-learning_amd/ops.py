"""Tensor-level wrappers over the C-ABI (one function per reference op sequence).

All inputs must live on the MI355X; outputs are allocated with torch (caller-owned memory is the
C-ABI's convention).  Nothing here computes on the CPU.
"""
import torch

from . import ffi


_data_streams = {}


def data_stream(device):
    """The stream of the data path (loader gather, buffer retrieve / update, concatenation, augmentation): none of it depends on
    the weights, so an agent can issue step i+1's data work next to step i's backward (agents/scr.py)."""
    key = torch.device(device).index
    if key not in _data_streams:
        _data_streams[key] = torch.cuda.Stream(device=device)
    return _data_streams[key]


def upload(t, device):
    """Asynchronous upload of a small CPU tensor (or numpy array) to `device` on the current stream.  A pageable-memory
    `.to(device)` blocks the host until the stream has drained, which serialises the host bookkeeping of step i+1 behind the GPU
    work of step i; `ocl_upload` stages the payload through the library's ring of pinned slots instead (one C call, no torch
    event / pinned-tensor objects: the index vectors of a replay step are 4 such uploads)."""
    if not torch.is_tensor(t):
        t = torch.from_numpy(t)
    if t.is_cuda:
        return t
    t = t.contiguous()
    d = torch.empty(t.shape, dtype=t.dtype, device=device)
    n = t.numel() * t.element_size()
    if n:
        if d.device.index != torch._C._cuda_getDevice():     # the staging ring and the stream belong to the current device
            with torch.cuda.device(d.device):
                return upload(t, device)
        ffi.init()
        ffi.check(ffi.lib().ocl_upload(ffi.vp(t.data_ptr()), n, ffi.vp(d.data_ptr()), ffi.stream()), "upload")
    return d


def _f32(t):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise RuntimeError("expected a float32 tensor on the GPU, got %s on %s" % (t.dtype, t.device))
    return t.contiguous()


def _i64(t):
    if t.dtype != torch.int64 or not t.is_cuda:
        raise RuntimeError("expected an int64 tensor on the GPU, got %s on %s" % (t.dtype, t.device))
    return t.contiguous()


# ---- K9 ----------------------------------------------------------------------------------------------
def gather_rows(src, idx, out=None):
    """src[idx] for a contiguous [R, ...] tensor (utils/buffer/buffer_utils.py:19-21)."""
    ffi.init()
    idx = _i64(idx)
    src = src.contiguous()
    n = idx.numel()
    row_bytes = src[0].numel() * src.element_size() if src.shape[0] > 0 else 0
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if n == 0:
        return out
    if row_bytes % 4 != 0:
        raise RuntimeError("gather_rows: row size must be a multiple of 4 bytes")
    ffi.check(ffi.lib().ocl_gather_rows(ffi.ptr(src), ffi.ptr(idx), n, row_bytes, ffi.ptr(out), ffi.stream()), "gather_rows")
    return out


def gather_pair(src_a, src_b, idx):
    """(src_a[idx], src_b[idx]) -- replay-buffer images and labels by one index vector -- as ONE call and one launch.  idx: an int64
    tensor on the host (the usual case: indices drawn by the numpy / torch-CPU generators; uploaded inside the call) or on the device."""
    ffi.init()
    n = idx.numel()
    dev = src_a.device
    out_a = torch.empty((n,) + tuple(src_a.shape[1:]), dtype=src_a.dtype, device=dev)
    out_b = torch.empty((n,) + tuple(src_b.shape[1:]), dtype=src_b.dtype, device=dev)
    if n == 0:
        return out_a, out_b
    if not (src_a.is_contiguous() and src_b.is_contiguous()):
        raise RuntimeError("gather_pair: sources must be contiguous")
    rb_a = src_a[0].numel() * src_a.element_size()
    rb_b = src_b[0].numel() * src_b.element_size()
    if idx.is_cuda:
        idx = _i64(idx)
        host_ptr, idx_dev = ffi.vp(0), idx
    else:
        idx = idx.contiguous()
        if idx.dtype != torch.int64:
            raise RuntimeError("gather_pair: int64 indices")
        host_ptr, idx_dev = ffi.vp(idx.data_ptr()), torch.empty(n, dtype=torch.int64, device=dev)
    if dev.index != torch._C._cuda_getDevice():
        with torch.cuda.device(dev):
            return gather_pair(src_a, src_b, idx)
    ffi.check(ffi.lib().ocl_gather_rows_pair(ffi.ptr(src_a), rb_a, ffi.ptr(out_a), ffi.ptr(src_b), rb_b, ffi.ptr(out_b), host_ptr,
                                             ffi.ptr(idx_dev), n, ffi.stream()), "gather_rows_pair")
    return out_a, out_b


def scatter_rows(dst, idx, src):
    """dst[idx] = src (utils/buffer/reservoir_update.py:59-60)."""
    ffi.init()
    idx = _i64(idx)
    n = idx.numel()
    if n == 0:
        return dst
    src = src.contiguous()
    if not dst.is_contiguous():
        raise RuntimeError("scatter_rows: destination must be contiguous")
    row_bytes = dst[0].numel() * dst.element_size()
    if src.numel() * src.element_size() != n * row_bytes:
        raise RuntimeError("scatter_rows: source/destination row size mismatch")
    ffi.check(ffi.lib().ocl_scatter_rows(ffi.ptr(dst), ffi.ptr(idx), n, row_bytes, ffi.ptr(src), ffi.stream()), "scatter_rows")
    return dst


def gather_u8_images(task_u8_nhwc, idx):
    """ToTensor() of task_u8_nhwc[idx]: uint8 [N,H,W,C] -> float32 [n,C,H,W] / 255."""
    ffi.init()
    idx = _i64(idx)
    n = idx.numel()
    _, h, w, c = task_u8_nhwc.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=task_u8_nhwc.device)
    if n:
        ffi.check(ffi.lib().ocl_gather_u8_hwc_to_f32_chw(ffi.ptr(task_u8_nhwc), ffi.ptr(idx), n, h, w, c, ffi.ptr(out),
                                                         ffi.stream()), "gather_u8")
    return out


def gather_f32_images(task_f32_nhwc, idx):
    """ToTensor() + .float() of task_f32_nhwc[idx] for a task that is float already (a new-instance stream): float32 [N,H,W,C] ->
    float32 [n,C,H,W], a transpose that keeps every bit.  The task may be a view whose rows are contiguous (a slice along N)."""
    ffi.init()
    idx = _i64(idx)
    n = idx.numel()
    if task_f32_nhwc.dtype != torch.float32 or not task_f32_nhwc.is_cuda or task_f32_nhwc.dim() != 4:
        raise RuntimeError("gather_f32_images: expected a float32 [N,H,W,C] tensor on the GPU, got %s %s on %s"
                           % (task_f32_nhwc.dtype, tuple(task_f32_nhwc.shape), task_f32_nhwc.device))
    _, h, w, c = task_f32_nhwc.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=task_f32_nhwc.device)
    if n:
        ffi.check(ffi.lib().ocl_gather_f32_hwc_to_f32_chw(ffi.ptr(task_f32_nhwc), ffi.ptr(idx), n, h, w, c, ffi.ptr(out),
                                                          ffi.stream()), "gather_f32")
    return out


# ---- K8, K8b-e: the flat-array kernels (csrc/flat_dev.h) ------------------------------------------------
def _flat_check(msg, first, *rest):
    """float32 arrays of one length on one GPU (a None among `rest` is skipped): returns the length, or raises RuntimeError(msg)."""
    n = first.numel()
    for t in (first,) + rest:
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_cuda or t.device != first.device):
            raise RuntimeError(msg)
    return n


def _flat_workspace(cache, doubles, msg, first, n, workspace):
    """The float64 workspace of one operation: the caller's, checked (RuntimeError(msg)), or the one of (device, n) in `cache`,
    allocated once with doubles(n) elements.  Every operation has a cache of its own: no two share a workspace."""
    if workspace is None:
        key = (first.device.index, n)
        workspace = cache.get(key)
        if workspace is None:
            workspace = cache[key] = torch.empty(doubles(n), dtype=torch.float64, device=first.device)
    elif workspace.dtype != torch.float64 or workspace.device != first.device:
        raise RuntimeError(msg)
    return workspace


# ---- K8 ----------------------------------------------------------------------------------------------
def sgd_step(params_flat, grads_flat, lr, weight_decay=0.0, grad_scale=1.0, out=None):
    ffi.init()
    ffi.check(ffi.lib().ocl_sgd_step(ffi.ptr(params_flat), ffi.ptr(grads_flat), params_flat.numel(), float(lr),
                                     float(weight_decay), float(grad_scale), ffi.ptr(out), ffi.stream()), "sgd_step")
    return out if out is not None else params_flat


# ---- K8b ---------------------------------------------------------------------------------------------
def adam_step(params_flat, grads_flat, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
              skip=(0, 0)):
    """One torch.optim.Adam step (amsgrad off) over the flat arrays, in place; `step` is this step's 1-based number, elements
    skip[0] .. skip[1] - 1 are left untouched."""
    ffi.init()
    n = _flat_check("adam_step: four float32 arrays of one length on one device", params_flat, grads_flat, exp_avg, exp_avg_sq)
    ffi.check(ffi.lib().ocl_adam_step(ffi.ptr(params_flat), ffi.ptr(grads_flat), ffi.ptr(exp_avg), ffi.ptr(exp_avg_sq), n,
                                      float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale),
                                      int(step), int(skip[0]), int(skip[1]), ffi.stream()), "adam_step")
    return params_flat


# ---- K8c ---------------------------------------------------------------------------------------------
_agem_workspaces = {}


def agem_project(g, g_ref_inout, workspace=None, info=None):
    """A-GEM's projection (agents/agem.py:72-80) in two launches: g_ref_inout <- g - (g.g_ref / g_ref.g_ref) * g_ref where g.g_ref < 0,
    else a copy of g; returns g_ref_inout.  workspace: a float64 tensor of ocl_agem_workspace_doubles(n) elements (default: one per
    (device, n), allocated once); info: a float32 tensor of 4 that receives prod, prod_ref, the coefficient and the decision."""
    ffi.init()
    n = _flat_check("agem_project: two float32 arrays of one length on one GPU", g, g_ref_inout)
    workspace = _flat_workspace(_agem_workspaces, ffi.lib().ocl_agem_workspace_doubles,
                                "agem_project: the workspace is a float64 tensor on the gradients' device", g, n, workspace)
    if info is not None and (info.dtype != torch.float32 or info.numel() < 4 or info.device != g.device):
        raise RuntimeError("agem_project: info is a float32 tensor of 4 on the gradients' device")
    ffi.check(ffi.lib().ocl_agem_project(ffi.ptr(g), ffi.ptr(g_ref_inout), n, ffi.ptr(workspace), workspace.numel(), ffi.ptr(info),
                                         ffi.stream()), "agem_project")
    return g_ref_inout


# ---- K8e ---------------------------------------------------------------------------------------------
_clip_workspaces = {}
_clip_infos = {}


def clip_grad_norm_(grads_flat, max_norm, workspace=None, info=None):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite off) on a flat gradient array, in two launches and in place:
    total = sqrt(sum g * g), g *= min(max_norm / (total + 1e-6), 1).  Returns the total norm as a one-element device tensor (a view of
    info[0]; no synchronisation), as torch's function does.  workspace: a float64 tensor of ocl_clip_workspace_doubles(n) elements
    (default: one per (device, n), allocated once); info: a float32 tensor of at least 4 that receives the total norm, the coefficient
    (1.0 when nothing was clipped), the decision and sum g * g (default: one per device, allocated once)."""
    ffi.init()
    n = _flat_check("clip_grad_norm_: a contiguous float32 array on the GPU", grads_flat)
    if not grads_flat.is_contiguous():
        raise RuntimeError("clip_grad_norm_: a contiguous float32 array on the GPU")
    dev = grads_flat.device
    workspace = _flat_workspace(_clip_workspaces, ffi.lib().ocl_clip_workspace_doubles,
                                "clip_grad_norm_: the workspace is a float64 tensor on the gradients' device", grads_flat, n, workspace)
    if info is None:
        info = _clip_infos.get(dev.index)
        if info is None:
            info = _clip_infos[dev.index] = torch.zeros(4, dtype=torch.float32, device=dev)
    elif info.dtype != torch.float32 or info.numel() < 4 or info.device != dev or not info.is_contiguous():
        raise RuntimeError("clip_grad_norm_: info is a float32 tensor of at least 4 on the gradients' device")
    ffi.check(ffi.lib().ocl_clip_grad_norm(ffi.ptr(grads_flat), n, float(max_norm), ffi.ptr(workspace), workspace.numel(), ffi.ptr(info),
                                           ffi.stream()), "clip_grad_norm")
    return info.reshape(-1)[0:1]


# ---- K8d ---------------------------------------------------------------------------------------------
_ewc_workspaces = {}


def _ewc_workspace(what, first, n, workspace):
    return _flat_workspace(_ewc_workspaces, ffi.lib().ocl_ewc_workspace_doubles,
                           "%s: the workspace is a float64 tensor on the arrays' device" % what, first, n, workspace)


def ewc_accumulate(grads_inout, tmp_fisher_inout, params, prev_params=None, fisher_hat=None, scale=0.0, workspace=None, penalty_out=None):
    """EWC++'s per-step bookkeeping (agents/ewc_pp.py:83-92, :104-106) in one launch: grads += scale * fisher_hat * (params - prev_params),
    tmp_fisher += grads ** 2; with prev_params and fisher_hat both None (first task) only the second.  penalty_out: a float32 tensor
    of 1 that receives sum fisher_hat * (params - prev_params) ** 2 (a second, one-block launch; the float64 workspace of
    ocl_ewc_workspace_doubles(n) elements is used only then -- default: one per (device, n), allocated once).  Returns grads_inout."""
    ffi.init()
    if (prev_params is None) != (fisher_hat is None):
        raise RuntimeError("ewc_accumulate: prev_params and fisher_hat are given together or not at all")
    n = _flat_check("ewc_accumulate: float32 arrays of one length on one GPU", grads_inout, tmp_fisher_inout, params, prev_params, fisher_hat)
    if penalty_out is not None:
        if penalty_out.dtype != torch.float32 or penalty_out.numel() < 1 or penalty_out.device != grads_inout.device:
            raise RuntimeError("ewc_accumulate: penalty_out is a float32 tensor of 1 on the arrays' device")
        workspace = _ewc_workspace("ewc_accumulate", grads_inout, n, workspace)
    elif workspace is not None and (workspace.dtype != torch.float64 or workspace.device != grads_inout.device):
        raise RuntimeError("ewc_accumulate: the workspace is a float64 tensor on the arrays' device")
    ffi.check(ffi.lib().ocl_ewc_accumulate(ffi.ptr(grads_inout), ffi.ptr(tmp_fisher_inout), ffi.ptr(params), ffi.ptr(prev_params),
                                           ffi.ptr(fisher_hat), n, float(scale), ffi.ptr(workspace),
                                           0 if workspace is None else workspace.numel(), ffi.ptr(penalty_out), ffi.stream()),
              "ewc_accumulate")
    return grads_inout


def ewc_fisher_ema(running_inout, tmp_inout, keep, gain):
    """running = keep * running + gain * tmp in float32 with separately rounded products (agents/ewc_pp.py:97-100), then tmp = 0 (:102)."""
    ffi.init()
    n = _flat_check("ewc_fisher_ema: float32 arrays of one length on one GPU", running_inout, tmp_inout)
    ffi.check(ffi.lib().ocl_ewc_fisher_ema(ffi.ptr(running_inout), ffi.ptr(tmp_inout), n, float(keep), float(gain), ffi.stream()),
              "ewc_fisher_ema")
    return running_inout


def ewc_fisher_normalize(running, fisher_hat_out, workspace=None, minmax_out=None):
    """fisher_hat_out = (running - min) / (max - min + 1e-32) over the whole array in IEEE float32 (agents/ewc_pp.py:76-80), two
    launches; minmax_out: a float32 tensor of 2 that receives min and max.  Returns fisher_hat_out."""
    ffi.init()
    n = _flat_check("ewc_fisher_normalize: float32 arrays of one length on one GPU", running, fisher_hat_out)
    workspace = _ewc_workspace("ewc_fisher_normalize", running, n, workspace)
    if minmax_out is not None and (minmax_out.dtype != torch.float32 or minmax_out.numel() < 2 or minmax_out.device != running.device):
        raise RuntimeError("ewc_fisher_normalize: minmax_out is a float32 tensor of 2 on the arrays' device")
    ffi.check(ffi.lib().ocl_ewc_fisher_normalize(ffi.ptr(running), ffi.ptr(fisher_hat_out), n, ffi.ptr(workspace), 2 * workspace.numel(),
                                                 ffi.ptr(minmax_out), ffi.stream()), "ewc_fisher_normalize")
    return fisher_hat_out


# ---- K6 ----------------------------------------------------------------------------------------------
def _refuse(op, what, t, dtype, shape):
    """The K6b-K6d functions convert nothing: anything but a contiguous tensor of this dtype and shape is refused."""
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous %s tensor of shape %s, got %s %s%s" % (
            op, what, dtype, tuple(shape), getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ())),
            "" if not torch.is_tensor(t) or t.is_contiguous() else " (not contiguous)"))


def cross_entropy(logits, y, reduction="mean", want_grad=True, dl_out=None):
    """(loss, dlogits): torch.nn.CrossEntropyLoss / F.cross_entropy(reduction='none').  dl_out: a contiguous float32 [n, c] tensor
    (e.g. a row block of a larger gradient buffer) that receives dlogits instead of a fresh one."""
    ffi.init()
    logits = _f32(logits)
    y = _i64(y)
    n, c = logits.shape
    red = {"none": 0, "mean": 1}[reduction]
    loss = torch.empty(n if red == 0 else 1, dtype=torch.float32, device=logits.device)
    if dl_out is not None:
        if dl_out.shape != logits.shape or dl_out.dtype != torch.float32 or not dl_out.is_contiguous() or dl_out.device != logits.device:
            raise RuntimeError("cross_entropy: dl_out must be a contiguous float32 %s tensor on %s" % (tuple(logits.shape), logits.device))
        dl = dl_out
    else:
        dl = torch.empty_like(logits) if want_grad else None
    ffi.check(ffi.lib().ocl_ce_fwd_bwd(ffi.ptr(logits), ffi.ptr(y), n, c, red, ffi.ptr(loss), ffi.ptr(dl), ffi.stream()), "ce")
    return (loss if red == 0 else loss[0]), dl


def cross_entropy_segmented(logits, y, seg, want_grad=True):
    """(mean loss, dlogits) of the softmax over each row's label segment; seg: int32 [c] on the device (agents/base.py:96-108)."""
    ffi.init()
    logits = _f32(logits)
    y = _i64(y)
    n, c = logits.shape
    if seg.dtype != torch.int32 or not seg.is_cuda or seg.numel() != c:
        raise RuntimeError("segment ids must be an int32 [%d] tensor on the GPU" % c)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    ffi.check(ffi.lib().ocl_ce_segmented_fwd_bwd(ffi.ptr(logits), ffi.ptr(y), ffi.ptr(seg.contiguous()), n, c, ffi.ptr(loss), ffi.ptr(dl),
                                                 ffi.stream()), "ce_segmented")
    return loss[0], dl


def kd_loss(scores, target_scores, T=2.0, want_grad=True):
    """(loss, dscores) of utils/kd_manager.py:6-11 (loss_fn_kd)."""
    ffi.init()
    scores, target_scores = _f32(scores), _f32(target_scores)
    if scores.shape != target_scores.shape or scores.dim() != 2:
        raise RuntimeError("kd_loss: scores %s vs target %s" % (tuple(scores.shape), tuple(target_scores.shape)))
    n, c = scores.shape
    loss = torch.empty(1, dtype=torch.float32, device=scores.device)
    ds = torch.empty_like(scores) if want_grad else None
    ffi.check(ffi.lib().ocl_kd_fwd_bwd(ffi.ptr(scores), ffi.ptr(target_scores), n, c, float(T), ffi.ptr(loss), ffi.ptr(ds), ffi.stream()), "kd")
    return loss[0], ds


# ---- K6b ---------------------------------------------------------------------------------------------
def ce_kd_blend(logits, y, teacher_logits, T, w_new, w_old, want_grad=True, dl_out=None):
    """(loss3, dlogits) of Learning without Forgetting's loss (agents/lwf.py:36-39) in one launch: loss3 = [w_new * ce + w_old * kd, ce, kd]
    with ce the mean cross-entropy of `logits` against `y` and kd loss_fn_kd(logits, teacher_logits, T); dlogits the gradient of
    loss3[0].  teacher_logits None (no teacher yet): kd = 0, the gradient is the cross-entropy's.  Nothing is made contiguous or
    converted here: a tensor of another dtype, shape, layout or device is refused.  dl_out: a contiguous float32 [n, c] tensor (e.g. a
    row block of a larger gradient buffer) that receives dlogits instead of a fresh one."""
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise RuntimeError("ce_kd_blend: logits must be a [n, c] tensor")
    _refuse("ce_kd_blend", "logits", logits, torch.float32, logits.shape)
    n, c = logits.shape
    _refuse("ce_kd_blend", "y", y, torch.int64, (n,))
    if teacher_logits is not None:
        _refuse("ce_kd_blend", "teacher_logits", teacher_logits, torch.float32, (n, c))
    if dl_out is not None:
        _refuse("ce_kd_blend", "dl_out", dl_out, torch.float32, (n, c))
    for what, t in (("logits", logits), ("y", y), ("teacher_logits", teacher_logits), ("dl_out", dl_out)):
        if t is not None and (not t.is_cuda or t.device != logits.device):
            raise RuntimeError("ce_kd_blend: %s is on %s; every tensor lives on the logits' GPU" % (what, t.device))
    ffi.init()
    loss = torch.empty(3, dtype=torch.float32, device=logits.device)
    dl = dl_out if dl_out is not None else (torch.empty_like(logits) if want_grad else None)
    ffi.check(ffi.lib().ocl_ce_kd_blend_fwd_bwd(ffi.ptr(logits), ffi.ptr(y), ffi.ptr(teacher_logits), n, c, float(T), float(w_new), float(w_old),
                                                ffi.ptr(loss), ffi.ptr(dl), ffi.stream()), "ce_kd_blend")
    return loss, dl


# ---- K6c ---------------------------------------------------------------------------------------------
def bce_distill(logits, teacher_logits, pos, n_stream, n_cls, n_old, want_grad=True, dl_out=None):
    """(loss3, dlogits) of iCaRL's loss (agents/icarl.py:42-62) in one launch: the binary cross-entropy of logits[:, :n_cls] against the
    target that is sigmoid(teacher_logits) on the columns below n_old and, on the columns from n_old to n_cls, the one-hot of `pos` for
    the first n_stream rows and zero for the others (the memory rows), summed over the columns and averaged over the rows.
    loss3 = [old + new, old, new] (the old and the new columns' parts); dlogits is the gradient of loss3[0], +0.0 in the columns from
    n_cls on.  pos: int64 [n_stream], the target column of each stream row.  teacher_logits None (no teacher yet) requires n_old == 0.
    Nothing is made contiguous or converted here: a tensor of another dtype, shape, layout or device is refused.  dl_out: a contiguous
    float32 [n, c] tensor (e.g. a row block of a larger gradient buffer) that receives dlogits instead of a fresh one."""
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise RuntimeError("bce_distill: logits must be a [n, c] tensor")
    _refuse("bce_distill", "logits", logits, torch.float32, logits.shape)
    n, c = logits.shape
    n_stream, n_cls, n_old = int(n_stream), int(n_cls), int(n_old)
    if not (1 <= n_stream <= n and 0 <= n_old <= n_cls <= c):
        raise RuntimeError("bce_distill: n_stream=%d n_cls=%d n_old=%d with logits %s (1 <= n_stream <= n, 0 <= n_old <= n_cls <= c)"
                           % (n_stream, n_cls, n_old, (n, c)))
    _refuse("bce_distill", "pos", pos, torch.int64, (n_stream,))
    if teacher_logits is not None:
        _refuse("bce_distill", "teacher_logits", teacher_logits, torch.float32, (n, c))
    elif n_old:
        raise RuntimeError("bce_distill: n_old=%d without teacher_logits" % n_old)
    if dl_out is not None:
        _refuse("bce_distill", "dl_out", dl_out, torch.float32, (n, c))
    for what, t in (("logits", logits), ("pos", pos), ("teacher_logits", teacher_logits), ("dl_out", dl_out)):
        if t is not None and (not t.is_cuda or t.device != logits.device):
            raise RuntimeError("bce_distill: %s is on %s; every tensor lives on the logits' GPU" % (what, t.device))
    ffi.init()
    loss = torch.empty(3, dtype=torch.float32, device=logits.device)
    dl = dl_out if dl_out is not None else (torch.empty_like(logits) if want_grad else None)
    ffi.check(ffi.lib().ocl_bce_distill_fwd_bwd(ffi.ptr(logits), ffi.ptr(teacher_logits), ffi.ptr(pos), n, n_stream, c, n_cls, n_old,
                                                ffi.ptr(loss), ffi.ptr(dl), ffi.stream()), "bce_distill")
    return loss, dl


# ---- K6e ---------------------------------------------------------------------------------------------
def der_loss(logits, y0, y2, stored, slots, n0, n1, n2, alpha, beta, want_grad=True, dl_out=None):
    """(loss4, dlogits) of Dark Experience Replay's loss (DER / DER++) in one launch.  `logits` [n0 + n1 + n2, c] is one block: the stream
    batch, the logit-replay batch, the label-replay batch.  loss4 = [ce + alpha * mse + beta * ce_m, ce, mse, ce_m] with ce the mean
    cross-entropy of the first n0 rows against `y0`, mse the mean squared error between the next n1 rows and stored[slots] (the logits
    those images had when they entered the memory; slots None: rows 0 .. n1 - 1 of `stored`), ce_m the mean cross-entropy of the last n2
    rows against `y2`; dlogits is the gradient of loss4[0].  n1 == 0 or n2 == 0 leaves the term out (0): `stored`, `slots`, `y2` may then
    be None.  stored: float32 [m, c], read in place; slots: int64 [n1].  Nothing is made contiguous or converted here: a tensor of another
    dtype, shape, layout or device is refused.  dl_out: a contiguous float32 [n0 + n1 + n2, c] tensor (e.g. a row block of a larger
    gradient buffer) that receives dlogits instead of a fresh one."""
    if not torch.is_tensor(logits) or logits.dim() != 2:
        raise RuntimeError("der_loss: logits must be a [n0 + n1 + n2, c] tensor")
    _refuse("der_loss", "logits", logits, torch.float32, logits.shape)
    n, c = logits.shape
    n0, n1, n2 = int(n0), int(n1), int(n2)
    if not (n0 >= 1 and n1 >= 0 and n2 >= 0 and n0 + n1 + n2 == n and c >= 1):
        raise RuntimeError("der_loss: n0=%d n1=%d n2=%d with logits %s (n0 >= 1, n1 >= 0, n2 >= 0, n0 + n1 + n2 rows, c >= 1)"
                           % (n0, n1, n2, (n, c)))
    _refuse("der_loss", "y0", y0, torch.int64, (n0,))
    if n2 or y2 is not None:
        _refuse("der_loss", "y2", y2, torch.int64, (n2,))
    m = 0
    if n1 or stored is not None:
        if not torch.is_tensor(stored) or stored.dim() != 2 or stored.shape[0] < 1:
            raise RuntimeError("der_loss: stored must be a [m, c] tensor with m >= 1")
        m = stored.shape[0]
        _refuse("der_loss", "stored", stored, torch.float32, (m, c))
    if slots is not None:
        _refuse("der_loss", "slots", slots, torch.int64, (n1,))
    elif n1 > m:
        raise RuntimeError("der_loss: n1=%d rows without slots, but stored has %d rows" % (n1, m))
    if dl_out is not None:
        _refuse("der_loss", "dl_out", dl_out, torch.float32, (n, c))
    for what, t in (("logits", logits), ("y0", y0), ("y2", y2), ("stored", stored), ("slots", slots), ("dl_out", dl_out)):
        if t is not None and (not t.is_cuda or t.device != logits.device):
            raise RuntimeError("der_loss: %s is on %s; every tensor lives on the logits' GPU" % (what, t.device))
    ffi.init()
    loss = torch.empty(4, dtype=torch.float32, device=logits.device)
    dl = dl_out if dl_out is not None else (torch.empty_like(logits) if want_grad else None)
    ffi.check(ffi.lib().ocl_der_fwd_bwd(ffi.ptr(logits), ffi.ptr(y0), ffi.ptr(y2) if n2 else None, ffi.ptr(stored) if n1 else None,
                                        ffi.ptr(slots) if n1 else None, n0, n1, n2, c, m, float(alpha), float(beta), ffi.ptr(loss), ffi.ptr(dl),
                                        ffi.stream()), "der_loss")
    return loss, dl


# ---- K6d ---------------------------------------------------------------------------------------------
def row_argmax_groupsum(x, col_group=None, sel=0, want_argmax=True, want_sum=True, argmax_out=None, sum_out=None):
    """(argmax int64 [n] | None, sums float64 [n] | None) of the rows of x [n, c] in one launch: the smallest column index among each row's
    maxima (a NaN is larger than everything and the first NaN wins, -0.0 equals +0.0: torch.max(x, 1) on the CPU), and the sum in double
    of the row's columns j with col_group[j] == sel (col_group int32 [c]; None sums every column; the other columns are not looked at,
    an empty group gives +0.0).  Nothing is made contiguous or converted here: a tensor of another dtype, shape, layout or device is
    refused.  argmax_out / sum_out: contiguous int64 / float64 [n] tensors (e.g. a row block of a loader-long table) that receive the
    results instead of fresh ones; giving one asks for that result."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise RuntimeError("row_argmax_groupsum: x must be a [n, c] tensor")
    _refuse("row_argmax_groupsum", "x", x, torch.float32, x.shape)
    n, c = x.shape
    if n < 1 or c < 1:
        raise RuntimeError("row_argmax_groupsum: x is %s (n and c must be >= 1)" % ((n, c),))
    want_argmax, want_sum = bool(want_argmax) or argmax_out is not None, bool(want_sum) or sum_out is not None
    if not (want_argmax or want_sum):
        raise RuntimeError("row_argmax_groupsum: neither the arg-max nor the sums are asked for")
    if col_group is not None:
        _refuse("row_argmax_groupsum", "col_group", col_group, torch.int32, (c,))
    if argmax_out is not None:
        _refuse("row_argmax_groupsum", "argmax_out", argmax_out, torch.int64, (n,))
    if sum_out is not None:
        _refuse("row_argmax_groupsum", "sum_out", sum_out, torch.float64, (n,))
    for what, t in (("x", x), ("col_group", col_group), ("argmax_out", argmax_out), ("sum_out", sum_out)):
        if t is not None and (not t.is_cuda or t.device != x.device):
            raise RuntimeError("row_argmax_groupsum: %s is on %s; every tensor lives on x's GPU" % (what, t.device))
    ffi.init()
    am = argmax_out if argmax_out is not None else (torch.empty(n, dtype=torch.int64, device=x.device) if want_argmax else None)
    sm = sum_out if sum_out is not None else (torch.empty(n, dtype=torch.float64, device=x.device) if want_sum else None)
    ffi.check(ffi.lib().ocl_row_argmax_groupsum(ffi.ptr(x), n, c, ffi.ptr(col_group), int(sel), ffi.ptr(am), ffi.ptr(sm), ffi.stream()),
              "row_argmax_groupsum")
    return am, sm


# ---- K7 ----------------------------------------------------------------------------------------------
def supcon(feat_view_major, y, n_views, temperature, want_grad=True):
    """(loss, dfeat) for view-major features [n_views*bsz, dim] (utils/loss.py:19-96)."""
    ffi.init()
    feat = _f32(feat_view_major)
    y = _i64(y)
    a, dim = feat.shape
    bsz = y.numel()
    if a != bsz * n_views:
        raise ValueError("Num of labels does not match num of features")
    ws = torch.empty(ffi.lib().ocl_supcon_workspace_bytes(a), dtype=torch.uint8, device=feat.device)
    loss = torch.empty(1, dtype=torch.float32, device=feat.device)
    df = torch.empty_like(feat) if want_grad else None
    ffi.check(ffi.lib().ocl_supcon_fwd_bwd(ffi.ptr(feat), ffi.ptr(y), bsz, n_views, dim, float(temperature), ffi.ptr(loss),
                                           ffi.ptr(df), ffi.ptr(ws), ffi.stream()), "supcon")
    return loss[0], df


# ---- K10 ---------------------------------------------------------------------------------------------
def knn_sv(eval_f, eval_y, cand_f, cand_y, k, want_order=False):
    """sv_matrix [n_eval, n_cand] (utils/buffer/aser_utils.py:7-61) from deep features."""
    ffi.init()
    eval_f, cand_f = _f32(eval_f), _f32(cand_f)
    eval_y, cand_y = _i64(eval_y), _i64(cand_y)
    ne, d = eval_f.shape
    nc = cand_f.shape[0]
    # (empty: the kernel's order is total, NaN distances included, so every cell is written for every input -- include/ocl_hip.h K10)
    sv = torch.empty((ne, nc), dtype=torch.float32, device=eval_f.device)
    order = torch.empty((ne, nc), dtype=torch.int64, device=eval_f.device) if want_order else None
    if ne and nc:
        ffi.check(ffi.lib().ocl_knn_sv(ffi.ptr(eval_f), ffi.ptr(eval_y), ne, ffi.ptr(cand_f), ffi.ptr(cand_y), nc, d, int(k),
                                       ffi.ptr(sv), ffi.ptr(order), ffi.stream()), "knn_sv")
    return (sv, order) if want_order else sv


def col_reduce(m, mode):
    ffi.init()
    m = _f32(m)
    r, c = m.shape
    out = torch.empty(c, dtype=torch.float32, device=m.device)
    ffi.check(ffi.lib().ocl_col_reduce(ffi.ptr(m), r, c, {"sum": 0, "mean": 1, "max": 2, "min": 3}[mode], ffi.ptr(out),
                                       ffi.stream()), "col_reduce")
    return out


def aser_score(sv_adv, sv_coop, aser_type):
    ffi.init()
    sv_adv = _f32(sv_adv)
    t = {"asvm": 0, "asv": 1, "neg_sv": 2}.get(aser_type, 0)  # "asvm or anything else" (aser_retrieve.py:80-82)
    n_adv, n_cand = sv_adv.shape
    out = torch.empty(n_cand, dtype=torch.float32, device=sv_adv.device)
    if t != 2:
        sv_coop = _f32(sv_coop)
        n_coop = sv_coop.shape[0]
    else:
        sv_coop, n_coop = None, 0
    ffi.check(ffi.lib().ocl_aser_score(ffi.ptr(sv_adv), n_adv, ffi.ptr(sv_coop), n_coop, n_cand, t, ffi.ptr(out), ffi.stream()),
              "aser_score")
    return out


def argsort_desc(v):
    ffi.init()
    v = _f32(v)
    out = torch.empty(v.numel(), dtype=torch.int64, device=v.device)
    ffi.check(ffi.lib().ocl_argsort_desc(ffi.ptr(v), v.numel(), ffi.ptr(out), ffi.stream()), "argsort_desc")
    return out


def cosine_max(mem_grads, grad, out=None, eps=1e-8):
    """max_i cosine_similarity(mem_grads[i], grad) (utils/buffer/buffer_utils.py:51-56, gss_greedy_update.py:79,121) -> [1]."""
    ffi.init()
    mem_grads, grad = _f32(mem_grads), _f32(grad)
    k, n = mem_grads.shape
    if grad.numel() != n:
        raise RuntimeError("cosine_max: %d-vector against rows of %d" % (grad.numel(), n))
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=grad.device)
    ws = torch.empty(ffi.lib().ocl_cosine_max_workspace_bytes(k), dtype=torch.uint8, device=grad.device)
    ffi.check(ffi.lib().ocl_cosine_max(ffi.ptr(mem_grads), k, n, ffi.ptr(grad), float(eps), ffi.ptr(out), ffi.ptr(ws), ffi.stream()),
              "cosine_max")
    return out


# ---- K11 ---------------------------------------------------------------------------------------------
def ncm_class_means(feat, labels, class_ids):
    ffi.init()
    feat, labels, class_ids = _f32(feat), _i64(labels), _i64(class_ids)
    n, d = feat.shape
    nc = class_ids.numel()
    means = torch.zeros((nc, d), dtype=torch.float32, device=feat.device)
    counts = torch.zeros(nc, dtype=torch.int32, device=feat.device)
    ffi.check(ffi.lib().ocl_ncm_class_means(ffi.ptr(feat), ffi.ptr(labels), n, d, ffi.ptr(class_ids), nc, ffi.ptr(means),
                                            ffi.ptr(counts), ffi.stream()), "ncm_class_means")
    return means, counts


def ncm_predict(feat, means):
    ffi.init()
    feat, means = _f32(feat), _f32(means)
    n, d = feat.shape
    pred = torch.empty(n, dtype=torch.int64, device=feat.device)
    ffi.check(ffi.lib().ocl_ncm_predict(ffi.ptr(feat), n, d, ffi.ptr(means), means.shape[0], ffi.ptr(pred), ffi.stream()),
              "ncm_predict")
    return pred


# ---- K12 ---------------------------------------------------------------------------------------------
def mir_scores(logits_pre, logits_post, y):
    ffi.init()
    a, b, y = _f32(logits_pre), _f32(logits_post), _i64(y)
    n, c = a.shape
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    ffi.check(ffi.lib().ocl_mir_scores(ffi.ptr(a), ffi.ptr(b), ffi.ptr(y), n, c, ffi.ptr(out), ffi.stream()), "mir_scores")
    return out


# ---- K13 ---------------------------------------------------------------------------------------------
AUG_NPARAM = 12
AUG_NUNIFORM = 30


def scr_augment(x, params):
    ffi.init()
    x, params = _f32(x), _f32(params)
    n, c, h, w = x.shape
    if c != 3 or params.shape != (n, AUG_NPARAM):
        raise RuntimeError("scr_augment: x must be [n,3,h,w] and params [n,%d]" % AUG_NPARAM)
    out = torch.empty_like(x)
    ffi.check(ffi.lib().ocl_scr_augment(ffi.ptr(x), ffi.ptr(out), n, h, w, ffi.ptr(params), ffi.stream()), "scr_augment")
    return out


def scr_augment_uniform(x, u, cfg12, want_params=False, out=None):
    """Augmented view from raw uniform draws u [n, AUG_NUNIFORM] (device): parameter arithmetic and the image kernel in one call.
    out: a contiguous [n,3,h,w] tensor (or row slice of one) to write into."""
    ffi.init()
    x, u = _f32(x), _f32(u)
    n, c, h, w = x.shape
    if c != 3 or u.shape != (n, AUG_NUNIFORM) or len(cfg12) != 12:
        raise RuntimeError("scr_augment_uniform: x must be [n,3,h,w], u [n,%d], cfg 12 floats" % AUG_NUNIFORM)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("scr_augment_uniform: out must be a contiguous float32 tensor of x's shape")
    params = torch.empty((n, AUG_NPARAM), dtype=torch.float32, device=x.device)
    cfg = (ffi.C.c_double * 12)(*[float(v) for v in cfg12])
    ffi.check(ffi.lib().ocl_scr_augment_uniform(ffi.ptr(x), ffi.ptr(out), n, h, w, ffi.ptr(u), cfg, ffi.ptr(params), ffi.stream()),
              "scr_augment_uniform")
    return (out, params) if want_params else out


def gemm_small(a, b, bias=None, relu=False, trans_b=False):
    """a[m,k] @ (b[k,n] or b[n,k]^T) — exposed for tests of the MFMA tile mapping."""
    ffi.init()
    a, b = _f32(a), _f32(b)
    m, k = a.shape
    n = b.shape[0] if trans_b else b.shape[1]
    c = torch.empty((m, n), dtype=torch.float32, device=a.device)
    b_rs, b_cs = (1, b.shape[1]) if trans_b else (b.shape[1], 1)
    ffi.check(ffi.lib().ocl_gemm_small(ffi.ptr(a), k, 1, ffi.ptr(b), b_rs, b_cs, ffi.ptr(c), n, m, n, k, ffi.ptr(bias),
                                       int(relu), 0, ffi.stream()), "gemm_small")
    return c


def prof_enable(on):
    ffi.check(ffi.lib().ocl_prof_enable(int(bool(on))), "prof_enable")


def prof_reset():
    ffi.check(ffi.lib().ocl_prof_reset(), "prof_reset")


def prof_query(cls):
    import ctypes as C
    ms = C.c_double(0)
    n = C.c_int64(0)
    ffi.check(ffi.lib().ocl_prof_query(int(cls), C.byref(ms), C.byref(n)), "prof_query")
    return ms.value, n.value


def mfma_calibrate(iters=20000):
    """(TFLOP/s, us) of a register-only v_mfma_f32_16x16x4_f32 stream on the current device, right now (measurement only:
    bench.py's `roofline.calibrated_peak`; blocks the host for ~iters * 60 ns)."""
    import ctypes as C
    ffi.init()
    scratch = torch.empty(256 * 1024, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    tf, us = C.c_double(0), C.c_double(0)
    ffi.check(ffi.lib().ocl_mfma_calibrate(int(iters), ffi.ptr(scratch), C.byref(tf), C.byref(us), ffi.stream()), "mfma_calibrate")
    return tf.value, us.value


def set_deterministic(on):
    """Order-independent (integer) BatchNorm batch sums: bit-reproducible training steps at ~12 % per step (include/ocl_hip.h)."""
    ffi.init()
    ffi.check(ffi.lib().ocl_set_deterministic(int(bool(on))), "set_deterministic")
