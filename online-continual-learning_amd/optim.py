"""torch.optim.SGD (momentum 0) and torch.optim.Adam, each as one HIP kernel over the flat parameter array (K8, K8b).

Replace `torch.optim.SGD.step` / `torch.optim.Adam.step` (utils/setup_elements.py:73-79; call sites agents/exp_replay.py:87,89,
agents/scr.py:60).  zero_grad() costs nothing: it only tells the engine that the next backward overwrites."""
import torch

from . import ops


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, model, lr, weight_decay=0.0):
        if not hasattr(model, "flat_params"):
            raise RuntimeError("FusedSGD needs an engine-backed model (ocl_amd.resnet)")
        self.model = model
        super().__init__(list(model.parameters()), dict(lr=lr, weight_decay=weight_decay))
        # parameters that take no part in forward() never get a gradient, and torch.optim.SGD skips a parameter whose grad is None
        # entirely -- weight decay included.  SupConResNet carries one such pair: the encoder's classifier (models/resnet.py:144,157-160)
        self._no_grad_names = [n for n, _ in model.named_parameters() if n.startswith("encoder.linear.")] if hasattr(model, "head_kind") else []

    def zero_grad(self, set_to_none=True):
        self.model.mark_grads_zero()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        g = self.param_groups[0]
        m = self.model
        if m._grads_fresh:
            return None  # no backward since zero_grad(): torch.optim.SGD skips parameters whose grad is None
        keep = None
        if g["weight_decay"] != 0 and self._no_grad_names:
            named = dict(m.named_parameters())
            keep = [(named[n], named[n].detach().clone()) for n in self._no_grad_names]
        ops.sgd_step(m.flat_params(), m.flat_grads(), g["lr"], g["weight_decay"], grad_scale)
        m.mark_weights_written()
        if keep is not None:      # undo the decay of the gradient-less tensors (two small device copies; weight_decay is 0 in every BASELINE config)
            for p, old in keep:
                p.data.copy_(old)
        return None


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad off) with its state as two flat arrays beside the flat parameters: one `adam_flat_kernel` launch per step."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        if not hasattr(model, "flat_params"):
            raise RuntimeError("FusedAdam needs an engine-backed model (ocl_amd.resnet)")
        self.model = model
        super().__init__(list(model.parameters()), dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self.step_count = 0
        self.exp_avg = self.exp_avg_sq = None   # allocated at the first counted step, on the parameters' device
        self._skip = None

    def add_param_group(self, param_group):
        if self.param_groups:   # (the constructor adds the one group through here)
            raise RuntimeError("FusedAdam steps the model's whole flat parameter array: one parameter group")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none=True):
        self.model.mark_grads_zero()

    def _skip_range(self):
        """Flat-array span of the parameters that take no part in forward() and therefore never get a gradient: torch.optim.Adam skips a
        parameter whose grad is None entirely -- no decay, no state.  SupConResNet carries one such pair, the encoder's classifier
        (models/resnet.py:144,157-160); weight and bias lie next to each other in the flat array (csrc/net.hip add_tensor: no padding)."""
        if self._skip is None:
            self._skip = (0, 0)
            if hasattr(self.model, "head_kind"):
                flat = self.model.flat_params()
                ps = [p for n, p in self.model.named_parameters() if n.startswith("encoder.linear.")]
                begin = min(p.storage_offset() for p in ps) - flat.storage_offset()
                end = max(p.storage_offset() + p.numel() for p in ps) - flat.storage_offset()
                if end - begin != sum(p.numel() for p in ps):
                    raise RuntimeError("FusedAdam: encoder.linear.* is not one contiguous span of the flat parameter array")
                self._skip = (begin, end)
        return self._skip

    def _ensure_state(self):
        flat = self.model.flat_params()
        if self.exp_avg is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        return flat

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        g = self.param_groups[0]
        m = self.model
        if m._grads_fresh:
            return None  # no backward since zero_grad(): torch.optim.Adam skips parameters whose grad is None, and counts no step for them
        if g["amsgrad"]:
            raise RuntimeError("FusedAdam: amsgrad is not implemented")
        flat = self._ensure_state()
        self.step_count += 1
        ops.adam_step(flat, m.flat_grads(), self.exp_avg, self.exp_avg_sq, self.step_count, g["lr"], g["betas"], g["eps"], g["weight_decay"],
                      grad_scale, self._skip_range())
        m.mark_weights_written()
        return None

    def state_dict(self):
        """The step count and the two flat moment arrays (None before the first counted step), beside the group's hyper-parameters."""
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        return dict(step=self.step_count, exp_avg=None if self.exp_avg is None else self.exp_avg.clone(),
                    exp_avg_sq=None if self.exp_avg_sq is None else self.exp_avg_sq.clone(), param_group=group)

    def load_state_dict(self, state_dict):
        n = sum(p.numel() for p in self.param_groups[0]["params"])
        for k in ("exp_avg", "exp_avg_sq"):
            t = state_dict[k]
            if t is not None and (t.dtype != torch.float32 or t.numel() != n):
                raise RuntimeError("FusedAdam.load_state_dict: %s must hold %d float32 values" % (k, n))
        self.step_count = int(state_dict["step"])
        if state_dict["exp_avg"] is None:
            self.exp_avg = self.exp_avg_sq = None
        else:
            dev = self.param_groups[0]["params"][0].device
            self.exp_avg = state_dict["exp_avg"].detach().reshape(-1).to(dev, copy=True)
            self.exp_avg_sq = state_dict["exp_avg_sq"].detach().reshape(-1).to(dev, copy=True)
        self.param_groups[0].update(state_dict.get("param_group", {}))
