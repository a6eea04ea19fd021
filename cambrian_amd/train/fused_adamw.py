"""AdamW with global gradient-norm clipping on the project's own kernels (csrc/optim.hip): one norm launch over all
gradients, one update launch per parameter group, no host synchronisation.

The reference clips: ``train_fsdp.py:122`` derives ``TrainingArguments`` from ``transformers.TrainingArguments``, no recipe
under ``scripts/cambrian`` passes ``--max_grad_norm`` and ``cambrian_trainer.py`` keeps the stock training loop, so every
released recipe runs with Hugging Face's default ``max_grad_norm = 1.0``: a global L2 clip before each optimizer step.
``FusedAdamW(..., max_grad_norm=1.0)`` is that algorithm.  It holds what ``MasterAdamW`` (master.py) holds — fp32 masters of
bf16 parameters, fp32 moments — and replaces its three passes (up-cast of the gradients, torch's AdamW on the masters, cast
back) and a caller's ``clip_grad_norm_`` (norm, host read, scale pass) by ``cmb_grad_sqnorm`` + ``cmb_adamw_step``: the clip
coefficient is formed on the device from the norm and folded into the gradient as it is read.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import ops


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW``'s update rule (decoupled weight decay) with an optional global L2 clip of the gradients.

    * ``params_or_groups``: parameters, or parameter groups with their own ``lr`` / ``weight_decay`` / ``betas`` / ``eps``
      (the reference builds decay / no-decay and per-module-lr groups, cambrian_trainer.py:255-365).  ``param_groups`` are
      real, so ``torch.optim.lr_scheduler.*`` and HF ``get_scheduler`` attach.  A bf16 parameter is stepped on an fp32
      master (``self.masters``, in a group in place of the parameter) and refreshed from it in the same pass; an fp32
      parameter is stepped in place.  Parameters live on a ROCm device and are contiguous.
    * State per stepped tensor: ``step``, ``exp_avg``, ``exp_avg_sq``; ``state_dict()`` adds the ``masters`` list — the
      layout of ``MasterAdamW.state_dict()``: a checkpoint written by either class loads into the other (one group, the
      same parameters in the same order).  The step counts are kept on the host.
    * ``max_grad_norm``: the threshold of ``torch.nn.utils.clip_grad_norm_`` over the gradients of ALL groups, or None.
      ``last_grad_norm`` is then the norm before clipping, an fp32 device scalar that whoever logs it reads when they need
      it; ``step()`` itself never waits for the device.  Under replicated data parallelism the gradients after
      ``GradSync.finish()`` are the same on every rank, so the norm is local and no collective is added.
    * Non-finite gradients: no step is skipped.  The coefficient is what ``min(1, max_norm / (norm + 1e-6))`` gives: a NaN
      norm fails the comparison, the coefficient is 1 and the NaN gradients reach their parameters; an infinite norm gives
      0, the infinite gradients become NaN (0 * inf) and the finite ones 0.  ``last_grad_norm`` reports the non-finite
      value, which is the caller's signal to act on.
    * ``grad_scale``: a factor every gradient still carries the inverse of (1 / world for gradients that are sums over
      ranks); the norm and the update see ``grad_scale * g``.
    * Not supported, ``ValueError``: ``amsgrad``, ``maximize``, ``capturable``, a closure, CPU parameters.
    """

    def __init__(self, params_or_groups, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, master_dtype: torch.dtype = torch.float32, amsgrad: bool = False,
                 maximize: bool = False, capturable: bool = False, grad_scale: float = 1.0):
        if amsgrad or maximize or capturable:
            raise ValueError("FusedAdamW: amsgrad / maximize / capturable are not implemented by cmb_adamw_step")
        if master_dtype != torch.float32:
            raise ValueError("FusedAdamW: the kernel steps fp32 masters only")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be positive or None, got {max_grad_norm}")
        # torch.optim.AdamW's own defaults (and its validation of lr / betas / eps / weight_decay), so that a state_dict of
        # this class carries every key torch's AdamW expects of a loaded group; `fused` as MasterAdamW sets it on a GPU
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        defaults["fused"] = True
        groups = list(params_or_groups)
        if not groups:
            raise ValueError("FusedAdamW: got an empty parameter list")
        if not isinstance(groups[0], dict):
            groups = [{"params": groups}]
        self.low: List[torch.nn.Parameter] = []
        self.full: List[torch.nn.Parameter] = []
        self.masters: List[torch.nn.Parameter] = []
        self._low_of: Dict[int, torch.nn.Parameter] = {}   # id(master) -> the bf16 parameter it is the master of
        built = []
        for g in groups:
            g = dict(g)
            _reject_modes(g)
            ps = g["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            ps = [p for p in ps if p.requires_grad]
            for p in ps:
                if not p.is_cuda:
                    raise ValueError("FusedAdamW: parameters must live on a ROCm device (the update is a HIP kernel; "
                                     "MasterAdamW steps CPU parameters)")
                if p.dtype not in (torch.float32, torch.bfloat16) or not p.is_contiguous():
                    raise ValueError(f"FusedAdamW: contiguous fp32 / bf16 parameters only, got {p.dtype} "
                                     f"{'' if p.is_contiguous() else '(not contiguous)'}")
            low = [p for p in ps if p.dtype != master_dtype]
            full = [p for p in ps if p.dtype == master_dtype]
            masters = [torch.nn.Parameter(p.detach().to(master_dtype), requires_grad=True) for p in low]
            for m, p in zip(masters, low):
                self._low_of[id(m)] = p
            self.low += low
            self.full += full
            self.masters += masters
            g["params"] = masters + full
            built.append(g)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_scale = float(grad_scale)
        self.last_grad_norm: Optional[torch.Tensor] = None
        super().__init__(built, defaults)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("FusedAdamW.step() takes no closure: evaluate the loss before calling it")
        work = []        # per group: [(stepped tensor, gradient, bf16 copy or None)]
        for group in self.param_groups:
            _reject_modes(group)
            live = []
            for t in group["params"]:
                low = self._low_of.get(id(t))
                g = (t if low is None else low).grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise ValueError("FusedAdamW does not take sparse gradients")
                live.append((t, g if g.is_contiguous() else g.contiguous(), None if low is None else low.data))
            work.append(live)
        grads = [g for live in work for _, g, _ in live]
        sumsq = None
        if self.max_grad_norm is not None and grads:
            sumsq = ops.grad_sqnorm(grads)
            self.last_grad_norm = sumsq.sqrt() * self.grad_scale if self.grad_scale != 1.0 else sumsq.sqrt()
        for group, live in zip(self.param_groups, work):
            by_step: Dict[int, list] = {}   # one launch per step count (they differ only after a parameter sat steps out)
            for t, g, low in live:
                st = self.state[t]
                if not st:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(t, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(t, memory_format=torch.contiguous_format)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append((t, g, low, st))
            beta1, beta2 = group["betas"]
            for k, items in by_step.items():
                ops.adamw_step([g for _, g, _, _ in items], [t.data for t, _, _, _ in items],
                               [st["exp_avg"] for *_, st in items], [st["exp_avg_sq"] for *_, st in items],
                               [low for _, _, low, _ in items], lr=float(group["lr"]), beta1=float(beta1), beta2=float(beta2),
                               eps=float(group["eps"]), weight_decay=float(group["weight_decay"]), step=k,
                               grad_scale=self.grad_scale, sumsq=sumsq,
                               max_norm=self.max_grad_norm if sumsq is not None else 0.0)
        return None

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.low + self.full:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()
        for m in self.masters:
            m.grad = None

    def state_bytes(self) -> int:
        """master copies + two moments per stepped element"""
        return (sum(m.numel() * m.element_size() * 3 for m in self.masters)
                + sum(p.numel() * p.element_size() * 2 for p in self.full))

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["masters"] = [m.detach().clone() for m in self.masters]
        return sd

    def load_state_dict(self, sd: dict) -> None:
        sd = dict(sd)
        masters = sd.pop("masters")
        if "inner" in sd:   # a round-5 MasterAdamW checkpoint
            sd = sd["inner"]
        if len(masters) != len(self.masters) or any(t.shape != m.shape for t, m in zip(masters, self.masters)):
            raise ValueError(f"FusedAdamW: the checkpoint holds {len(masters)} masters, this optimizer {len(self.masters)} "
                             "(or their shapes differ): other parameters, or another order")
        super().load_state_dict(sd)
        for group in self.param_groups:
            _reject_modes(group)
        for st in self.state.values():   # the step counts stay on the host (a fused torch AdamW keeps them on the device)
            if "step" in st:
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).detach().cpu().reshape(())
        with torch.no_grad():
            for m, t, p in zip(self.masters, masters, self.low):
                m.copy_(t)
                p.copy_(m)

    def resync_masters(self) -> None:
        """Masters := the parameters as they are now (weights loaded into the module after the optimizer was built)."""
        with torch.no_grad():
            for m, p in zip(self.masters, self.low):
                m.copy_(p)


def _reject_modes(group: dict) -> None:
    for key in ("amsgrad", "maximize", "capturable"):
        if group.get(key):
            raise ValueError(f"FusedAdamW: {key} is not implemented by cmb_adamw_step")
