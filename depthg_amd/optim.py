"""The optimisation step's Adams as one HIP launch (src/train_segmentation.py:447-455, 537-547: three torch.optim.Adam - the head's,
the cluster probe's, the linear probe's - stepped one after the other over nine small tensors).

    FusedAdam       a torch.optim.Optimizer with torch.optim.Adam's default algorithm (weight_decay = 0, amsgrad = False,
                    maximize = False) and its state layout - {"step", "exp_avg", "exp_avg_sq"} per parameter, created on the first
                    step that sees a gradient - so that a state_dict written by torch.optim.Adam (the reference's Lightning
                    checkpoints) loads into it and back.  step() is ONE ops.adam_step call (dg_adam_step) over all its parameters.
    FusedAdamSet    several FusedAdam stepped together: ONE ops.adam_step call for all members' parameters; the members keep
                    their own param_groups and state (state_dict / load_state_dict per member, as with the three torch Adams).

Step count: a group with `capturable` false keeps `step` on the CPU and the bias corrections are formed on the host (as torch
does); with `capturable` true `step` lives on the parameter's device, the kernel reads and advances it, and a step recorded into a
hipGraph (torch.cuda.graph) advances at every replay - nothing the host computed at capture time is baked in.  `load_state_dict` is
the base class's: it restores the SAVED groups, their `capturable` included; set `group["capturable"] = True` afterwards (the
torch idiom) to replay a loaded optimiser from a graph - the step tensors follow at the next step.

There is no eager path: parameters on the CPU are refused at step()."""
from typing import Iterable, List, Optional, Sequence

import torch

from . import ops


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdam: `lr` must be a Python number (a tensor lr is not implemented)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        # the keys of torch.optim.Adam's groups, so that either class reads the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=capturable, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_group(group)
        self._tickets = None

    @torch.no_grad()
    def step(self, closure=None, grads: Optional[Sequence[Optional[torch.Tensor]]] = None):
        """One launch over this optimiser's parameters.  grads: optional sequence aligned with the parameters (group by group),
        read instead of p.grad; an entry None skips that parameter, as p.grad = None does."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._tickets = _step_all([self], grads, self._tickets)
        return loss


class FusedAdamSet:
    """FusedAdam optimisers stepped in ONE ops.adam_step call (the members' own hyper-parameters and state)."""

    def __init__(self, optimisers: Iterable[FusedAdam]):
        self.optimisers: List[FusedAdam] = list(optimisers)
        for o in self.optimisers:
            if not isinstance(o, FusedAdam):
                raise TypeError(f"FusedAdamSet: members must be FusedAdam (got {type(o).__name__})")
        self._tickets = None

    def parameters(self) -> List[torch.Tensor]:
        """The stepped parameters in the order `step(grads=...)` expects their gradients."""
        return [p for o in self.optimisers for g in o.param_groups for p in g["params"]]

    def zero_grad(self, set_to_none: bool = True):
        for o in self.optimisers:
            o.zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self, grads: Optional[Sequence[Optional[torch.Tensor]]] = None):
        self._tickets = _step_all(self.optimisers, grads, self._tickets)


_REFUSED = (("weight_decay", 0), ("amsgrad", False), ("maximize", False), ("differentiable", False), ("decoupled_weight_decay", False))


def _check_group(group):
    for key, want in _REFUSED:
        if group.get(key, want) != want:
            raise ValueError(f"FusedAdam: `{key}={group[key]}` is not implemented by the kernel (torch.optim.Adam's default "
                             f"algorithm only: {key}={want})")
    if isinstance(group["lr"], torch.Tensor):
        raise ValueError("FusedAdam: `lr` must be a Python number (a tensor lr is not implemented)")
    for p in group["params"]:
        if p.dtype != torch.float32:
            raise ValueError(f"FusedAdam: parameters must be float32 (got {p.dtype}, shape {tuple(p.shape)})")
        if p.is_sparse or not p.is_contiguous():
            raise ValueError(f"FusedAdam: parameters must be dense and contiguous (shape {tuple(p.shape)}, strides {p.stride()})")


def _step_all(optimisers, grads, tickets):
    """The segment table of every parameter of `optimisers` that has a gradient, host-mode and device-mode groups apart, and one
    ops.adam_step per non-empty table (one in all when the groups agree on `capturable`).  Returns the ticket words."""
    host, dev, groups = [], [], []
    k = 0
    for o in optimisers:
        for group in o.param_groups:
            _check_group(group)
            capturable = bool(group["capturable"])
            gi = len(groups)
            groups.append((group["lr"], group["betas"][0], group["betas"][1], group["eps"]))
            for p in group["params"]:
                g = grads[k] if grads is not None else p.grad
                k += 1
                if not p.is_cuda:
                    raise RuntimeError(f"depthg_amd: FusedAdam parameters must live on the GPU (got {p.device}); there is no CPU path")
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("FusedAdam does not support sparse gradients")
                if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != p.numel():
                    raise RuntimeError(f"FusedAdam: gradients must be contiguous float32 tensors of the parameter's size (got {g.dtype}, "
                                       f"{tuple(g.shape)}, strides {g.stride()} for a parameter of shape {tuple(p.shape)})")
                state = o.state[p]
                if len(state) == 0:          # as torch.optim.Adam._init_group: lazily, zero-filled
                    state["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable else torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = state["step"]
                if capturable:
                    if not step.is_cuda:     # (a state loaded from a host-mode checkpoint, `capturable` set afterwards)
                        step = state["step"] = step.to(device=p.device, dtype=torch.float32)
                    dev.append((p, g, state["exp_avg"], state["exp_avg_sq"], step, gi))
                else:
                    if step.is_cuda:
                        step = state["step"] = step.cpu()
                    step += 1
                    host.append((p, g, state["exp_avg"], state["exp_avg_sq"], step.item(), gi))
    if grads is not None and k != len(grads):
        raise ValueError(f"FusedAdam: {len(grads)} gradients for {k} parameters")
    if host:
        ops.adam_step(host, groups, device_steps=False)
    if dev:
        d = dev[0][0].device
        if tickets is None or tickets.numel() < len(dev) or tickets.device != d:
            tickets = torch.zeros(max(len(dev), 16), dtype=torch.int32, device=d)
        ops.adam_step(dev, groups, device_steps=True, tickets=tickets)
    return tickets
