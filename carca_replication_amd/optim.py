"""The optimizer of the train driver as one launch per step.

The reference builds `torch.optim.Adam(model.parameters(), lr=..., betas=(0.9, 0.98), weight_decay=...)`
(scripts/training.py:174) and calls `.step()` once per batch (src/train.py:96).  torch's own Adam works unchanged on
the HIP-backed modules; this class is the same update (same state keys, interchangeable state_dict) issued through
carca_adam_step: every parameter of every group in ONE kernel launch, ~0.03 ms of host time instead of ~0.25 ms.

Beyond the reference: clipping by global gradient norm inside the step (max_grad_norm: two more
launches, carca_grad_norm), decoupled weight decay (AdamW), and global_grad_norm for logging.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Tuple

import torch

from . import _lib
from .ops import CarcaHipError, _stream


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) without amsgrad / maximize / capturable: fp32 CUDA
    parameters with dense gradients.  State per parameter: 'step' (CPU float tensor), 'exp_avg', 'exp_avg_sq'.

    max_grad_norm: clip by the global gradient norm inside the step.  step() takes the 2-norm over
    the gradients of ALL parameter groups -- torch.nn.utils.clip_grad_norm_(all params, max_grad_norm) -- and every group
    steps with g * min(1, max_grad_norm / (norm + 1e-6)).  Unlike torch's in-place clip, p.grad is left unscaled; the
    update has the bits of scaling first (the product is rounded once either way).  `last_grad_norm` is the device
    tensor holding the last step's norm before clipping (None without clipping or before the first step); reading it is
    the caller's synchronisation, step() adds none.  The value lives in param_groups (and so in the state dict); the
    groups must agree on it.  None: no clipping."""

    _decoupled = False  # AdamW below: p = p (1 - lr wd) instead of g = g + wd p
    last_grad_norm = None

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self.last_grad_norm = None
        self._steps = {}  # id(parameter) -> step count as a python int (state['step'] stays the tensor torch expects)
        self._marked = set()  # id(parameter) of the tables whose touched rows were announced for the coming step

    def mark_rows(self, param: torch.nn.Parameter, ids: torch.Tensor) -> bool:
        """Touched-row update of an embedding table: `ids` are the rows this step's gradient
        can be non-zero in.  The step then skips every row that has never been marked -- exactly the rows whose
        g = m = v = 0, for which dense Adam's update is exactly 0 -- so parameters and state keep the bits of the dense
        sweep without moving 7 floats per element of the whole table (1 M x 128: 2.5 GB per step).
        Must be called before EVERY step from the first one on; a step without it marks the whole table touched (dense
        from then on: still correct).  Refused (returns False) when weight decay would move untouched rows, or for a parameter of no group."""
        group = next((g for g in self.param_groups if any(q is param for q in g["params"])), None)
        if group is None:  # not this optimizer's parameter (frozen, or stepped by another optimizer): nothing to announce
            return False
        if group["weight_decay"] != 0 or param.dim() != 2:
            return False
        st = self.state[param]
        if "row_touched" not in st:
            started = bool(st) and float(st.get("step", 0.0)) > 0
            fill = torch.ones if started else torch.zeros  # (steps already taken densely: every row may carry state)
            st["row_touched"] = fill(param.shape[0], dtype=torch.uint8, device=param.device)
            self._fast = {}
        from . import ops

        ops.mark_rows(st["row_touched"], ids)
        self._marked.add(id(param))
        return True

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = {}
        self._fast = {}
        for st in self.state.values():  # (torch casts every state tensor to the parameter's dtype on load)
            if "row_touched" in st:
                st["row_touched"] = (st["row_touched"] != 0).to(torch.uint8)

    def state_dict(self):
        sd = super().state_dict()
        # The group's entries share ONE step tensor here; torch's format has one each.  The per-parameter dicts torch
        # hands back ARE this optimizer's own state dicts: build new ones -- writing the clone into them cut the live
        # state off the shared counter, and every later state_dict() (a checkpoint) reported the step count of the
        # first call (found by tools/two_rank_check.py: a resumed optimizer took its next step with a stale bias correction).
        sd["state"] = {k: (dict(st, step=st["step"].clone()) if "step" in st else st) for k, st in sd["state"].items()}
        return sd

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:  # (a state dict written by torch's optimizer has no such key)
            group.setdefault("max_grad_norm", self.defaults.get("max_grad_norm"))

    def _max_grad_norm(self):
        """The one clip threshold of the step: clipping is by the norm over ALL groups, so they must agree on it."""
        values = {g.get("max_grad_norm") for g in self.param_groups}
        if len(values) > 1:
            raise ValueError(f"carca Adam: max_grad_norm differs between parameter groups ({sorted(map(str, values))}); "
                             "the clip is by the global norm over all of them")
        value = values.pop() if values else None
        if value is not None and not value > 0:
            raise ValueError(f"Invalid max_grad_norm value: {value}")
        return value

    def _fast_group(self, fast, gi, group):
        """Steady state: every parameter has a gradient and state, all at the same step -> the cached table (p, m, v
        pointers and sizes are fixed) only needs this step's gradient pointers.  Returns the group's cache entry with its
        counters advanced, or None (the entry is dropped and the slow path rebuilds it)."""
        params = group["params"]
        c = fast.get(gi)
        if c is not None and c["n"] == len(params) and all(p.grad is not None for p in params) and \
                all(pp == p.data_ptr() for pp, p in zip(c["pp"], params)):
            arr = c["arr"]
            for i, p in enumerate(params):
                g = p.grad
                if not g.is_contiguous() or g.is_sparse:
                    c = None
                    break
                arr[i].g = g.data_ptr()
            if c is not None and c["masked"] and not all(i in self._marked for i in c["masked"]):
                c = None  # a masked table was not announced for this step: the slow path below turns it dense
            if c is not None:
                c["t"] += 1
                c["step"] += 1  # ONE CPU tensor shared by the group's state entries (37 separate ones cost 75 us)
                for p in params:
                    self._steps[id(p)] = c["t"]
                torch.autograd.graph.increment_version(params)
                return c
        fast.pop(gi, None)
        fast.pop("clip", None)
        return None

    def _slow_group(self, fast, gi, group, keep):
        """State set-up and the table of one group built from scratch: returns its launches [(table, n, step count)]."""
        params = group["params"]
        live = [p for p in params if p.grad is not None]
        if not live:
            return []
        steps = set()
        arr = (_lib.AdamTensor * len(live))()
        n_keep = len(keep)
        masked = []
        for i, p in enumerate(live):
            g = p.grad
            if g.is_sparse or p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise CarcaHipError("carca Adam: parameters must be contiguous fp32 CUDA tensors with dense gradients")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            st = self.state[p]
            if "step" not in st:  # (mark_rows may have put the row mask there already)
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            t = self._steps.get(id(p))
            if t is None:
                t = int(st["step"])
            self._steps[id(p)] = t + 1
            steps.add(t + 1)
            a = arr[i]
            a.p, a.g, a.m, a.v, a.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), \
                p.numel()
            if "row_touched" in st:
                if id(p) not in self._marked:  # an unannounced step: rows unknown -> every row counts as touched
                    st["row_touched"].fill_(1)
                a.row_mask, a.row_len = st["row_touched"].data_ptr(), p.shape[1]
                masked.append(id(p))
        # the kernel writes the parameters behind torch's back: bump their version counters, which is what the
        # modules' packed-weight caches (and autograd's saved-tensor checks) go by
        torch.autograd.graph.increment_version(live)
        if len(steps) == 1:
            t = steps.pop()
            shared = torch.tensor(float(t), dtype=torch.float32)
            for p in live:
                self.state[p]["step"] = shared
            if len(live) == len(params) and len(keep) == n_keep:
                fast[gi] = dict(arr=arr, n=len(params), t=t, pp=[p.data_ptr() for p in params], step=shared,
                                masked=masked)
            return [(arr, len(live), t)]
        # parameters that joined later carry their own step count: one launch per count
        for p in live:
            self.state[p]["step"] = torch.tensor(float(self._steps[id(p)]), dtype=torch.float32)
        launches = []
        for t in sorted(steps):
            idx = [i for i, p in enumerate(live) if self._steps[id(p)] == t]
            launches.append(((_lib.AdamTensor * len(idx))(*[arr[i] for i in idx]), len(idx), t))
        return launches

    def _clip_scale(self, lib, fast, plans, all_fast, max_norm) -> int:
        """The norm over the gradients of every launch of the step (two launches, no sync): returns the device address of
        the clip factor.  Steady state: ONE table holds every group's entries -- the groups' own tables are views into
        it, so the gradient pointers written for the step are already there -- and it is cached beside `partials` and the
        two floats of `out` until the fast path is rebuilt."""
        c = fast.get("clip") if all_fast else None
        if c is None:
            total = sum(n for _, launches in plans for _, n, _ in launches)
            big = (_lib.AdamTensor * total)()
            k = 0
            for _, launches in plans:
                for arr, n, _ in launches:
                    for i in range(n):
                        big[k] = arr[i]
                        k += 1
            chunks = sum((big[i].n + 1023) // 1024 for i in range(total))
            device = plans[0][0]["params"][0].device
            out = torch.empty(2, dtype=torch.float32, device=device)
            c = dict(arr=big, n=total, chunks=chunks, out=out, norm=out[0], scale_ptr=out.data_ptr() + 4,
                     partials=torch.empty(max(chunks, 1), dtype=torch.float32, device=device))
            if all(gi in fast for gi in range(len(self.param_groups))):  # every group is in its steady state from here on
                k = 0
                for gi in range(len(self.param_groups)):
                    n = fast[gi]["n"]
                    fast[gi]["arr"] = (_lib.AdamTensor * n).from_buffer(big, k * C.sizeof(_lib.AdamTensor))
                    k += n
                fast["clip"] = c
        _lib.check(lib.carca_grad_norm(c["arr"], c["n"], float(max_norm), c["partials"].data_ptr(), c["chunks"],
                                       c["out"].data_ptr(), _stream()), "grad_norm")
        self.last_grad_norm = c["norm"]
        return c["scale_ptr"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        fast = self.__dict__.setdefault("_fast", {})
        max_norm = self._max_grad_norm()
        plans = []  # (group, [(table, entries, step count)]) of every group with a gradient
        keep = []  # contiguous copies of gradients: alive until the launches are out
        all_fast = True
        for gi, group in enumerate(self.param_groups):
            c = self._fast_group(fast, gi, group)
            if c is not None:
                plans.append((group, [(c["arr"], c["n"], c["t"])]))
                continue
            all_fast = False
            launches = self._slow_group(fast, gi, group, keep)
            if launches:
                plans.append((group, launches))
        scale = None
        if max_norm is not None and plans:  # ONE norm over all groups, ahead of the first update (clip_grad_norm_(all))
            scale = self._clip_scale(lib, fast, plans, all_fast, max_norm)
        stream = _stream()
        for group, launches in plans:
            b1, b2 = group["betas"]
            for arr, n, t in launches:
                _lib.check(lib.carca_adam_step_ex(arr, n, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                                  float(group["weight_decay"]), t, int(self._decoupled), scale, stream),
                           "adam_step")
        self._marked.clear()
        return loss


class AdamW(Adam):
    """torch.optim.AdamW(params, lr, betas, eps, weight_decay) through the same launch: the decay is decoupled,
    p = p (1 - lr wd) and then Adam's update on the undecayed gradient.  Same state keys; the state dict is interchangeable
    with torch.optim.AdamW's.  mark_rows refuses a table under weight decay as Adam's does."""

    _decoupled = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)


def global_grad_norm(params) -> torch.Tensor:
    """The 2-norm of the gradients of `params` taken as one vector (what torch.nn.utils.clip_grad_norm_ returns), by the
    two launches of carca_grad_norm: a device scalar, no synchronisation.  Parameters without a gradient are skipped."""
    if isinstance(params, torch.Tensor):
        params = [params]
    grads = []
    for p in params:
        g = p.grad
        if g is None:
            continue
        if g.is_sparse or g.dtype != torch.float32 or not g.is_cuda:
            raise CarcaHipError("global_grad_norm: gradients must be dense fp32 CUDA tensors")
        grads.append(g if g.is_contiguous() else g.contiguous())
    if not grads:
        return torch.tensor(0.0)
    if any(g.device != grads[0].device for g in grads):
        raise CarcaHipError("global_grad_norm: gradients on more than one device")
    arr = (_lib.AdamTensor * len(grads))()
    for a, g in zip(arr, grads):
        a.g, a.n = g.data_ptr(), g.numel()
    chunks = sum((g.numel() + 1023) // 1024 for g in grads)
    partials = torch.empty(max(chunks, 1), dtype=torch.float32, device=grads[0].device)
    out = torch.empty(2, dtype=torch.float32, device=grads[0].device)
    with torch.cuda.device(grads[0].device):
        _lib.check(_lib.load().carca_grad_norm(arr, len(grads), 1.0, partials.data_ptr(), chunks, out.data_ptr(), _stream()),
                   "grad_norm")
    return out[0]
