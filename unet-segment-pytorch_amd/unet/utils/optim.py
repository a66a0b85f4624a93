"""Gradient-norm clip + AdamW as one fused device step (csrc/optim.hip).

`FusedClipAdamW` replaces the pair the reference's `train_one_epoch` runs after every backward
(scripts/train.py:140-142: `clip_grad_norm_(model.parameters(), clip)` and `torch.optim.AdamW.step()`) with at
most three launches over a device *segment table* (one row per parameter that has a gradient) and its *chunk map*:
`unet_optim_gradnorm` -> `unet_optim_prepare` -> `unet_optim_adamw`.  Nothing is read back to the host: the clip
coefficient, a GradScaler's unscale and its inf check, the step counts and the bias corrections are formed on the
device by the prepare launch.  There is no fallback: a gradient the kernels cannot take raises.
"""

from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .._hip import lib as L
from .._hip.runtime import require_device, stream, vp

CHUNK = L.OPTIM_CHUNK   # elements of a tensor one workgroup serves (UNET_OPTIM_CHUNK)


def build_chunk_map(numels: Sequence[int]) -> np.ndarray:
    """The chunk map of a segment table: int32 rows {segment, chunk index}; chunk c of a segment covers its elements
    [c * CHUNK, min((c + 1) * CHUNK, numel)), and a tensor shorter than a chunk (an empty one too) is one chunk."""
    rows = []
    for s, n in enumerate(numels):
        c = max(1, -(-int(n) // CHUNK))
        rows.append(np.stack([np.full(c, s, np.int32), np.arange(c, dtype=np.int32)], axis=1))
    return np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)


def upload(host: np.ndarray, dst: Optional[torch.Tensor], device) -> torch.Tensor:
    """Copy a host table into device memory (into `dst` when it has the size) on the current stream, without a
    device synchronise.  The bytes go through a pinned staging buffer allocated for this one copy: torch's host
    allocator hands a pinned block out again only after the copies recorded on it have finished, so building the
    next table can never overwrite one that is still in flight."""
    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    stage = torch.empty(raw.size, dtype=torch.uint8, pin_memory=True)
    stage.numpy()[:] = raw
    if dst is None or dst.numel() != raw.size or dst.device != torch.device(device):
        dst = torch.empty(raw.size, dtype=torch.uint8, device=device)
    dst.copy_(stage, non_blocking=True)
    return dst


def aligned16(*ptrs: int) -> bool:
    return all(p % 16 == 0 for p in ptrs)


class FusedClipAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay; amsgrad / maximize off) with `clip_grad_norm_(all parameters,
    max_grad_norm)` folded in (`max_grad_norm=None`: no clip).  The clip norm is global over every group.

    State per parameter is torch AdamW's capturable layout (`step`: a device fp32 scalar, `exp_avg`,
    `exp_avg_sq`), and the param_groups carry torch AdamW's keys, so a `torch.optim.AdamW` state_dict loads into
    this class and back.  Hyperparameters are read from `param_groups` at every step (schedulers work); an `lr`
    that is a device tensor is read on the device.

    `last_grad_norm`: the total norm `clip_grad_norm_` would have returned, a device scalar that the next step
    overwrites (None when neither a clip nor a GradScaler asked for the norm pass).

    GradScaler: `_step_supports_amp_scaling` is set, so `GradScaler.step` hands over `grad_scale` / `found_inf` as
    device tensors and does not read the inf flag on the host.  The unscale is folded into the clip coefficient; on
    an inf / NaN gradient (or `found_inf != 0`) parameters, moments and step counts stay bit-unchanged."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
        elif not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (None switches the clip off)")
        # torch.optim.AdamW's own group keys, so that state_dicts travel both ways
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=True, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._key = None          # pointers the uploaded table was built from
        self._group_key = None    # hyperparameters the uploaded group block holds
        self._segs = self._map = self._groups = self._partial = self._bc = self._result = None
        self._nsegs = self._nchunks = 0

    # table invalidation: both replace state tensors / groups wholesale
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._key = self._group_key = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._key = self._group_key = None

    def _name(self, p) -> str:
        for gi, group in enumerate(self.param_groups):
            for i, q in enumerate(group["params"]):
                if q is p:
                    names = group.get("param_names")
                    return f"'{names[i]}'" if names else f"parameter {i} of group {gi} (shape {tuple(p.shape)})"
        return "parameter"

    def _init_state(self, p, g):
        require_device(p, "parameter " + self._name(p))
        if g.dtype != torch.float32 or p.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() \
                or not p.is_contiguous() or g.is_sparse:
            raise RuntimeError(f"FusedClipAdamW: {self._name(p)} needs a contiguous fp32 parameter and gradient on "
                               f"one device (parameter {p.dtype} on {p.device}, gradient {g.dtype} on {g.device}, "
                               f"contiguous {p.is_contiguous()} / {g.is_contiguous()}); there is no fallback path")
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        step = st["step"]
        if not isinstance(step, torch.Tensor) or step.device != p.device or step.dtype != torch.float32:
            # a state_dict of a non-capturable torch AdamW keeps `step` on the host
            st["step"] = torch.as_tensor(float(step), dtype=torch.float32).to(p.device)
        for k in ("exp_avg", "exp_avg_sq"):
            if st[k].dtype != torch.float32 or st[k].device != p.device or not st[k].is_contiguous():
                raise RuntimeError(f"FusedClipAdamW: state '{k}' of {self._name(p)} is not a contiguous fp32 tensor "
                                   f"on {p.device}")
        return st

    def _scan(self):
        """The tensors of this step and the key (their addresses) the uploaded table is valid for."""
        items, key = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                st = self.state[p]
                items.append((gi, p, g, st))
                if st:
                    key.extend((gi, p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                st["step"].data_ptr(), g.dtype))
                else:
                    key.append(None)      # fresh parameter: forces a rebuild, which creates the state
        return items, key

    def _build(self, items):
        rows = np.zeros(len(items), dtype=np.dtype(L.OptimSeg))
        for i, (gi, p, g, _) in enumerate(items):
            st = self._init_state(p, g)
            ptrs = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
            rows[i] = (*ptrs, st["step"].data_ptr(), p.numel(), gi,
                       L.OPT_ADAMW | L.OPT_ACTIVE | (L.OPT_ALIGNED if aligned16(*ptrs) else 0))
        cmap = build_chunk_map([p.numel() for _, p, _, _ in items])
        dev = items[0][1].device
        if any(p.device != dev for _, p, _, _ in items):
            raise RuntimeError("FusedClipAdamW: all parameters must live on one device")
        self._segs = upload(rows, self._segs, dev)
        self._map = upload(cmap, self._map, dev)
        if self._nsegs != len(items) or self._nchunks != len(cmap) or self._result is None or self._result.device != dev:
            self._partial = torch.empty(len(cmap), dtype=torch.float64, device=dev)
            self._bc = torch.empty(len(items), 2, dtype=torch.float64, device=dev)
            self._result = torch.zeros(4, dtype=torch.float32, device=dev)
        self._nsegs, self._nchunks = len(items), len(cmap)
        return self._scan()[1]

    def _refresh_groups(self, dev):
        key, rows = [], np.zeros(len(self.param_groups), dtype=np.dtype(L.OptimGroup))
        for i, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or not group.get("decoupled_weight_decay", True):
                raise RuntimeError("FusedClipAdamW: amsgrad, maximize and coupled (L2) weight decay are not served")
            lr, (b1, b2) = group["lr"], group["betas"]
            lr_ptr = 0
            if isinstance(lr, torch.Tensor):
                if lr.is_cuda:
                    if lr.dtype != torch.float32 or lr.device != dev:
                        raise RuntimeError("FusedClipAdamW: a tensor lr must be an fp32 scalar on the parameters' device")
                    lr_ptr, lr = lr.data_ptr(), 0.0
                else:
                    lr = float(lr)
            rows[i] = (lr, b1, b2, group["eps"], group["weight_decay"], lr_ptr)
            key.append((lr, b1, b2, group["eps"], group["weight_decay"], lr_ptr))
        if key != self._group_key:
            self._groups = upload(rows, self._groups, dev)
            self._group_key = key

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items, key = self._scan()
        if not items:
            return loss
        if key != self._key:
            self._key = self._build(items)
        dev = items[0][1].device
        self._refresh_groups(dev)
        scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for name, t in (("grad_scale", scale), ("found_inf", found)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32
                                      and t.numel() == 1):
                raise RuntimeError(f"FusedClipAdamW: {name} must be a 1-element fp32 tensor on {dev} (as GradScaler.step "
                                   f"sets it), got {t!r}")
        s = stream()
        want_norm = self.max_grad_norm is not None or scale is not None
        if want_norm:
            L.call("unet_optim_gradnorm", vp(self._segs), vp(self._map), self._nchunks, vp(self._partial), s)
        L.call("unet_optim_prepare", vp(self._segs), self._nsegs, vp(self._groups), vp(self._partial),
               self._nchunks if want_norm else 0, float(self.max_grad_norm or 0.0), vp(scale), vp(found),
               vp(self._bc), vp(self._result), s)
        L.call("unet_optim_adamw", vp(self._segs), vp(self._map), self._nchunks, vp(self._groups), vp(self._bc),
               vp(self._result), s)
        self.last_grad_norm = self._result[0] if want_norm else None
        return loss
