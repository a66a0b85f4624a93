"""Segmentation losses with the reference's API (unet/utils/loss.py of seagochen/unet-segment-pytorch).

DiceLoss, BalancedCELoss and DiceBCELoss run as one fused HIP reduction + gradient pass
(`unet_loss_*` in include/unet_hip.h): the reference's per-image Python loop with boolean-mask
indexing (loss.py:134-145) becomes device-side per-image reductions, with no host sync.
CrossEntropyLoss (the factory's 'ce') and DiceCELoss ('dice_ce') serve 2 to 16 classes with per-class weights,
ignore_index and label smoothing through the `unet_ce_*` passes (csrc/loss_ce.hip).
"""

from typing import Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .._hip import lib as L
from .._hip.runtime import f32, require_device, stream, vp

_RED = {"mean": 0, "sum": 1, "none": 2}


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, t, ce_w, dice_w, class_w, ce_smooth, dice_smooth, ignore_bg, reduction):
        N, K, H, W = z.shape
        zc = z.detach()
        if zc.dtype != torch.float32 or not zc.is_contiguous():
            zc = zc.float().contiguous()
        tc = t if (t.dtype == torch.int64 and t.is_contiguous()) else t.long().contiguous()
        HW = H * W
        rows = L.load().unet_loss_rows(HW)
        part = f32(N, rows, 4 + 3 * K, device=z.device)
        L.call("unet_loss_reduce", N, K, HW, vp(zc), vp(tc), vp(part), stream())
        coef = f32(N, 2 + 2 * K, device=z.device)
        nd = K - (1 if (ignore_bg and K > 1) else 0)
        loss = f32(N, nd, device=z.device) if reduction == 2 else f32((), device=z.device)
        L.call("unet_loss_finalize", vp(part), rows, N, K, ce_w, dice_w, class_w, ce_smooth, dice_smooth,
               int(ignore_bg), reduction, vp(loss), vp(coef), stream())
        ctx.save_for_backward(zc, tc, coef)
        ctx.cfg = (reduction, int(ignore_bg))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        zc, tc, coef = ctx.saved_tensors
        reduction, ignore_bg = ctx.cfg
        N, K, H, W = zc.shape
        go = gout.float().contiguous()
        dz = torch.empty_like(zc)
        L.call("unet_loss_grad", N, K, H * W, vp(zc), vp(tc), vp(coef), vp(go), int(reduction == 2), ignore_bg,
               vp(dz), stream())
        return dz, None, None, None, None, None, None, None, None


class _FusedMultiLoss(torch.autograd.Function):
    """Σ_s w_s · base(z_s, t) over S same-shape logit sets in one reduce / finalize / grad launch each."""

    @staticmethod
    def forward(ctx, t, weights, cfg, *zs):
        ce_w, dice_w, class_w, ce_smooth, dice_smooth, ignore_bg = cfg
        S = len(zs)
        N, K, H, W = zs[0].shape
        zc = [z.detach() if (z.dtype == torch.float32 and z.is_contiguous()) else z.detach().float().contiguous()
              for z in zs]
        tc = t if (t.dtype == torch.int64 and t.is_contiguous()) else t.long().contiguous()
        HW = H * W
        rows = L.load().unet_loss_rows(HW)
        dev = zs[0].device
        part = f32(S, N, rows, 4 + 3 * K, device=dev)
        zp = (L.c_vp * S)(*[z.data_ptr() for z in zc])
        L.call("unet_loss_reduce_multi", S, N, K, HW, zp, vp(tc), vp(part), stream())
        coef = f32(S, N, 2 + 2 * K, device=dev)
        loss = f32((), device=dev)
        wts = (L.c_float * S)(*weights)
        L.call("unet_loss_finalize_multi", vp(part), rows, S, wts, N, K, ce_w, dice_w, class_w, ce_smooth, dice_smooth,
               int(ignore_bg), 0, vp(loss), vp(coef), stream())
        ctx.save_for_backward(tc, coef, *zc)
        ctx.ignore_bg = int(ignore_bg)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        tc, coef, *zc = ctx.saved_tensors
        S = len(zc)
        N, K, H, W = zc[0].shape
        go = gout.float().contiguous()
        dz = [torch.empty_like(z) for z in zc]
        zp = (L.c_vp * S)(*[z.data_ptr() for z in zc])
        dp = (L.c_vp * S)(*[d.data_ptr() for d in dz])
        L.call("unet_loss_grad_multi", S, N, K, H * W, zp, vp(tc), vp(coef), vp(go), 0, ctx.ignore_bg, dp, stream())
        return (None, None, None, *dz)


class _FusedCE(torch.autograd.Function):
    """Σ_s w_s · (ce_w · CE(z_s, t) + dice_w · Dice(z_s, t)) over S <= 4 same-shape logit sets: one reduce, one
    finalize and one grad launch (`unet_ce_*`, csrc/loss_ce.hip; the `_multi` entry points when S > 1).
    cfg = (ce_w, dice_w, ignore_index, label_smoothing, dice_smooth, ignore_bg, dice, reduction)."""

    @staticmethod
    def forward(ctx, t, weight, set_weights, cfg, *zs):
        ce_w, dice_w, ignore_index, eps, dice_smooth, ignore_bg, dice, reduction = cfg
        S = len(zs)
        N, K, H, W = zs[0].shape
        zc = [z.detach() if (z.dtype == torch.float32 and z.is_contiguous()) else z.detach().float().contiguous()
              for z in zs]
        tc = t if (t.dtype == torch.int64 and t.is_contiguous()) else t.long().contiguous()
        wc = None if weight is None else weight.detach().float().contiguous()
        HW, dev = H * W, zs[0].device
        rows = L.load().unet_loss_rows(HW)
        F = 4 + (3 * K if dice else 0)
        part = f32(S, N, rows, F, device=dev)
        coef = f32(S, 4 + (2 * N * K if dice else 0), device=dev)
        loss = f32((), device=dev) if reduction != 2 else None
        pmap = f32(N, H, W, device=dev) if reduction == 2 else None
        fin = (N, K, vp(wc), ce_w, dice_w, eps, dice_smooth, int(ignore_bg), int(dice), reduction, vp(loss), vp(coef),
               stream())
        if S == 1:
            L.call("unet_ce_reduce", N, K, HW, vp(zc[0]), vp(tc), vp(wc), ignore_index, eps, int(dice), vp(part),
                   vp(pmap), stream())
            L.call("unet_ce_finalize", vp(part), rows, *fin)
        else:
            zp = (L.c_vp * S)(*[z.data_ptr() for z in zc])
            L.call("unet_ce_reduce_multi", S, N, K, HW, zp, vp(tc), vp(wc), ignore_index, eps, int(dice), vp(part),
                   vp(pmap), stream())
            L.call("unet_ce_finalize_multi", vp(part), rows, S, (L.c_float * S)(*set_weights), *fin)
        ctx.save_for_backward(tc, coef, *([] if wc is None else [wc]), *zc)
        ctx.cfg = (wc is not None, ignore_index, int(dice), int(ignore_bg), reduction)
        return loss if reduction != 2 else pmap

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        has_w, ignore_index, dice, ignore_bg, reduction = ctx.cfg
        tc, coef, *rest = ctx.saved_tensors
        wc, zc = (rest[0], rest[1:]) if has_w else (None, rest)
        S = len(zc)
        N, K, H, W = zc[0].shape
        go = gout.float().contiguous()
        dz = [torch.empty_like(z) for z in zc]
        tail = (vp(coef), vp(go), int(reduction == 2), dice, ignore_bg)
        if S == 1:
            L.call("unet_ce_grad", N, K, H * W, vp(zc[0]), vp(tc), vp(wc), ignore_index, *tail, vp(dz[0]), stream())
        else:
            zp = (L.c_vp * S)(*[z.data_ptr() for z in zc])
            dp = (L.c_vp * S)(*[d.data_ptr() for d in dz])
            L.call("unet_ce_grad_multi", S, N, K, H * W, zp, vp(tc), vp(wc), ignore_index, *tail, dp, stream())
        return (None, None, None, None, *dz)


def _ce_hip_ok(z, t, weight) -> bool:
    """whether (logits, class-index targets, weight buffer) is a case of the HIP cross-entropy"""
    return (z.is_cuda and z.dim() == 4 and 2 <= z.shape[1] <= 16 and not t.is_floating_point()
            and t.device == z.device and t.shape == (z.shape[0], z.shape[2], z.shape[3])
            and (weight is None or (weight.device == z.device and weight.numel() == z.shape[1])))


def _fused(z, t, ce_w, dice_w, class_w, ce_smooth=1e-6, dice_smooth=1.0, ignore_bg=True, reduction="mean"):
    require_device(z, "predictions")
    if z.dim() != 4 or t.shape != (z.shape[0], z.shape[2], z.shape[3]):
        raise RuntimeError(f"expected predictions (N, C, H, W) and targets (N, H, W); got {tuple(z.shape)} and "
                           f"{tuple(t.shape)}")
    return _FusedLoss.apply(z, t, float(ce_w), float(dice_w), float(class_w), float(ce_smooth), float(dice_smooth),
                            bool(ignore_bg), _RED[reduction])


class DiceLoss(nn.Module):
    """1 - (2|P∩G| + s)/(|P| + |G| + s) on softmax probabilities — reference loss.py:18-85."""

    def __init__(self, smooth: float = 1.0, reduction: str = "mean", ignore_background: bool = True):
        super().__init__()
        self.smooth = smooth
        self.reduction = reduction
        self.ignore_background = ignore_background

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        return _fused(predictions, targets, 0.0, 1.0, 0.5, 1e-6, self.smooth, self.ignore_background, self.reduction)


class BalancedCELoss(nn.Module):
    """Per-image balanced cross entropy (tumour pixels share `class_weight`, background the rest) —
    reference loss.py:88-150."""

    def __init__(self, class_weight: float = 0.5, smooth: float = 1e-6):
        super().__init__()
        self.class_weight = class_weight
        self.smooth = smooth

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        return _fused(predictions, targets, 1.0, 0.0, self.class_weight, self.smooth, 1.0, True, "mean")


class DiceBCELoss(nn.Module):
    """ce_weight * BalancedCE + dice_weight * Dice — reference loss.py:153-191 (one fused pass)."""

    def __init__(self, ce_weight: float = 1.0, dice_weight: float = 1.0, class_weight: float = 0.5):
        super().__init__()
        self.ce_weight = ce_weight
        self.dice_weight = dice_weight
        self.balanced_ce = BalancedCELoss(class_weight=class_weight)
        self.dice_loss = DiceLoss(ignore_background=True)

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        return _fused(predictions, targets, self.ce_weight, self.dice_weight, self.balanced_ce.class_weight,
                      self.balanced_ce.smooth, self.dice_loss.smooth, self.dice_loss.ignore_background, "mean")


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """torch.nn.CrossEntropyLoss (same constructor, same `weight` buffer) whose (N, K, H, W) case with class-index
    targets (N, H, W), 2 <= K <= 16, on a ROCm device runs as one fused HIP reduction + gradient pass
    (csrc/loss_ce.hip).  There, a label outside [0, K) counts as ignored instead of raising a device assert.
    Every other input (CPU tensors, probability targets, other ranks, other K) goes to torch's own forward."""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not _ce_hip_ok(input, target, self.weight):
            return super().forward(input, target)
        L.load(require_gpu=True)
        cfg = (1.0, 0.0, int(self.ignore_index), float(self.label_smoothing), 1.0, False, False, _RED[self.reduction])
        return _FusedCE.apply(target, self.weight, [1.0], cfg, input)


class DiceCELoss(nn.Module):
    """ce_weight * weighted CE(mean) + dice_weight * Dice(mean) for 2 to 16 classes, one fused pass of both terms:
    the cross-entropy weights every class (`class_weights`), and both terms leave out the pixels labelled
    `ignore_index` or outside [0, K)."""

    def __init__(self, ce_weight: float = 1.0, dice_weight: float = 1.0, class_weights: Optional[list] = None,
                 ignore_index: int = -100, label_smoothing: float = 0.0, smooth: float = 1.0,
                 ignore_background: bool = True):
        super().__init__()
        self.ce_weight = ce_weight
        self.dice_weight = dice_weight
        self.register_buffer("weight", None if class_weights is None
                             else torch.as_tensor(class_weights, dtype=torch.float32))
        self.ignore_index = ignore_index
        self.label_smoothing = label_smoothing
        self.smooth = smooth
        self.ignore_background = ignore_background

    def _cfg(self):
        return (float(self.ce_weight), float(self.dice_weight), int(self.ignore_index), float(self.label_smoothing),
                float(self.smooth), bool(self.ignore_background), True, 0)

    def forward(self, predictions: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        require_device(predictions, "predictions")
        if not _ce_hip_ok(predictions, targets, self.weight):
            raise RuntimeError(f"DiceCELoss expects predictions (N, 2..16, H, W), class-index targets (N, H, W) and its "
                               f"weights on one device; got {tuple(predictions.shape)} and {tuple(targets.shape)}")
        return _FusedCE.apply(targets, self.weight, [1.0], self._cfg(), predictions)


class DeepSupervisionLoss(nn.Module):
    """Σ_k w_k · base(pred_k, targets) over [main, ds1, ds2, ds3] — reference loss.py:194-229.
    With one of the fused bases (DiceBCE / Dice(mean) / BalancedCE, or CrossEntropyLoss(mean | sum) / DiceCELoss)
    all the sets run through one launch of each loss pass; any other base criterion is applied per set as in the
    reference."""

    def __init__(self, base_criterion: nn.Module, weights: list = None):
        super().__init__()
        self.base_criterion = base_criterion
        self.weights = weights or [1.0, 0.4, 0.2, 0.1]

    def forward(self, predictions, targets: torch.Tensor) -> torch.Tensor:
        if isinstance(predictions, (list, tuple)):
            cfg = _fused_cfg(self.base_criterion)
            n = min(len(predictions), len(self.weights))
            same = 1 <= n <= 4 and all(p.dim() == 4 and p.shape == predictions[0].shape for p in predictions[:n])
            ce_cfg = _ce_cfg(self.base_criterion)
            if ce_cfg is not None and same and _ce_hip_ok(predictions[0], targets, self.base_criterion.weight):
                # likewise through unet_ce_*_multi
                L.load(require_gpu=True)
                return _FusedCE.apply(targets, self.base_criterion.weight, [float(w) for w in self.weights[:n]],
                                      ce_cfg, *predictions[:n])
            if cfg is not None and same:
                # the four logit sets through one reduce / finalize / grad launch (unet_loss_*_multi)
                require_device(predictions[0], "predictions")
                if targets.shape != (predictions[0].shape[0], predictions[0].shape[2], predictions[0].shape[3]):
                    raise RuntimeError(f"expected targets (N, H, W), got {tuple(targets.shape)}")
                return _FusedMultiLoss.apply(targets, [float(w) for w in self.weights[:n]], cfg,
                                             *predictions[:n])
            total = 0.0
            for pred, w in zip(predictions, self.weights):
                total = total + w * self.base_criterion(pred, targets)
            return total
        return self.base_criterion(predictions, targets)


def _fused_cfg(crit: nn.Module):
    """(ce_w, dice_w, class_w, ce_smooth, dice_smooth, ignore_bg) of a mean-reduced fused loss, else None."""
    if type(crit) is DiceBCELoss:
        return (float(crit.ce_weight), float(crit.dice_weight), float(crit.balanced_ce.class_weight),
                float(crit.balanced_ce.smooth), float(crit.dice_loss.smooth), bool(crit.dice_loss.ignore_background))
    if type(crit) is DiceLoss and crit.reduction == "mean":
        return (0.0, 1.0, 0.5, 1e-6, float(crit.smooth), bool(crit.ignore_background))
    if type(crit) is BalancedCELoss:
        return (1.0, 0.0, float(crit.class_weight), float(crit.smooth), 1.0, True)
    return None


def _ce_cfg(crit: nn.Module):
    """the _FusedCE configuration of a CrossEntropyLoss (mean or sum) or DiceCELoss base, else None"""
    if type(crit) is CrossEntropyLoss and crit.reduction in ("mean", "sum"):
        return (1.0, 0.0, int(crit.ignore_index), float(crit.label_smoothing), 1.0, False, False, _RED[crit.reduction])
    if type(crit) is DiceCELoss:
        return crit._cfg()
    return None


def create_loss_function(loss_type: str = "dice_bce", ce_weight: float = 1.0, dice_weight: float = 1.0,
                         class_weights: Optional[list] = None, balanced_class_weight: float = 0.5,
                         **kwargs) -> nn.Module:
    """Factory — reference loss.py:232-271 ('dice' | 'ce'/'crossentropy' | 'balanced_ce' | 'dice_bce'), and
    'dice_ce': DiceCELoss(ce_weight, dice_weight, class_weights)."""
    kind = loss_type.lower()
    if kind == "dice":
        return DiceLoss(ignore_background=True)
    if kind in ("ce", "crossentropy"):
        if class_weights is not None:
            return CrossEntropyLoss(weight=torch.tensor(class_weights, dtype=torch.float32))
        return CrossEntropyLoss()
    if kind == "dice_ce":
        return DiceCELoss(ce_weight=ce_weight, dice_weight=dice_weight, class_weights=class_weights)
    if kind == "balanced_ce":
        return BalancedCELoss(class_weight=balanced_class_weight)
    if kind == "dice_bce":
        return DiceBCELoss(ce_weight=ce_weight, dice_weight=dice_weight, class_weight=balanced_class_weight)
    raise ValueError(f"Unknown loss type: {loss_type}")
