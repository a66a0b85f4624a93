"""Segmentation metrics on the device (reference: unet/utils/metrics.py).

`SegmentationMetrics` keeps the reference's API (metrics.py:16-158): `update(predictions, targets)`
accumulates a K x K int64 confusion matrix, `compute()` returns pixel accuracy, per-class and mean
IoU / Dice with the same formulas (metrics.py:86-143, classes whose score is exactly 0 are left out of
the means, :131-135).  The difference is where the counting runs: the reference moves every batch to the
host and walks the pixels in a Python loop (metrics.py:78-84); here `update` is one HIP launch
(`unet_confusion_matrix`: argmax over the logits + LDS histogram + 64-bit atomics) that accumulates into
a device tensor without synchronising, and only `compute()` / `get_confusion_matrix()` read it back.
Counts are integers, so the matrix is bit-identical to the reference's.  The kernel's per-workgroup histogram
holds up to 16 classes (1 <= num_classes <= 16, the loss kernels' range); more are refused with an error.

`compute_iou` / `compute_dice` (metrics.py:160-231) are built on the same kernel.

`surface_distances` / `SurfaceDistanceMetrics` add the boundary metrics the reference does not have: Hausdorff
distance, its percentile (HD95) and the average symmetric surface distance per (image, class), computed on the
device by `unet_surface_distances` (csrc/surface.hip).
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .._hip import lib as L
from .._hip.runtime import require_device, stream

__all__ = ["SegmentationMetrics", "compute_iou", "compute_dice", "confusion_matrix", "surface_distances",
           "SurfaceDistanceMetrics"]


def confusion_matrix(predictions: torch.Tensor, targets: torch.Tensor, num_classes: int = 2,
                     ignore_index: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [K, K] device tensor, confusion[t, p] (+)= pixel counts (into `out` when given).

    predictions: logits (N, C, H, W) — argmax over dim 1 — or class indices (N, H, W).  Host tensors (what
    the reference's loop takes) are copied to the current GPU first; the counting always runs in HIP.

    Targets outside [0, K) (and `ignore_index`) are not counted, as in the reference's update()
    (metrics.py:76-84).  (compute_iou / compute_dice count every pixel instead: `_class_counts`.)"""
    if not predictions.is_cuda:
        predictions = predictions.to(f"cuda:{torch.cuda.current_device()}")
    if targets.device != predictions.device:
        targets = targets.to(predictions.device)
    require_device(predictions, "predictions")
    require_device(targets, "targets")
    K = int(num_classes)
    if out is None:
        out = torch.zeros(K, K, dtype=torch.int64, device=predictions.device)
    t = targets.to(torch.int64).contiguous()
    if predictions.dim() == 4:
        z = predictions.detach().float().contiguous()
        # argmax over however many channels the logits have; a class >= K is then skipped like the
        # reference's `0 <= p < num_classes` test (metrics.py:68-84)
        N, C, H, W = z.shape
        logits, labels = z.data_ptr(), None
    else:
        p = predictions.detach().to(torch.int64).contiguous()
        N = p.shape[0]
        C, H, W = 1, 1, p.numel() // max(N, 1)
        logits, labels = None, p.data_ptr()
    if t.numel() != N * H * W:
        raise ValueError(f"targets have {t.numel()} elements, predictions describe {N * H * W} pixels")
    L.call("unet_confusion_matrix", N, C, K, H * W, logits, labels, t.data_ptr(),
           int(ignore_index) if ignore_index is not None else 0, int(ignore_index is not None), out.data_ptr(),
           stream())
    return out


class SegmentationMetrics:
    """Accumulates a confusion matrix over batches and computes segmentation metrics
    (reference: metrics.py:16-158; same constructor, methods and result keys)."""

    def __init__(self, num_classes: int = 2, class_names: Optional[List[str]] = None,
                 ignore_index: Optional[int] = None):
        self.num_classes = num_classes
        self.class_names = class_names or [f'class_{i}' for i in range(num_classes)]
        self.ignore_index = ignore_index
        self._cm: Optional[torch.Tensor] = None   # device int64 accumulator

    @property
    def confusion_matrix(self) -> np.ndarray:
        """confusion[i, j] = pixels with true class i predicted as class j (host copy)."""
        if self._cm is None:
            return np.zeros((self.num_classes, self.num_classes), dtype=np.int64)
        return self._cm.cpu().numpy()

    def reset(self) -> None:
        """Reset accumulated statistics."""
        self._cm = None

    def update(self, predictions: torch.Tensor, targets: torch.Tensor) -> None:
        """Add a batch: logits (N, C, H, W) or class indices (N, H, W); targets (N, H, W).  Host tensors
        are accepted (copied to the current GPU)."""
        if not predictions.is_cuda:
            predictions = predictions.to(f"cuda:{torch.cuda.current_device()}")
        if self._cm is None:
            self._cm = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=predictions.device)
        elif self._cm.device != predictions.device:
            predictions = predictions.to(self._cm.device)
        confusion_matrix(predictions, targets, self.num_classes, self.ignore_index, out=self._cm)

    def compute(self) -> Dict[str, float]:
        """pixel_accuracy, mean_iou, mean_dice, class_iou, class_dice (metrics.py:86-143).

        All classes at once from the matrix: with tp = diag, |pred| = column sums and |true| = row sums,
        IoU = tp / (|pred| + |true| - tp) and Dice = 2 tp / (|pred| + |true|), 0 where the denominator
        is 0; the means run over the classes whose score is non-zero.  Integer counts divided in float64,
        as the reference's per-class scalar arithmetic does, so the values are identical."""
        cm = self.confusion_matrix
        names = self.class_names
        total = int(cm.sum())
        tp = np.diagonal(cm)
        both = cm.sum(0) + cm.sum(1)                 # |pred| + |true| per class
        union, dsum = both - tp, both
        iou = np.divide(tp, union, out=np.zeros(len(tp)), where=union > 0)
        dice = np.divide(2 * tp, dsum, out=np.zeros(len(tp)), where=dsum > 0)

        def nz_mean(v):
            v = v[v > 0]
            return float(np.mean(v)) if v.size else 0.0

        return {
            'pixel_accuracy': float(tp.sum() / total) if total else 0.0,
            'mean_iou': nz_mean(iou) if total else 0.0,
            'mean_dice': nz_mean(dice) if total else 0.0,
            'class_iou': dict(zip(names, map(float, iou))),
            'class_dice': dict(zip(names, map(float, dice))),
        }

    def get_confusion_matrix(self) -> np.ndarray:
        """Return the confusion matrix (host copy)."""
        return self.confusion_matrix.copy()


def _class_counts(predictions: torch.Tensor, targets: torch.Tensor, num_classes: int):
    """(|pred ∩ target|, |pred|, |target|) per class c < num_classes over EVERY pixel, as the reference's
    per-class masks count them (metrics.py:183-188, 217-221): one `unet_confusion_matrix_ext` launch
    into a (K+1) x (K+1) matrix whose last row / column holds targets / predictions outside [0, K)
    (e.g. an ignore label 255, or argmax classes >= K when the logits have C != K channels)."""
    if not predictions.is_cuda:
        predictions = predictions.to(f"cuda:{torch.cuda.current_device()}")
    if targets.device != predictions.device:
        targets = targets.to(predictions.device)
    require_device(predictions, "predictions")
    K = int(num_classes)
    t = targets.to(torch.int64).contiguous()
    if predictions.dim() == 4:
        z = predictions.detach().float().contiguous()
        N, C, H, W = z.shape
        logits, labels, P = z.data_ptr(), None, N * H * W
    else:
        p = predictions.detach().to(torch.int64).contiguous()
        N, C, P = p.shape[0], 0, p.numel()
        logits, labels = None, p.data_ptr()
    if t.numel() != P:
        raise ValueError(f"targets have {t.numel()} elements, predictions describe {P} pixels")
    cm = torch.zeros(K + 1, K + 1, dtype=torch.int64, device=predictions.device)
    L.call("unet_confusion_matrix_ext", N, C, K, P // max(N, 1), logits, labels, t.data_ptr(), cm.data_ptr(),
           stream())
    cm = cm.to(torch.float32)
    tp = torch.diagonal(cm)[:K]
    pred = cm.sum(0)[:K]     # pixels predicted as class c (any target)
    true = cm.sum(1)[:K]     # pixels labelled class c (any prediction)
    return tp, pred, true


def compute_iou(predictions: torch.Tensor, targets: torch.Tensor, num_classes: int = 2,
                smooth: float = 1e-6) -> torch.Tensor:
    """Per-class (I + s) / (U + s), U = |pred ∪ target| (metrics.py:160-193)."""
    tp, pred, true = _class_counts(predictions, targets, num_classes)
    return (tp + smooth) / ((pred + true - tp) + smooth)


def compute_dice(predictions: torch.Tensor, targets: torch.Tensor, num_classes: int = 2,
                 smooth: float = 1e-6) -> torch.Tensor:
    """Per-class (2I + s) / (|pred| + |target| + s) (metrics.py:196-231)."""
    tp, pred, true = _class_counts(predictions, targets, num_classes)
    return (2.0 * tp + smooth) / ((pred + true) + smooth)


def surface_distances(predictions: torch.Tensor, targets: torch.Tensor, num_classes: int = 2,
                      spacing: Sequence[float] = (1.0, 1.0), percentile: float = 95.0) -> Dict[str, torch.Tensor]:
    """Hausdorff distance, its percentile and the average symmetric surface distance per (image, class).

    predictions: logits (N, C, H, W), argmax over dim 1 by the confusion matrix's rule (first maximum wins), or class
    indices (N, H, W); targets (N, H, W).  1 <= num_classes <= 16 and 1 <= H, W <= 2048 (ValueError otherwise); a
    label outside [0, K) belongs to no class.  Host tensors are copied to the current GPU; nothing synchronises.

    For class c of image n, A = (P[n] == c) and B = (T[n] == c).  The surface S(A) is the set of pixels of A with at
    least one 4-neighbour not in A, pixels outside the frame counting as not in A: A ^ binary_erosion(A), the
    convention of medpy and MONAI.  With spacing (sy, sx), d(a, S(B)) = min over b in S(B) of
    sqrt(sy^2 (ya - yb)^2 + sx^2 (xa - xb)^2) for a in S(A), and the same the other way.  Returns device tensors
    [N, K]:
      hd             fp64, the larger of the two directed maxima
      hd_percentile  fp64, the larger of the two directed `percentile`-th percentiles (numpy.percentile's default
                     linear interpolation between ranks floor(q/100 (m-1)) and the next)
      assd           fp64, (sum_a d(a, S(B)) + sum_b d(b, S(A))) / (|S(A)| + |S(B)|)
      n_pred, n_true int64, the surface pixel counts |S(A)|, |S(B)|
    The three distances are NaN where either surface is empty.  With unit spacing every squared distance is an
    exact fp32 integer (2 * 2047^2 < 2^24: the reason for the 2048 limit); two calls give the same bits."""
    K = int(num_classes)
    if predictions.dim() not in (3, 4) or targets.dim() != 3:
        raise ValueError("predictions must be logits (N, C, H, W) or class indices (N, H, W), targets (N, H, W)")
    N, H, W = predictions.shape[0], predictions.shape[-2], predictions.shape[-1]
    if not 1 <= K <= 16:
        raise ValueError(f"surface_distances serves 1 <= num_classes <= 16, got {K}")
    if not (1 <= H <= 2048 and 1 <= W <= 2048) or N < 1 or N * K > 65535:
        raise ValueError(f"surface_distances serves 1 <= H, W <= 2048 and N * num_classes <= 65535, got "
                         f"N = {N}, H = {H}, W = {W}")
    if tuple(targets.shape) != (N, H, W):
        raise ValueError(f"targets are {tuple(targets.shape)}, predictions describe {(N, H, W)}")
    sy, sx = (float(v) for v in spacing)
    if not (0.0 < sy < math.inf and 0.0 < sx < math.inf):
        raise ValueError(f"spacing must be positive and finite, got {tuple(spacing)}")
    q = float(percentile)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentile must lie in [0, 100], got {percentile}")
    if not predictions.is_cuda:
        L.load(require_gpu=True)
        predictions = predictions.to(f"cuda:{torch.cuda.current_device()}")
    if targets.device != predictions.device:
        targets = targets.to(predictions.device)
    require_device(predictions, "predictions")
    dev = predictions.device
    t = targets.to(torch.int64).contiguous()
    if predictions.dim() == 4:
        z = predictions.detach().float().contiguous()
        C, logits, labels = z.shape[1], z.data_ptr(), None
    else:
        z = predictions.detach().to(torch.int64).contiguous()
        C, logits, labels = 1, None, z.data_ptr()
    ws = torch.empty(L.load().unet_surface_workspace(N, K, H, W), dtype=torch.uint8, device=dev)
    out = {k: torch.empty(N, K, dtype=torch.float64, device=dev) for k in ("hd", "hd_percentile", "assd")}
    out.update({k: torch.empty(N, K, dtype=torch.int64, device=dev) for k in ("n_pred", "n_true")})
    L.call("unet_surface_distances", N, C, K, H, W, logits, labels, t.data_ptr(), sy, sx, q / 100, ws.data_ptr(),
           out["hd"].data_ptr(), out["hd_percentile"].data_ptr(), out["assd"].data_ptr(), out["n_pred"].data_ptr(),
           out["n_true"].data_ptr(), stream())
    return out


class SurfaceDistanceMetrics:
    """Accumulates `surface_distances` over batches, in the shape of `SegmentationMetrics`.

    `update` adds, per class and on the device (no synchronisation), the sums of hd, hd_percentile and assd over the
    images where they are finite (both surfaces present) and the count of those images.  `compute()` returns
    `mean_hd`, `mean_hd<q>` (`mean_hd95` for the default percentile), `mean_assd` and the dicts `class_hd`,
    `class_hd<q>`, `class_assd` keyed by class name.  A class with no valid image is NaN in the dicts and left out of
    the means, as is class 0 unless `include_background`; NaN means when no class is left."""

    _KEYS = ("hd", "hd_percentile", "assd")

    def __init__(self, num_classes: int = 2, class_names: Optional[List[str]] = None,
                 spacing: Sequence[float] = (1.0, 1.0), percentile: float = 95.0, include_background: bool = False):
        self.num_classes = num_classes
        self.class_names = class_names or [f'class_{i}' for i in range(num_classes)]
        self.spacing = tuple(spacing)
        self.percentile = percentile
        self.include_background = include_background
        self._acc: Optional[torch.Tensor] = None   # device fp64 [4, K]: the three sums and the valid-image count

    def reset(self) -> None:
        """Reset accumulated statistics."""
        self._acc = None

    def update(self, predictions: torch.Tensor, targets: torch.Tensor) -> None:
        """Add a batch: logits (N, C, H, W) or class indices (N, H, W); targets (N, H, W)."""
        if self._acc is not None and predictions.is_cuda and predictions.device != self._acc.device:
            predictions = predictions.to(self._acc.device)
        r = surface_distances(predictions, targets, self.num_classes, self.spacing, self.percentile)
        ok = ~torch.isnan(r["hd"])
        rows = [torch.where(ok, r[k], torch.zeros_like(r[k])).sum(0) for k in self._KEYS]
        batch = torch.stack(rows + [ok.sum(0).to(torch.float64)])
        self._acc = batch if self._acc is None else self._acc + batch.to(self._acc.device)

    def compute(self) -> Dict[str, object]:
        """mean_hd, mean_hd<q>, mean_assd and the per-class dicts (host values; the one synchronising call)."""
        K, names = self.num_classes, self.class_names
        acc = np.zeros((4, K)) if self._acc is None else self._acc.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            per = acc[:3] / acc[3]                     # 0 / 0 = NaN: no valid image of the class
        first = 0 if self.include_background else 1
        tag = f"hd{float(self.percentile):g}"
        res: Dict[str, object] = {}
        for name, v in zip(("hd", tag, "assd"), per):
            kept = v[first:][~np.isnan(v[first:])]
            res[f"mean_{name}"] = float(kept.mean()) if kept.size else float("nan")
            res[f"class_{name}"] = dict(zip(names, map(float, v)))
        return res
