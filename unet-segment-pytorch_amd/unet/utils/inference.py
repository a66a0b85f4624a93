"""Inference path on the device (reference scripts/predict.py).

* `preprocess_images`: predict.py:100-135 (`preprocess_image`) for a batch — PIL BILINEAR resize of the
  8-bit slice to img_size, /255, (x - mean) / std — as byte kernels with Pillow's tables.
* `postprocess_masks`: predict.py:138-165 (`postprocess_mask`) — softmax over the classes,
  p[cls] > threshold -> 255 / 0, PIL NEAREST resize to the original size — one kernel, no host copy of
  the probabilities.
* `GraphedPredictor`: the eval-mode forward (BN with running statistics, applied inside the next conv's
  loader; no batch statistics, no backward state) captured once into a HIP graph and replayed per batch,
  so a batch-1 prediction costs one graph launch instead of ~150 kernel launches from Python.
* `predict_masks`: predict_single (predict.py:206-240) for a batch: preprocess -> graph replay ->
  postprocess, plus the tumour ratio (mask > 127).mean().
* `connected_components` / `filter_components`: per-class connected components of a label map and the usual
  clean-up (drop blobs below a minimum area, keep the largest per class) without the host round trip through
  scipy.ndimage.label (csrc/cc.hip); `postprocess_masks` and `predict_masks` take the same options.
"""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .._hip import lib as L
from .._hip.runtime import require_device, stream, vp
from .gpu_pipeline import _Tables, resize_bilinear_u8

_TABLES = {}


def _tables(device) -> _Tables:
    key = str(device)
    if key not in _TABLES:
        _TABLES[key] = _Tables(device)
    return _TABLES[key]


def preprocess_images(images: torch.Tensor, img_size: int = 256, mean: float = 0.5, std: float = 0.5,
                      device="cuda") -> torch.Tensor:
    """uint8 (N, h, w) -> fp32 (N, 1, img_size, img_size), as preprocess_image (predict.py:100-135)."""
    x = torch.as_tensor(images)
    if x.dim() == 2:
        x = x[None]
    if x.dtype != torch.uint8 or x.dim() != 3:
        raise RuntimeError(f"expected uint8 images (N, H, W), got {x.dtype} {tuple(x.shape)}")
    x = x.to(device, non_blocking=True).contiguous()
    require_device(x, "images")
    N = x.shape[0]
    r, _ = resize_bilinear_u8(x, img_size, img_size, _tables(x.device), roundtrip=False)
    out = torch.empty(N, 1, img_size, img_size, dtype=torch.float32, device=x.device)
    L.call("unet_slice_finish", N, img_size, img_size, vp(r), 0, 0, 0, None, None, None, None, float(mean),
           float(std), vp(out), None, stream())
    return out


def _cc_label(predictions: torch.Tensor, num_classes: int, connectivity: int, background: int):
    """Checks, then unet_cc_label: (outputs, whether the input was a uint8 mask, the workspace)."""
    K, conn, bg = int(num_classes), int(connectivity), int(background)
    if predictions.dim() not in (3, 4):
        raise ValueError("predictions must be logits (N, C, H, W), class indices (N, H, W) or a uint8 mask (N, H, W)")
    is_mask = predictions.dim() == 3 and predictions.dtype == torch.uint8
    N, H, W = predictions.shape[0], predictions.shape[-2], predictions.shape[-1]
    if not 1 <= K <= 16 or (is_mask and K != 2):
        raise ValueError(f"connected components serve 1 <= num_classes <= 16 and 2 classes for a uint8 mask, got {K}")
    if conn not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if not -1 <= bg < K:
        raise ValueError(f"background must lie in [-1, num_classes), got {background}")
    if not (1 <= H <= 4096 and 1 <= W <= 4096) or N < 1 or N * H * W >= 2 ** 31:
        raise ValueError(f"connected components serve 1 <= H, W <= 4096 and N * H * W < 2^31, got N = {N}, H = {H}, "
                         f"W = {W}")
    if predictions.dim() == 4 and predictions.shape[1] < 1:
        raise ValueError("logits need at least one channel")
    if not predictions.is_cuda:
        L.load(require_gpu=True)
        predictions = predictions.to(f"cuda:{torch.cuda.current_device()}")
    require_device(predictions, "predictions")
    dev = predictions.device
    C, logits, labels, mask = 1, None, None, None
    if predictions.dim() == 4:
        src = predictions.detach().float().contiguous()
        C, logits = src.shape[1], src.data_ptr()
    elif is_mask:
        src = predictions.detach().contiguous()
        mask = src.data_ptr()
    else:
        src = predictions.detach().to(torch.int64).contiguous()
        labels = src.data_ptr()
    ws = torch.empty(L.load().unet_cc_workspace(N, H, W), dtype=torch.uint8, device=dev)
    out = {"components": torch.empty(N, H, W, dtype=torch.int32, device=dev),
           "areas": torch.empty(N, H, W, dtype=torch.int32, device=dev),
           "classes": torch.empty(N, H, W, dtype=torch.uint8, device=dev),
           "count": torch.empty(N, K, dtype=torch.int64, device=dev)}
    L.call("unet_cc_label", N, C, K, H, W, logits, labels, mask, conn, bg, ws.data_ptr(), vp(out["components"]),
           vp(out["areas"]), vp(out["classes"]), vp(out["count"]), stream())
    return out, is_mask, ws


def connected_components(predictions: torch.Tensor, num_classes: int = 2, connectivity: int = 8,
                         background: int = 0):
    """Connected components per image and class, on the device (csrc/cc.hip).

    predictions: logits (N, C, H, W), argmax over dim 1 by the confusion matrix's rule (first maximum wins), class
    indices (N, H, W), or a uint8 mask (N, H, W) where a byte > 127 is class 1 and anything else class 0 (2 classes).
    1 <= num_classes <= 16, connectivity 4 or 8, background in [-1, num_classes) (-1: every class is labelled),
    1 <= H, W <= 4096 and N * H * W < 2^31 (ValueError otherwise).  A label outside [0, K) belongs to no class.  Host
    tensors are copied to the current GPU; nothing synchronises.  Returns device tensors:
      components int32 (N, H, W)  the smallest linear index y * W + x of the pixel's component, -1 for background
                                  and no-class pixels
      areas      int32 (N, H, W)  the component's pixel count at that smallest-index pixel, 0 elsewhere
      classes    uint8 (N, H, W)  the class, 255 for no class
      count      int64 (N, K)     components per image and class
    Every value is a function of the input alone: two calls give the same bits."""
    return _cc_label(predictions, num_classes, connectivity, background)[0]


def filter_components(predictions: torch.Tensor, num_classes: int = 2, min_size: int = 0, keep_largest: bool = False,
                      connectivity: int = 8, background: int = 0, fill: Optional[int] = None) -> torch.Tensor:
    """Drop the components (see `connected_components`) below `min_size` pixels and, with `keep_largest`, all but the
    largest of every (image, class), the one with the smaller id on a tie.  Returns int64 labels (N, H, W): kept
    components keep their class, background pixels the background class, everything else becomes `fill` (default:
    `background`, or 0 when background is -1).  A uint8 mask gives a uint8 mask: 255 on the kept components of class
    1, else 0."""
    out, is_mask, ws = _cc_label(predictions, num_classes, connectivity, background)
    comp = out["components"]
    N, H, W = comp.shape
    bg = int(background)
    fill = (bg if bg >= 0 else 0) if fill is None else int(fill)
    res = torch.empty(N, H, W, dtype=torch.uint8 if is_mask else torch.int64, device=comp.device)
    L.call("unet_cc_filter", N, int(num_classes), H, W, vp(comp), vp(out["areas"]), vp(out["classes"]),
           max(int(min_size), 0), int(bool(keep_largest)), bg, fill, ws.data_ptr(), None if is_mask else vp(res),
           vp(res) if is_mask else None, stream())
    return res


def postprocess_masks(logits: torch.Tensor, out_size: Optional[Tuple[int, int]] = None, threshold: float = 0.5,
                      cls: int = 1, min_size: int = 0, keep_largest: bool = False,
                      connectivity: int = 8) -> torch.Tensor:
    """uint8 (N, H', W') masks of 0 / 255; out_size = (W', H') as PIL's size (predict.py:142, 162).  With min_size >
    0 or keep_largest the mask at the output size goes through `filter_components`."""
    require_device(logits, "logits")
    z = logits.detach()
    if z.dtype != torch.float32 or not z.is_contiguous():
        z = z.float().contiguous()
    N, K, H, W = z.shape
    ow, oh = (W, H) if out_size is None else (int(out_size[0]), int(out_size[1]))
    t = _tables(z.device)
    out = torch.empty(N, oh, ow, dtype=torch.uint8, device=z.device)
    L.call("unet_postprocess_mask", N, K, H, W, vp(z), int(cls), float(threshold), oh, ow, vp(t.nearest(H, oh)),
           vp(t.nearest(W, ow)), vp(out), stream())
    if min_size > 0 or keep_largest:
        out = filter_components(out, 2, min_size, keep_largest, connectivity)
    return out


class GraphedPredictor:
    """model.eval() forward for a fixed input shape, captured into a HIP graph (torch.cuda.CUDAGraph
    drives hipGraph on ROCm).  Parameters and BN buffers are read at replay time, so weight updates
    (e.g. a reloaded checkpoint copied into the same tensors) are picked up without re-capturing."""

    def __init__(self, model: torch.nn.Module, input_shape: Sequence[int], device="cuda", warmup: int = 2):
        self.model = model.eval()
        self.x = torch.zeros(*input_shape, dtype=torch.float32, device=device)
        s = torch.cuda.Stream(device=device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.no_grad(), torch.cuda.stream(s):
            for _ in range(warmup):
                self.model(self.x)
        torch.cuda.current_stream(device).wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self.model(self.x)

    def __call__(self, x: torch.Tensor, copy: bool = True) -> torch.Tensor:
        """Logits of x.  copy=False returns the graph's static output buffer itself, which the next call
        overwrites (no extra 8-byte-per-logit copy); the default returns an independent tensor."""
        self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.out.clone() if copy else self.out


def predict_masks(model: torch.nn.Module, images: torch.Tensor, img_size: int = 256, threshold: float = 0.5,
                  predictor: Optional[GraphedPredictor] = None, min_size: int = 0, keep_largest: bool = False,
                  connectivity: int = 8):
    """predict_single (predict.py:206-240) for a batch of uint8 slices of one original size: returns
    (uint8 masks at the original size, tumour ratio per image).  min_size / keep_largest / connectivity filter the
    masks' components as in `postprocess_masks`; the ratio is that of the filtered mask."""
    x = torch.as_tensor(images)
    if x.dim() == 2:
        x = x[None]
    N, h, w = x.shape
    dev = next(model.parameters()).device
    inp = preprocess_images(x, img_size, device=dev)
    if predictor is not None:
        logits = predictor(inp)
    else:
        with torch.no_grad():
            logits = model.eval()(inp)
    masks = postprocess_masks(logits, (w, h), threshold, min_size=min_size, keep_largest=keep_largest,
                              connectivity=connectivity)
    ratio = (masks > 127).float().mean((1, 2))
    return masks, ratio
