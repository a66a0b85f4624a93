"""Hot-path utilities (reference: unet/utils/__init__.py): the losses and the segmentation metrics
(confusion matrix counted on the device), the fused clip + AdamW step and ModelEMA (the tail of the
training step).  The reference's host-side callbacks/plots/dataset are out of scope."""

from .loss import (DiceLoss, BalancedCELoss, DiceBCELoss, CrossEntropyLoss, DiceCELoss, DeepSupervisionLoss,
                   create_loss_function)
from .metrics import (SegmentationMetrics, compute_dice, compute_iou, surface_distances,
                      SurfaceDistanceMetrics)
from .config import load_config, create_model, create_criterion, build_from_config, create_train_transform
from .optim import FusedClipAdamW
from .general import ModelEMA
from .inference import connected_components, filter_components

__all__ = ["FusedClipAdamW", "ModelEMA","DiceLoss", "BalancedCELoss", "DiceBCELoss", "CrossEntropyLoss", "DiceCELoss", "DeepSupervisionLoss", "create_loss_function",
           "SegmentationMetrics", "compute_iou", "compute_dice", "surface_distances", "SurfaceDistanceMetrics", "load_config", "create_model", "create_criterion",
           "build_from_config", "create_train_transform", "connected_components", "filter_components"]
