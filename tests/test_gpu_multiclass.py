"""Twelve and sixteen classes end to end: the networks' OutConv and deep-supervision heads on the multi-class MFMA
kernels (csrc/outconv_mc.hip, routed by OutConvStage) and the confusion matrix up to 16 classes (csrc/metrics.hip),
against the CPU oracle in fp64 with the gates of test_gpu_parity.py's fp32 golden cases."""

import numpy as np
import pytest
import torch

from hip_helpers import grad_report, max_abs

pytestmark = pytest.mark.gpu
K = 12


def _o():
    from oracle import unet_oracle as O
    return O


@pytest.mark.parametrize("kind", ["attention_unet_ds", "unet"])
def test_network_twelve_classes_fp32_vs_oracle(kind):
    """One training step of the 12-class network in fp32 operand mode against the oracle run in fp64: logits and
    the three deep-supervision outputs within 1e-4, loss within 1e-5·(1 + |ref|), every parameter gradient within
    1e-3 of its tensor's largest entry.  Inputs: a net this small (2x3 bottleneck maps) has pre-activations and
    pooling windows within fp32 noise of a tie on some draws, and one flipped ReLU or max-pool choice moves a
    gradient tensor by percents: the oracle itself, fp32 against fp64 on the CPU, reaches 3.9e-2 (UNet) on generator
    seed 71, 7.8e-1 (AttentionUNet) on 73 and misses 1e-3 on 5 of the seeds 71..82.  Seed 76 is the draw on which
    the oracle is best conditioned: fp32 against fp64 1.6e-5 (AttentionUNet) and 6.6e-6 (UNet)."""
    from unet.models import AttentionUNet, UNet
    from unet.utils.loss import DeepSupervisionLoss, DiceBCELoss
    O = _o()
    torch.manual_seed(0)
    ds = kind != "unet"
    m = (AttentionUNet(n_channels=1, n_classes=K, bilinear=True, base_features=16, deep_supervision=True) if ds
         else UNet(n_channels=1, n_classes=K, bilinear=True, base_features=16))
    p = {k: (v.detach().double().requires_grad_(v.requires_grad) if v.is_floating_point() else v)
         for k, v in O.params_from_module(m).items()}
    gen = torch.Generator().manual_seed(76)
    x = torch.rand(2, 1, 40, 48, generator=gen) * 2 - 1
    t = torch.randint(0, K, (2, 40, 48), generator=gen)
    m = m.cuda().train()
    m.hip_precision = "fp32"
    out = m(x.cuda())
    loss = (DeepSupervisionLoss(DiceBCELoss()) if ds else DiceBCELoss())(out, t.cuda())
    loss.backward()
    ref = (O.attention_unet_forward(p, x.double(), training=True, deep_supervision=True) if ds
           else O.unet_forward(p, x.double(), training=True))
    ref_loss = O.deep_supervision_loss(ref, t, O.dice_bce_loss)
    ref_loss.backward()
    outs, refs = (out, ref) if ds else ([out], [ref])
    assert len(outs) == len(refs) == (4 if ds else 1)
    for o, r in zip(outs, refs):
        assert o.shape == (2, K, 40, 48) and max_abs(o, r) <= 1e-4, kind
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= 1e-5 * (1 + abs(float(ref_loss.detach())))
    e, k = grad_report(m, {k: v.grad for k, v in p.items() if v.is_floating_point() and v.requires_grad})
    assert e <= 1e-3, (kind, k, e)


@pytest.mark.parametrize("k", [12, 16])
def test_metrics_up_to_sixteen_classes(k):
    """SegmentationMetrics.update with and without ignore_index, compute_iou / compute_dice: exact counts against
    the oracle on the argmax labels, with a few targets outside [0, K)"""
    from unet.utils.metrics import SegmentationMetrics, compute_dice, compute_iou
    O = _o()
    gen = torch.Generator().manual_seed(72 + k)
    z = torch.randn(3, k, 37, 50, generator=gen)
    t = torch.randint(0, k, (3, 37, 50), generator=gen)
    t[0, :4] = 255
    t[2, 5, :7] = k
    t[1, 3, 5] = -1
    p = z.argmax(1)
    for ignore in (None, 3):
        m = SegmentationMetrics(num_classes=k, ignore_index=ignore)
        m.update(z.cuda(), t.cuda())
        keep = (t >= 0) & (t < k) & (t != (-2 if ignore is None else ignore))
        assert np.array_equal(m.get_confusion_matrix(), O.confusion_matrix(p[keep], t[keep], k).numpy())
    ri, rd = O.class_iou_dice(p, t, k)
    assert torch.equal(compute_iou(z.cuda(), t.cuda(), k).cpu(), ri)
    assert torch.equal(compute_dice(z.cuda(), t.cuda(), k).cpu(), rd)
