"""CPU: the argument checks of unet.utils.metrics.surface_distances run before anything touches the device, and
host tensors on a machine without a GPU meet the package's usual error (there is no CPU path)."""

import pytest
import torch


def _labels(n=1, h=8, w=8):
    return torch.zeros(n, h, w, dtype=torch.int64)


@pytest.mark.parametrize("pred,target,kwargs", [
    (_labels(), _labels(), dict(num_classes=17)),
    (_labels(), _labels(), dict(num_classes=0)),
    (_labels(1, 2049, 1), _labels(1, 2049, 1), dict()),
    (_labels(1, 1, 2049), _labels(1, 1, 2049), dict()),
    (_labels(), _labels(), dict(spacing=(-1.0, 1.0))),
    (_labels(), _labels(), dict(spacing=(1.0, 0.0))),
    (_labels(), _labels(), dict(percentile=101.0)),
    (_labels(1, 8, 8), _labels(1, 8, 9), dict()),
    (torch.zeros(2, 3, 8, 8), _labels(1, 8, 8), dict(num_classes=3)),
])
def test_bad_arguments_raise_before_the_device(pred, target, kwargs):
    from unet.utils.metrics import surface_distances
    with pytest.raises(ValueError):
        surface_distances(pred, target, **kwargs)


def test_host_tensors_need_a_gpu():
    from unet.utils import SurfaceDistanceMetrics, surface_distances
    if torch.cuda.is_available():
        assert surface_distances(_labels(), _labels())["hd"].is_cuda
        return
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        surface_distances(_labels(), _labels())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        SurfaceDistanceMetrics().update(torch.zeros(1, 2, 8, 8), _labels())
