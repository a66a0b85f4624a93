"""CPU: the argument checks of unet.utils.connected_components / filter_components run before anything touches the
device, host tensors on a machine without a GPU meet the package's usual error (there is no CPU path), and the
workspace query answers without a device."""

import pytest
import torch


def _labels(n=1, h=8, w=8, dtype=torch.int64):
    return torch.zeros(n, h, w, dtype=dtype)


@pytest.mark.parametrize("pred,kwargs", [
    (_labels(), dict(num_classes=17)),
    (_labels(), dict(num_classes=0)),
    (_labels(dtype=torch.uint8), dict(num_classes=3)),
    (_labels(), dict(connectivity=6)),
    (_labels(), dict(background=2)),
    (_labels(), dict(background=-2)),
    (_labels(1, 4097, 1), dict()),
    (_labels(1, 1, 4097), dict()),
    (torch.zeros(8, 8, dtype=torch.int64), dict()),
    (torch.zeros(2, 0, 8, 8), dict()),
    (torch.zeros(1, dtype=torch.uint8).expand(2 ** 19, 64, 64), dict()),     # N * H * W = 2^31
])
def test_bad_arguments_raise_before_the_device(pred, kwargs):
    from unet.utils import connected_components, filter_components
    with pytest.raises(ValueError):
        connected_components(pred, **kwargs)
    with pytest.raises(ValueError):
        filter_components(pred, min_size=3, **kwargs)


def test_host_tensors_need_a_gpu():
    from unet.utils import connected_components, filter_components
    if torch.cuda.is_available():
        assert connected_components(_labels())["count"].is_cuda and filter_components(_labels()).is_cuda
        return
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        connected_components(_labels())
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        filter_components(_labels(dtype=torch.uint8), min_size=4)


def test_workspace_query():
    from unet._hip import lib as L
    ws = L.load().unet_cc_workspace
    assert "unet_cc_workspace" in L._NO_LAUNCH
    assert ws(2, 70, 130) >= 2 * 70 * 130 * 4 and ws(1, 1, 1) > 0 and ws(1, 4096, 4096) > 0
    for shape in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 4097, 8), (1, 8, 4097), (128, 4096, 4096)):
        assert ws(*shape) == 0, shape
