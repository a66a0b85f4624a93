"""CPU: the host side of the optimizer tail (unet/utils/optim.py, unet/utils/general.py): the chunk map, the
reference's import line, and the constructor's argument checks."""

import numpy as np
import pytest
import torch


def test_chunk_map_covers_every_element_once():
    from unet._hip import lib as L
    from unet.utils.optim import CHUNK, build_chunk_map
    sizes = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
    cmap = build_chunk_map(sizes)
    assert cmap.dtype == np.int32 and cmap.shape[1] == 2
    seen = [np.zeros(n, np.int64) for n in sizes]
    for s, c in cmap:
        assert 0 <= s < len(sizes) and 0 <= c * CHUNK < sizes[s]
        seen[s][c * CHUNK:min((c + 1) * CHUNK, sizes[s])] += 1
    assert all((a == 1).all() for a in seen)
    # the library's kernels cut the same chunks
    assert CHUNK == L.OPTIM_CHUNK
    assert [int((cmap[:, 0] == s).sum()) for s in range(len(sizes))] == [L.load().unet_optim_chunks(n) for n in sizes]


def test_reference_import_line_resolves():
    from unet.utils.general import ModelEMA, set_seed, get_device, load_config, increment_path  # noqa: F401
    from unet.utils import FusedClipAdamW, ModelEMA as E2, config
    assert E2 is ModelEMA and load_config is config.load_config
    assert issubclass(FusedClipAdamW, torch.optim.Optimizer)


@pytest.mark.parametrize("kw", [{"lr": -1e-3}, {"eps": -1e-8}, {"betas": (1.0, 0.999)}, {"betas": (0.9, -0.1)},
                                {"weight_decay": -1.0}])
def test_constructor_rejects_what_torch_rejects(kw):
    from unet.utils.optim import FusedClipAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        torch.optim.AdamW(p, **kw)
    with pytest.raises(ValueError):
        FusedClipAdamW(p, **kw)
