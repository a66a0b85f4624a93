"""GPU: every weight-gradient kernel form against fp64, bit for bit (the method of tests/test_gpu_conv_exact.py).

dw is compared in OIHW with torch.equal: the split-K slabs are fp32 and every partial sum of grid operands is exact,
whatever the split count, the slab order or the reduction tree.  dw sits between NaN sentinels (prefilled with grid
values where the call accumulates) and the workspace is NaN-filled, so a slab read before it is written shows."""

import pytest

import conv_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CC.WGRAD_CASES, ids=[c["id"] for c in CC.WGRAD_CASES])
def test_wgrad_exact(case, monkeypatch):
    from unet._hip import lib as L
    from unet._hip import runtime as R
    CC.set_env(case, monkeypatch)
    o = CC.to_device(CC.wgrad_operands(case), "cuda")
    ref = CC.wgrad_reference(case, o)
    run = CC.launch_wgrad(L, R, case, o)
    CC.check_outputs(case, run, ref)
