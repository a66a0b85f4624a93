"""GPU: every conv / dgrad kernel form against fp64, bit for bit.

The cases of tests/conv_cases.py draw every operand on a dyadic grid, so every product is a multiple of one unit and
every partial sum of a correct kernel's fp32 accumulator is exact (tests/test_conv_cases_cpu.py proves the condition
for each case): the fp32 outputs must EQUAL the fp64 reference of tests/ref_ops.py, the 16-bit ones its single
round-to-nearest-even.  No tolerance is chosen; one dropped, doubled or misplaced term fails.  Weights go through
unet_pack_weight (transposed for the dgrads), so the packing is inside the claim.  Every output sits between NaN
sentinels, the partial-sum tables are sized by unet_conv_stats_rows and NaN-prefilled, the workspace is NaN-filled.
The few cases marked gate='elem' (an fp32 operand through a gate's sigmoid, the general-scale bilinear) use
ref_ops.check_elem."""

import pytest
import torch

import conv_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CC.CONV_CASES, ids=[c["id"] for c in CC.CONV_CASES])
def test_conv_exact(case, monkeypatch):
    from unet._hip import lib as L
    from unet._hip import runtime as R
    CC.set_env(case, monkeypatch)
    o = CC.to_device(CC.conv_operands(case), "cuda")
    ref = CC.conv_reference(case, o)
    run = CC.launch_conv(L, R, case, o)
    CC.check_outputs(case, run, ref)
    gates = list(case["sums"])
    if run.stats is not None:
        CC.check_sums(case, run.stats, ref.sums["stats"], gates[:2], "stats")
        gates = gates[2:]
    if run.bnb is not None:
        CC.check_sums(case, run.bnb, ref.sums["bnb"], gates[:2], "bnb")
    if case["out"] == "pool_bwd":   # rows / columns past the last window keep their prefill
        N, H, W = case["shape"]
        body = run.outs["out"].body
        assert torch.equal(body[:, 2 * H:], o.old[:, 2 * H:]) and torch.equal(body[:, :, 2 * W:], o.old[:, :, 2 * W:])
