"""GPU: the first conv with 5 to 16 fp32 NCHW input channels (csrc/stem.hip) against fp64.

The exact-grid method of tests/conv_cases.py with a finer input grid: x = k/4096, |k| <= 4095 (12 significant bits:
representable in neither bf16 nor fp16, exactly x_hi + x_lo in both, x_lo a normal fp16 number), weights k/8 with
|w| <= 1/2, dy = k/4 with |dy| <= 1.  Forward: every product is a multiple of 2^-15 and Σ|terms| <= 144·½·1 = 72 =
2.4e6 units < 2^24, so a correct kernel's fp32 accumulator equals the fp64 value and the 16-bit output its single
rounding.  Weight gradient: unit 2^-14, Σ|dy·x| ~ 0.3·P units·2^14 against the cap of 1024 (P <= 1260), asserted per
draw.  A kernel that rounds x to 16 bits first (the generic route) differs in nearly every element."""

import functools
from types import SimpleNamespace as NS

import pytest
import torch

import conv_cases as CC
import ref_ops as ro
from fullsize_common import discs, grad_errs, hip_run, oracle_run, rel_l2, seeded_init

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7), (2, 9, 70), (1, 17, 33)]   # below one 8 x 64 tile; one row / six columns over, N = 2; 3 row tiles
UX, UW, UDY = 2.0 ** -12, 0.125, 0.25
grid_params = pytest.mark.parametrize("dt,cout,cin,shape", [(dt, co, ci, s) for dt in ("bf16", "fp16") for co in (32, 64)
                                                            for ci in (5, 8, 9, 16) for s in SHAPES])


@functools.lru_cache(maxsize=None)
def _operands(cin, cout, shape):
    """x, w, dy, old (CPU, fp32) and the fp64 references of both kernels, shared by the dtypes"""
    N, H, W = shape
    gen = torch.Generator().manual_seed(1000 * cin + 10 * cout + H)
    x = ro.grid((N, cin, H, W), UX, 4095, torch.float32, gen)
    w = ro.grid((cout, cin, 3, 3), UW, 4, torch.float32, gen)
    dy = ro.grid((N, H, W, cout), UDY, 4, torch.float32, gen)
    old = ro.grid((cout, cin, 3, 3), UDY, 12, torch.float32, gen)
    xh = x.double().permute(0, 2, 3, 1).contiguous()
    return NS(x=x, w=w, dy=dy, old=old, fwd=ro.conv_fwd(xh, w.double(), 3), wg=ro.conv_wgrad(xh, dy.double(), 3))


def _src(x):
    return [NS(x=x.cuda(), scale=None, shift=None, gate_p=None, gate_ab=None)]


@grid_params
def test_stem_forward_exact(monkeypatch, dt, cout, cin, shape):
    from unet._hip import lib as L
    from unet._hip import runtime as R
    monkeypatch.delenv("UNET_STEM_MFMA", raising=False)
    p = _operands(cin, cout, shape)
    case = CC.conv(f"stem-{dt}-{cin}-{cout}-{shape}", dt, 3, shape, [CC.S("nchw", cin)], cout,
                   f"stem_fwd_mfma_kernel<{dt},{cout}>", stats=1)
    run = CC.launch_conv(L, R, case, NS(srcs=_src(p.x), w=p.w.cuda()))
    assert ro.exact_units(p.fwd.abs_terms, UX * UW) < ro.EXACT_CAP
    run.outs["out"].check(case["id"])
    ro.check_exact(run.outs["out"].body.cpu(), p.fwd.y, CC.DT[dt], case["id"])
    st = ro.conv_stats(p.fwd.y)
    ro.check_sums(run.stats[0].cpu(), st.sum, st.abs_sum, case["id"] + " Σy")
    ro.check_sums(run.stats[1].cpu(), st.sumsq, st.abs_sumsq, case["id"] + " Σy²")


@pytest.mark.parametrize("accum", [0, 1])
@grid_params
def test_stem_wgrad_exact(monkeypatch, dt, cout, cin, shape, accum):
    from unet._hip import lib as L
    from unet._hip import runtime as R
    monkeypatch.delenv("UNET_STEM_MFMA", raising=False)
    p = _operands(cin, cout, shape)
    case = CC.wgrad(f"stem-{dt}-{cin}-{cout}-{shape}-{accum}", dt, 3, shape, [CC.S("nchw", cin)], cout,
                    f"stem_wgrad_mfma_kernel<{dt},{cout}>", accum=accum)
    want, a = p.wg.dw, p.wg.abs_terms
    if accum:
        want, a = want + p.old.double(), a + p.old.double().abs()
    assert ro.exact_units(a, UX * UDY) < ro.EXACT_CAP
    o = NS(srcs=_src(p.x), dy=p.dy.to(CC.DT[dt]).cuda(), old=p.old.cuda() if accum else None)
    run = CC.launch_wgrad(L, R, case, o)
    run.outs["dw"].check(case["id"])
    ro.check_exact(run.outs["dw"].body.cpu(), want, torch.float32, case["id"], ("co", "ci", "kh", "kw"), (16, 16, 0, 0))
    if shape == SHAPES[1]:   # no atomics: a second call gives the same bits
        again = CC.launch_wgrad(L, R, case, o)
        assert torch.equal(again.outs["dw"].body, run.outs["dw"].body)


@pytest.mark.parametrize("kind,in_ch,prec", [("unet", 9, "bf16"), ("attention", 5, "fp16")])
def test_stem_through_the_models(monkeypatch, kind, in_ch, prec):
    """UNet / AttentionUNet with a multi-channel input, forward + DiceBCE + backward against the fp64 oracle: logits,
    all-parameter gradients and the first conv's weight gradient within 1.1 x torch autocast's own error + 5e-3."""
    monkeypatch.delenv("UNET_STEM_MFMA", raising=False)
    init = seeded_init(kind, in_ch)
    g = torch.Generator().manual_seed(31 + in_ch)
    x = torch.rand(2, in_ch, 64, 64, generator=g) * 2 - 1
    t = discs(2, 64, 64, g)
    f64 = oracle_run(init, x, t, "cuda", torch.float64, kind=kind, want_eval=False)
    ac = oracle_run(init, x, t, "cuda", torch.float32, kind=kind, want_eval=False,
                    autocast=torch.bfloat16 if prec == "bf16" else torch.float16)
    log = []
    _, out, _, grads = hip_run(init, x, t, prec, kind=kind, in_ch=in_ch, log=log)
    names = {k for k, _ in log}
    assert f"stem_fwd_mfma_kernel<{prec},64>" in names and not any(n.startswith("conv_generic") for n in names), names
    k0 = "inc.double_conv.0.weight"
    ours = (rel_l2(out, f64["out"]), grad_errs(grads, f64["grads"])[2], rel_l2(grads[k0], f64["grads"][k0]))
    theirs = (rel_l2(ac["out"], f64["out"]), grad_errs(ac["grads"], f64["grads"])[2],
              rel_l2(ac["grads"][k0], f64["grads"][k0]))
    print(f"\n{kind} {in_ch} ch {prec}: logits / all grads / {k0} rel-L2 ours {ours} autocast {theirs}")
    for e, e_a in zip(ours, theirs):
        assert e <= 1.1 * e_a + 5e-3, (ours, theirs)
