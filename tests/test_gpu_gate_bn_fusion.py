"""unet_bn_bwd_reduce_pool_gate / unet_bn_bwd_apply_pool_gate: the pooled BatchNorm backward of an attention Up
block's skip activation that forms the gate's gradient of that activation, W_x^T dxw + sigmoid(a p + b) d(x s), on
the fly, against the three launches it replaces.

  kernel level   bit identity (torch.equal) with unet_conv (UNET_OUT_F32_GATED, asserted to run on pw_conv_kernel)
                 -> unet_bn_bwd_reduce_pool -> unet_bn_bwd_finalize -> unet_bn_bwd_apply_pool on the same inputs: the
                 partial sums [2][rows][C], dgamma, dbeta, coef and dy.  Every output sits between NaN sentinels
                 that must come back untouched, and is NaN-filled itself.
  fp64           the same outputs against the fp64 restatement of tests/ref_ops.py (never another kernel), at the
                 gates of tests/test_gpu_bn_gate_ops.py: partial sums 2e-5 sum|terms| + 1e-6 (the terms being those
                 of the formed gradient: the Ci products, s d(x s) and the routed pooled value), dy at the 16-bit
                 gate eps |ref| + eps 1e-3 max|ref| with the kernel's own coef as input.
  model level    AttentionUNet(1, 2) at 4 x 128^2, bf16: loss and every parameter gradient bit-identical with and
                 without UNET_NO_GATE_BN_FUSE; both served levels (4 x 128^2 x 64, 4 x 64^2 x 128) take the new calls,
                 counted through L.call.  UNet and fp32 mode never do.
  fallback       a second contribution to the skip's gradient after the deferral stores dx with the deferred launch.

Shapes: the smallest with the 16384 pixels the 1x1 kernel asks for.  A: P = 16512 is no multiple of the partial
row length (ragged last row) and C 64 has two 16-pixel tile classes per block; B: odd H and W (last row / column
without a pooled gradient), three images, two chunks, one tile class (R = 16), 16650 pixels."""

import functools
import os

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
PAD = 4096
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = {"A": (1, 128, 129, 64, 32), "B": (3, 74, 75, 128, 64)}


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


class Guarded:
    """a NaN-filled tensor of `shape` in the middle of a NaN-filled buffer"""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), NAN, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.n = n

    def ok(self):
        """written everywhere, and nowhere outside"""
        return bool(torch.isfinite(self.t).all()) and bool(torch.isnan(self.buf[:PAD]).all()) \
            and bool(torch.isnan(self.buf[PAD + self.n:]).all())


@functools.lru_cache(maxsize=None)
def _inputs(case, prec):
    N, H, W, C, Ci = CASES[case]
    dt = DT[prec]
    g = torch.Generator().manual_seed(41)
    ph, pw = H // 2, W // 2
    t = dict(
        # about half the pre-activations y * scale + shift are negative (y symmetric, small shifts, mixed signs)
        y=(torch.randn(N, H, W, C, generator=g) * 1.5).to(dt),
        dxs=torch.randn(N, H, W, C, generator=g),
        dxw=(torch.randn(N, H, W, Ci, generator=g) * 0.5).to(dt),
        w=torch.randn(Ci, C, 1, 1, generator=g) / Ci ** 0.5,            # W_x: Conv2d(C, Ci, 1).weight
        p=torch.randn(N, H, W, generator=g) * 2,
        pab=torch.tensor([0.7, -0.2]),
        g2=torch.randn(N, ph, pw, C, generator=g),
        code=torch.randint(0, 4, (N, ph, pw, C), generator=g, dtype=torch.uint8),   # every window position occurs
        scale=(torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0),
        shift=torch.randn(C, generator=g) * 0.1,
        mean=torch.randn(C, generator=g) * 0.3,
        invstd=torch.rand(C, generator=g) * 1.5 + 0.5,
        gamma=torch.randn(C, generator=g) * 0.3 + 1.0,
    )
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


def _three_launches(case, prec):
    """partial, dgamma, dbeta, coef, dy of today's route"""
    L, R = _lr()
    N, H, W, C, Ci = CASES[case]
    P, ph, pw = N * H * W, H // 2, W // 2
    pr = R._PRECISIONS[prec]
    i = _inputs(case, prec)
    vp = R.vp
    wt = R.pack_weight(i["w"], pr, transpose=True)
    dx = Guarded((N, H, W, C), torch.float32)
    d = L.ConvDesc()
    d.dtype = pr.code
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = N, H, W, Ci, C, 1, 1
    s = L.Src()
    s.kind, s.H, s.W, s.C, s.data = L.SRC_PLAIN, H, W, Ci, i["dxw"].data_ptr()
    d.src[0] = s
    d.weight = wt.data_ptr()
    d.out_mode, d.out, d.accum, d.split = L.OUT_F32_GATED, dx.t.data_ptr(), 0, C
    ps = L.Src()
    ps.kind, ps.C, ps.H, ps.W = L.SRC_PLAIN, C, H, W
    ps.data, ps.gate_p, ps.gate_ab = vp(i["dxs"]), vp(i["p"]), vp(i["pab"])
    d.pool_src = ps
    ws = L.attach_workspace(d, DEV)
    assert R.conv_kernel_name(d).startswith("pw_conv_kernel"), R.conv_kernel_name(d)
    L.call("unet_conv", d, R.stream())
    rows = L.load().unet_bn_bwd_reduce_rows(P, C)
    part = Guarded((2, rows, C), torch.float32)
    L.call("unet_bn_bwd_reduce_pool", pr.code, N, H, W, C, vp(dx.t), vp(i["g2"]), vp(i["code"]), ph, pw, vp(i["y"]),
           vp(i["scale"]), vp(i["shift"]), 1, vp(i["mean"]), vp(i["invstd"]), vp(part.t), R.stream())
    dg, db, coef = (Guarded((C,), torch.float32), Guarded((C,), torch.float32), Guarded((3, C), torch.float32))
    L.call("unet_bn_bwd_finalize", vp(part.t[0]), vp(part.t[1]), rows, C, P, vp(i["gamma"]), vp(i["mean"]),
           vp(i["invstd"]), vp(dg.t), vp(db.t), 0, vp(coef.t), R.stream())
    dy = Guarded((N, H, W, C), DT[prec])
    L.call("unet_bn_bwd_apply_pool", pr.code, N, H, W, C, vp(dx.t), vp(i["g2"]), vp(i["code"]), ph, pw, vp(i["y"]),
           vp(i["scale"]), vp(i["shift"]), 1, vp(coef.t), vp(dy.t), R.stream())
    torch.cuda.synchronize()
    for gd in (dx, part, dg, db, coef, dy):
        assert gd.ok()
    return part, dg, db, coef, dy


def _two_launches(case, prec):
    L, R = _lr()
    N, H, W, C, Ci = CASES[case]
    P, ph, pw = N * H * W, H // 2, W // 2
    pr = R._PRECISIONS[prec]
    i = _inputs(case, prec)
    vp = R.vp
    wt = R.pack_weight(i["w"], pr, transpose=True)
    assert L.load().unet_bn_bwd_pool_gate_ok(pr.code, N, H, W, C, Ci)
    rows = L.load().unet_bn_bwd_reduce_rows(P, C)
    part = Guarded((2, rows, C), torch.float32)
    head = (pr.code, N, H, W, C, Ci, vp(i["dxs"]), vp(i["dxw"]), vp(wt), vp(i["p"]), vp(i["pab"]), vp(i["g2"]),
            vp(i["code"]), ph, pw, vp(i["y"]), vp(i["scale"]), vp(i["shift"]), 1)
    L.call("unet_bn_bwd_reduce_pool_gate", *head, vp(i["mean"]), vp(i["invstd"]), vp(part.t), R.stream())
    dg, db, coef = (Guarded((C,), torch.float32), Guarded((C,), torch.float32), Guarded((3, C), torch.float32))
    L.call("unet_bn_bwd_finalize", vp(part.t[0]), vp(part.t[1]), rows, C, P, vp(i["gamma"]), vp(i["mean"]),
           vp(i["invstd"]), vp(dg.t), vp(db.t), 0, vp(coef.t), R.stream())
    dy = Guarded((N, H, W, C), DT[prec])
    L.call("unet_bn_bwd_apply_pool_gate", *head, vp(coef.t), vp(dy.t), R.stream())
    torch.cuda.synchronize()
    for gd in (part, dg, db, coef, dy):
        assert gd.ok()
    return part, dg, db, coef, dy


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_launches_bit_identical_to_three(case, prec, monkeypatch):
    for k in ("UNET_BN_ROWS", "UNET_PW_WIDE", "UNET_PW_XD", "UNET_PW_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    before = {k: v.clone() for k, v in _inputs(case, prec).items()}
    ref = _three_launches(case, prec)
    got = _two_launches(case, prec)
    for name, a, b in zip(("partial", "dgamma", "dbeta", "coef", "dy"), got, ref):
        assert torch.equal(a.t, b.t), (name, float((a.t.double() - b.t.double()).abs().max()))
    for k, v in _inputs(case, prec).items():       # the operands are read only
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_launches_against_fp64(case, prec, monkeypatch):
    monkeypatch.delenv("UNET_BN_ROWS", raising=False)
    N, H, W, C, Ci = CASES[case]
    i = _inputs(case, prec)
    part, dg, db, coef, dy = _two_launches(case, prec)
    w16 = i["w"].reshape(Ci, C).to(DT[prec]).double()                  # the 16-bit-rounded weight
    s = torch.sigmoid(i["p"].double() * i["pab"][0].double() + i["pab"][1].double()).unsqueeze(-1)
    da = i["dxw"].double() @ w16 + s * i["dxs"].double()
    da_abs = i["dxw"].double().abs() @ w16.abs() + s * i["dxs"].double().abs()
    da = RO.pool_bwd(i["g2"], i["code"], H, W, da).reshape(-1, C)
    da_abs = RO.pool_bwd(i["g2"].abs(), i["code"], H, W, da_abs).reshape(-1, C)
    y = i["y"].reshape(-1, C)
    ref = RO.bn_bwd_sums(da, y, i["scale"], i["shift"], 1, i["mean"], i["invstd"])
    passed = y.double() * i["scale"].double() + i["shift"].double() > 0
    abs_g = torch.where(passed, da_abs, torch.zeros_like(da_abs))
    abs_gx = abs_g * (y.double().abs() + i["mean"].double().abs()) * i["invstd"].double().abs()
    got = part.t.double().sum(1)
    RO.check_sums(got[0], ref.sum_g, abs_g.sum(0), "sum g")
    RO.check_sums(got[1], ref.sum_gx, abs_gx.sum(0), "sum g xhat")
    frac = 1.0 - float(passed.double().mean())
    print(f"masked fraction {frac:.3f}")
    assert 0.3 < frac < 0.7
    r = RO.bn_bwd_apply(ref.g, y, coef.t)
    RO.check_elem(dy.t, r.dy.reshape(N, H, W, C), r.abs_terms, prec, "dy")


# ---- model level ------------------------------------------------------------------------------------------

ENV_KEYS = ("UNET_NO_GATE_BN_FUSE", "UNET_NO_GATE_FUSE", "UNET_NO_POOL_FOLD", "UNET_PW_WIDE", "UNET_BN_ROWS")
NEW = ("unet_bn_bwd_reduce_pool_gate", "unet_bn_bwd_apply_pool_gate")


def _step(model, x, t, env, seen):
    from unet._hip import lib as L
    from unet.utils.loss import DiceBCELoss
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    orig = L.call

    def rec(name, *args):
        seen.append(name)
        return orig(name, *args)

    L.call = rec
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        model.zero_grad(set_to_none=True)
        loss = DiceBCELoss()(model(x), t)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    finally:
        L.call = orig
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ab(model, prec, seed=3):
    """one step with the route on and one with UNET_NO_GATE_BN_FUSE from the same state"""
    torch.manual_seed(seed)
    m = model().cuda().train()
    m.hip_precision = prec
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(4, 1, 128, 128, generator=g) * 2 - 1).cuda()
    t = (torch.rand(4, 128, 128, generator=g) < 0.1).long().cuda()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    seen0, seen1 = [], []
    l0, g0 = _step(m, x, t, {}, seen0)
    m.load_state_dict(state)   # the same BN running statistics going in
    l1, g1 = _step(m, x, t, {"UNET_NO_GATE_BN_FUSE": "1"}, seen1)
    assert torch.equal(l0, l1)
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff
    assert all(torch.isfinite(v).all() for v in g0.values())
    return seen0, seen1


def test_model_backward_bit_identical():
    from unet.models import AttentionUNet
    seen0, seen1 = _ab(lambda: AttentionUNet(1, 2), "bf16")
    for n in NEW:
        assert seen0.count(n) == 2 and seen1.count(n) == 0, (n, seen0.count(n), seen1.count(n))
    # each fused level drops its pooled passes and its gated dgrad
    assert seen0.count("unet_bn_bwd_reduce_pool") == seen1.count("unet_bn_bwd_reduce_pool") - 2
    assert seen0.count("unet_bn_bwd_apply_pool") == seen1.count("unet_bn_bwd_apply_pool") - 2
    assert seen0.count("unet_conv") == seen1.count("unet_conv") - 2


@pytest.mark.parametrize("kind", ["unet_bf16", "attention_fp32"])
def test_other_configurations_untouched(kind):
    from unet.models import AttentionUNet, UNet
    if kind == "unet_bf16":
        seen0, seen1 = _ab(lambda: UNet(1, 2), "bf16")
    else:
        seen0, seen1 = _ab(lambda: AttentionUNet(1, 2), "fp32")
    assert seen0 == seen1
    assert not any(n in seen0 for n in NEW)


def test_second_contribution_stores_the_deferred_gradient(monkeypatch):
    """The top level's skip activation gets another gradient contribution between the gate's backward and its own
    BatchNorm backward (added here at the start of the Down block's backward, in both runs): the deferred dgrad
    is then launched as it would have been, and the level takes the three-launch route with the same bits."""
    from unet._hip import stages as S
    from unet.models import AttentionUNet
    orig = S.DownStage.backward
    hits = []

    def backward(self, prec, grads):
        x = self.x
        if x.C == 64:
            pending = x.gate_fused is not None
            g, acc = x.grad_target()
            assert acc == 1 and x.gate_fused is None     # dx is there: stored by the gate, or by the flush just now
            g += 0.25
            hits.append(pending)
        return orig(self, prec, grads)

    monkeypatch.setattr(S.DownStage, "backward", backward)
    seen0, seen1 = _ab(lambda: AttentionUNet(1, 2), "bf16")
    assert hits == [True, False]
    for n in NEW:
        assert seen0.count(n) == 1 and seen1.count(n) == 0     # the 64^2 level still defers
    assert seen0.count("unet_conv") == seen1.count("unet_conv") - 1
