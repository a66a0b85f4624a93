"""unet_upsample_bwd_pw with row-group tiles (a block owns several source rows and walks the union of their
destination windows once): the cases where the new row table, the ragged last row group, the block-index
decomposition and the 4- and 8-chunk forms can go wrong.

  kernel level   bit-identical to unet_conv (UNET_OUT_F32, accumulating into a copy of d_up) followed by
                 unet_upsample_bwd, at the smallest maps with the 16384 destination pixels the 1x1 MFMA kernel asks
                 for (asserted); operands inside sentinel-filled buffers that must come back untouched.
  padded frame   the same identity with the x2 map placed in a larger frame (pad_t or pad_l = 1), which the model
                 never asks of the fused call but the C ABI admits: the 1x1 reference runs over the whole frame.
  small maps     no bit-identical reference exists below the 1x1 kernel's threshold: the fp64 adjoint of
                 d_up + dgw.W^T (W the 16-bit-rounded weight) to the a-priori bound 2 (Ci + 16) 2^-24 S of
                 test_gpu_gate_up_fusion.py.
  model level    AttentionUNet(base 64) on 1 x 512^2 in bf16, one forward + DiceBCE + backward with and without
                 UNET_NO_GUP_FUSE from the same state: logits and every parameter gradient bit-identical, one fused
                 call per gate level that up_fused_ok admits."""

import os

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -12345.0          # (rounded to the buffer's type; compared in that type)
PAD = 4096               # sentinel elements on either side of an operand (keeps 16-byte alignment)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ENV = ("UNET_UPB_TILE", "UNET_PW_WIDE", "UNET_PW_XD", "UNET_PW_BLOCKS", "UNET_NO_GUP_FUSE")


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _prec(R, prec):
    return R.BF16 if prec == "bf16" else R.FP16


class Guarded:
    """a tensor of `shape` in the middle of a sentinel-filled buffer"""

    def __init__(self, shape, dtype, src=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n].view(*shape)
        self.n = n
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        s = torch.tensor(SENT, dtype=self.buf.dtype, device=DEV)
        return bool((self.buf[:PAD] == s).all()) and bool((self.buf[PAD + self.n:] == s).all())


def _inputs(prec, N, Hs, Ws, C, Ci, seed, frame=None):
    """d_up and dgw at the frame (default: the x2 map itself), W_g, dx's old value"""
    g = torch.Generator().manual_seed(seed)
    Hp, Wp = frame if frame else (2 * Hs, 2 * Ws)
    d_up = torch.randn(N, Hp, Wp, C, generator=g)
    dgw = (torch.randn(N, Hp, Wp, Ci, generator=g) * 0.5).to(DT[prec])
    w = torch.randn(Ci, C, 1, 1, generator=g) / Ci ** 0.5          # W_g: Conv2d(C, Ci, 1).weight
    dx0 = torch.randn(N, Hs, Ws, C, generator=g)
    return d_up.to(DEV), dgw.to(DEV), w.to(DEV), dx0.to(DEV)


def _dgrad_desc(L, R, prec, N, H, W, C, Ci, dgw, wt, out):
    d = L.ConvDesc()
    d.dtype = _prec(R, prec).code
    d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = N, H, W, Ci, C, 1, 1
    s = L.Src()
    s.kind, s.H, s.W, s.C, s.data = L.SRC_PLAIN, H, W, Ci, dgw.data_ptr()
    d.src[0] = s
    d.weight = wt.data_ptr()
    d.out_mode, d.out, d.accum, d.split = L.OUT_F32, out.data_ptr(), 1, C
    return d


def _geom(R, Hs, Ws, frame, pad):
    up_h, up_w = 2 * Hs, 2 * Ws
    Hp, Wp = frame if frame else (up_h, up_w)
    return up_h, up_w, Hp, Wp, pad[0], pad[1], R.up_scale(Hs, up_h), R.up_scale(Ws, up_w)


def _fused(L, R, prec, N, Hs, Ws, C, Ci, d_up, dgw, wt, dx, accum, frame=None, pad=(0, 0)):
    up_h, up_w, Hp, Wp, pt, pl, sh, sw = _geom(R, Hs, Ws, frame, pad)
    code = _prec(R, prec).code
    assert L.load().unet_upsample_bwd_pw_ok(code, N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, sh, sw, Ci)
    L.call("unet_upsample_bwd_pw", code, N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, sh, sw, R.vp(d_up), R.vp(dgw), Ci,
           R.vp(wt), R.vp(dx), accum, R.stream())
    torch.cuda.synchronize()


def _check_against_two_launches(prec, case, seed, frame=None, pad=(0, 0)):
    L, R = _lr()
    N, Hs, Ws, C, Ci = case
    up_h, up_w, Hp, Wp, pt, pl, sh, sw = _geom(R, Hs, Ws, frame, pad)
    d_up0, dgw0, w, dx0 = _inputs(prec, N, Hs, Ws, C, Ci, seed, frame)
    wt = R.pack_weight(w, _prec(R, prec), transpose=True)
    for accum in (0, 1):
        # the two launches: d_up += W_g^T dgw on the 1x1 MFMA kernel over the whole frame, then the adjoint
        d_ref = Guarded((N, Hp, Wp, C), torch.float32, d_up0)
        x_ref = Guarded((N, Hp, Wp, Ci), DT[prec], dgw0)
        o_ref = Guarded((N, Hs, Ws, C), torch.float32, dx0)
        d = _dgrad_desc(L, R, prec, N, Hp, Wp, C, Ci, x_ref.t, wt, d_ref.t)
        ws = L.attach_workspace(d, DEV)
        assert R.conv_kernel_name(d).startswith("pw_conv_kernel"), R.conv_kernel_name(d)
        L.call("unet_conv", d, R.stream())
        L.call("unet_upsample_bwd", N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, sh, sw, R.vp(d_ref.t), R.vp(o_ref.t), accum,
               R.stream())
        torch.cuda.synchronize()
        del ws
        # the fused call
        d_fu = Guarded((N, Hp, Wp, C), torch.float32, d_up0)
        x_fu = Guarded((N, Hp, Wp, Ci), DT[prec], dgw0)
        o_fu = Guarded((N, Hs, Ws, C), torch.float32, dx0)
        _fused(L, R, prec, N, Hs, Ws, C, Ci, d_fu.t, x_fu.t, wt, o_fu.t, accum, frame, pad)
        assert torch.isfinite(o_ref.t).all()
        assert torch.equal(o_fu.t, o_ref.t), (accum, float((o_fu.t - o_ref.t).abs().max()))
        for gd in (d_ref, x_ref, o_ref, d_fu, x_fu, o_fu):
            assert gd.intact()
        assert torch.equal(d_fu.t, d_up0) and torch.equal(x_fu.t, dgw0)      # the fused call writes dx only
        assert torch.equal(x_ref.t, dgw0)


# (N, Hs, Ws, C, Ci), each the smallest map with the 16384 destination pixels the 1x1 kernel asks for:
#  a prime row count (the last row group is ragged whatever the group size), three images (the block-index
#    decomposition) and a ragged last column tile;
#  fewer rows than a row group, 22 column tiles, the last one ragged;
#  4 chunks of projection channels, two channel tiles, one row past a multiple of 2, 4 and 8;
#  8 chunks, four channel tiles, ragged both ways
KERNEL_CASES = [(3, 37, 40, 64, 32), (4, 3, 342, 64, 64), (1, 33, 128, 128, 128), (1, 35, 120, 256, 256)]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_row_groups_bit_identical_to_two_calls(case, prec, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    _check_against_two_launches(prec, case, 21)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("pad", [(1, 0), (0, 1)], ids=["pad_t", "pad_l"])
def test_padded_frame_bit_identical_to_two_calls(pad, prec, monkeypatch):
    """the 64 x 128 map of a 32 x 64 source inside a 65 x 129 frame, one row down or one column right: the row table
    (and the column table) must place the window rows at u + pad_t (v + pad_l) of the frame"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    _check_against_two_launches(prec, (2, 32, 64, 64, 32), 22, frame=(65, 129), pad=pad)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("cc", [(64, 32), (128, 128), (64, 64)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("geo", [(1, 2, 3), (2, 5, 7)], ids=lambda g: "x".join(map(str, g)))
def test_small_maps_against_fp64(geo, cc, accum, prec, monkeypatch):
    L, R = _lr()
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    N, Hs, Ws = geo
    C, Ci = cc
    H, W = 2 * Hs, 2 * Ws
    d_up0, dgw0, w, dx0 = _inputs(prec, N, Hs, Ws, C, Ci, 23)
    wt = R.pack_weight(w, _prec(R, prec), transpose=True)
    d_fu = Guarded((N, H, W, C), torch.float32, d_up0)
    x_fu = Guarded((N, H, W, Ci), DT[prec], dgw0)
    o_fu = Guarded((N, Hs, Ws, C), torch.float32, dx0)
    _fused(L, R, prec, N, Hs, Ws, C, Ci, d_fu.t, x_fu.t, wt, o_fu.t, accum)
    for gd in (d_fu, x_fu, o_fu):
        assert gd.intact()
    assert torch.equal(d_fu.t, d_up0) and torch.equal(x_fu.t, dgw0)
    w16 = w.reshape(Ci, C).to(DT[prec]).double()                    # the 16-bit-rounded weight
    v = d_up0.double() + dgw0.double() @ w16
    va = d_up0.double().abs() + dgw0.double().abs() @ w16.abs()
    old = dx0 if accum else None
    ref = RO.upsample_bwd(v, Hs, Ws, H, W, 0, 0, old)
    S = RO.upsample_bwd(va, Hs, Ws, H, W, 0, 0, old.abs() if accum else None)
    tol = 2 * (Ci + 16) * 2.0 ** -24 * S
    err = (o_fu.t.double() - ref).abs()
    print(f"max err {float(err.max()):.3e}  max err/tol {float((err / tol).max()):.3f}")
    assert torch.isfinite(o_fu.t).all()
    assert (err <= tol).all(), RO._worst(err, tol)


def _step(model, x, t, env, seen, admitted):
    from unet._hip import lib as L, stages as S
    from unet.utils.loss import DiceBCELoss
    keys = ("UNET_NO_GUP_FUSE", "UNET_UPB_TILE", "UNET_PW_WIDE")
    old = {k: os.environ.get(k) for k in keys}
    orig, orig_ok = L.call, S.GateStage.up_fused_ok

    def rec(name, *args):
        seen.append(name)
        return orig(name, *args)

    def ok(self, prec, g, xx):
        r = orig_ok(self, prec, g, xx)
        admitted.append((self.ci, bool(r)))
        return r

    L.call = rec
    S.GateStage.up_fused_ok = ok
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        model.zero_grad(set_to_none=True)
        out = model(x)
        DiceBCELoss()(out, t).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    finally:
        L.call = orig
        S.GateStage.up_fused_ok = orig_ok
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_model_backward_bit_identical_512():
    """base 64 on 1 x 512^2: the gates at 512^2, 256^2 and 128^2 (Ci 32, 64, 128; 262144, 65536 and 16384 pixels)
    have a W_g dgrad on the 1x1 MFMA kernel and are eligible; the Ci 256 gate at 64^2 is not (4096 pixels)."""
    from unet.models import AttentionUNet
    torch.manual_seed(3)
    m = AttentionUNet(1, 2, base_features=64).cuda().train()
    m.hip_precision = "bf16"
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(1, 1, 512, 512, generator=g) * 2 - 1).cuda()
    t = (torch.rand(1, 512, 512, generator=g) < 0.1).long().cuda()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    seen0, seen1, adm0, adm1 = [], [], [], []
    out0, g0 = _step(m, x, t, {}, seen0, adm0)
    m.load_state_dict(state)   # the same BN running statistics going in
    out1, g1 = _step(m, x, t, {"UNET_NO_GUP_FUSE": "1"}, seen1, adm1)
    n0, n1 = seen0.count("unet_upsample_bwd_pw"), seen1.count("unet_upsample_bwd_pw")
    assert n1 == 0 and not any(r for _, r in adm1)
    assert len(adm0) == 4, adm0
    assert n0 == sum(r for _, r in adm0), (n0, adm0)
    assert n0 >= 2, adm0
    assert not dict(adm0)[256], adm0     # too few pixels for the 1x1 kernel whatever the policy
    # each fused call stands for one adjoint and one 1x1 dgrad of the other run
    assert seen0.count("unet_upsample_bwd") == seen1.count("unet_upsample_bwd") - n0
    assert seen0.count("unet_conv") == seen1.count("unet_conv") - n0
    assert torch.equal(out0, out1)
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff
