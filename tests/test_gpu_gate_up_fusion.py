"""unet_upsample_bwd_pw: the bilinear adjoint that forms the attention gate's W_g input gradient (a 1x1 dgrad,
Ci -> C channels, accumulated into d_up) as it loads d_up, against the two launches it replaces.

  kernel level   where the 1x1 dgrad runs on pw_conv_kernel (>= 16384 destination pixels, asserted), the fused call
                 is bit-identical to unet_conv (UNET_OUT_F32, accumulating into a copy of d_up) followed by
                 unet_upsample_bwd: the same MFMA chain from zero, the same fp32 add, the same adjoint.  Every
                 operand sits inside a larger sentinel-filled buffer that must come back untouched.
  small maps     below that threshold no bit-identical reference exists: the fp64 adjoint of d_up + dgw.W^T (W the
                 16-bit-rounded weight) from tests/ref_ops.py, to the a-priori bound 2 (Ci + 16) 2^-24 S, S the same
                 expression on absolute values (all interpolation weights are non-negative): Ci products and sums in
                 fp32 for the projection, one add, up to 8 + 7 fmaf steps of the two adjoint phases and one for dx's
                 old value, the factor 2 for the MFMA's internal accumulation order.
  model level    one forward + DiceBCE + backward of AttentionUNet(base 64) with and without UNET_NO_GUP_FUSE from
                 the same state: logits and every parameter gradient bit-identical; the fused entry point runs in one
                 run only, and never in fp32."""

import os

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -12345.0          # (rounded to the buffer's type; compared in that type)
PAD = 4096               # sentinel elements on either side of an operand (keeps 16-byte alignment)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


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


def _inputs(prec, N, Hs, Ws, C, Ci, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = 2 * Hs, 2 * Ws
    d_up = torch.randn(N, H, W, C, generator=g)
    dgw = (torch.randn(N, H, W, Ci, generator=g) * 0.5).to(DT[prec])
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


def _fused(L, R, prec, N, Hs, Ws, C, Ci, d_up, dgw, wt, dx, accum):
    H, W = 2 * Hs, 2 * Ws
    sh, sw = R.up_scale(Hs, H), R.up_scale(Ws, W)
    code = _prec(R, prec).code
    assert L.load().unet_upsample_bwd_pw_ok(code, N, C, Hs, Ws, H, W, 0, 0, H, W, sh, sw, Ci)
    L.call("unet_upsample_bwd_pw", code, N, C, Hs, Ws, H, W, 0, 0, H, W, sh, sw, R.vp(d_up), R.vp(dgw), Ci, R.vp(wt),
           R.vp(dx), accum, R.stream())
    torch.cuda.synchronize()


# (N, Hs, Ws, C, Ci): one chunk and several column tiles; two channel tiles with a ragged last column tile
# (104 = 6 * 16 + 8); 8 chunks and 8 channel tiles; a destination row that is no multiple of the 16-pixel MFMA tile
# (230 columns) with a ragged source column tile (115 = 7 * 16 + 3).  Each is the smallest map that still has the
# 16384 destination pixels the 1x1 kernel asks for
KERNEL_CASES = [(2, 32, 128, 64, 32), (1, 40, 104, 128, 64), (1, 64, 64, 512, 256), (1, 36, 115, 64, 32)]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_call_bit_identical_to_two_calls(case, prec, monkeypatch):
    L, R = _lr()
    for k in ("UNET_UPB_TILE", "UNET_PW_WIDE", "UNET_PW_XD", "UNET_PW_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    N, Hs, Ws, C, Ci = case
    H, W = 2 * Hs, 2 * Ws
    d_up0, dgw0, w, dx0 = _inputs(prec, N, Hs, Ws, C, Ci, 11)
    wt = R.pack_weight(w, _prec(R, prec), transpose=True)
    sh, sw = R.up_scale(Hs, H), R.up_scale(Ws, W)
    for accum in (0, 1):
        # the two launches: d_up += W_g^T dgw on the 1x1 MFMA kernel, then the adjoint
        d_ref = Guarded((N, H, W, C), torch.float32, d_up0)
        x_ref = Guarded((N, H, W, Ci), DT[prec], dgw0)
        o_ref = Guarded((N, Hs, Ws, C), torch.float32, dx0)
        d = _dgrad_desc(L, R, prec, N, H, W, C, Ci, x_ref.t, wt, d_ref.t)
        ws = L.attach_workspace(d, DEV)
        assert R.conv_kernel_name(d).startswith("pw_conv_kernel"), R.conv_kernel_name(d)
        L.call("unet_conv", d, R.stream())
        L.call("unet_upsample_bwd", N, C, Hs, Ws, H, W, 0, 0, H, W, sh, sw, R.vp(d_ref.t), R.vp(o_ref.t), accum, R.stream())
        torch.cuda.synchronize()
        # the fused call
        d_fu = Guarded((N, H, W, C), torch.float32, d_up0)
        x_fu = Guarded((N, H, W, Ci), DT[prec], dgw0)
        o_fu = Guarded((N, Hs, Ws, C), torch.float32, dx0)
        _fused(L, R, prec, N, Hs, Ws, C, Ci, d_fu.t, x_fu.t, wt, o_fu.t, accum)
        assert torch.isfinite(o_ref.t).all()
        assert torch.equal(o_fu.t, o_ref.t), (accum, float((o_fu.t - o_ref.t).abs().max()))
        for gd in (d_ref, x_ref, o_ref, d_fu, x_fu, o_fu):
            assert gd.intact()
        assert torch.equal(d_fu.t, d_up0) and torch.equal(x_fu.t, dgw0)      # the fused call writes dx only
        assert torch.equal(x_ref.t, dgw0)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("geo", [(2, 5, 7), (1, 9, 20)], ids=lambda g: "x".join(map(str, g)))
def test_small_maps_against_fp64(geo, accum, prec, monkeypatch):
    L, R = _lr()
    monkeypatch.delenv("UNET_UPB_TILE", raising=False)
    N, Hs, Ws = geo
    C, Ci = 64, 32
    H, W = 2 * Hs, 2 * Ws
    d_up0, dgw0, w, dx0 = _inputs(prec, N, Hs, Ws, C, Ci, 12)
    wt = R.pack_weight(w, _prec(R, prec), transpose=True)
    d_fu = Guarded((N, H, W, C), torch.float32, d_up0)
    x_fu = Guarded((N, H, W, Ci), DT[prec], dgw0)
    o_fu = Guarded((N, Hs, Ws, C), torch.float32, dx0)
    _fused(L, R, prec, N, Hs, Ws, C, Ci, d_fu.t, x_fu.t, wt, o_fu.t, accum)
    for gd in (d_fu, x_fu, o_fu):
        assert gd.intact()
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


def _step(model, x, t, env, seen):
    from unet._hip import lib as L
    from unet.utils.loss import DiceBCELoss
    keys = ("UNET_NO_GUP_FUSE", "UNET_UPB_TILE", "UNET_PW_WIDE")
    old = {k: os.environ.get(k) for k in keys}
    orig = L.call

    def rec(name, *args):
        seen.append(name)
        return orig(name, *args)

    L.call = rec
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
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("size", [128, 98])
def test_model_backward_bit_identical(prec, size):
    """base 64 at 2 x 128^2: the top gate (64 -> 32 channels at 128^2, 32768 pixels) is the level whose W_g dgrad
    runs on the 1x1 MFMA kernel, so it alone takes the fused call; the levels below (<= 8192 pixels) keep the two
    launches.  At 98^2 the top level still fuses (19208 pixels); 49 -> 24 -> 12 -> 6 leaves padded levels below."""
    from unet.models import AttentionUNet
    torch.manual_seed(3)
    m = AttentionUNet(1, 2, base_features=64).cuda().train()
    m.hip_precision = prec
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 1, size, size, generator=g) * 2 - 1).cuda()
    t = (torch.rand(2, size, size, generator=g) < 0.1).long().cuda()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    seen0, seen1 = [], []
    out0, g0 = _step(m, x, t, {}, seen0)
    m.load_state_dict(state)   # the same BN running statistics going in
    out1, g1 = _step(m, x, t, {"UNET_NO_GUP_FUSE": "1"}, seen1)
    n0, n1 = seen0.count("unet_upsample_bwd_pw"), seen1.count("unet_upsample_bwd_pw")
    assert n1 == 0
    assert n0 == (0 if prec == "fp32" else 1), n0
    # the fused call stands for one adjoint and one 1x1 dgrad of the other run
    assert seen0.count("unet_upsample_bwd") == seen1.count("unet_upsample_bwd") - n0
    assert seen0.count("unet_conv") == seen1.count("unet_conv") - n0
    assert torch.equal(out0, out1)
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff
