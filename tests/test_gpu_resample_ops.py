"""GPU op-level numerics of the resampling kernels of csrc/misc.hip — unet_resize_nchw / unet_resize_nchw_bwd (the
deep-supervision heads), unet_upsample_bwd (all four kernels, each case asserted to reach the kernel it is meant
for) and unet_convt_bwd_prep — against the fp64 references of tests/ref_ops.py (F.interpolate, autograd and a
selection; proved against dense tap matrices, pixel_unshuffle and ConvTranspose2d's autograd in
tests/test_ref_ops_cpu.py).  Outputs are NaN-filled before a storing launch and 1.5-filled before an accumulating one.

Bounds, all a priori:
  resize forward    2^-24·(8·Σ_taps w|a| + 4·in_size·max_taps|a|), the form tests/test_gpu_materialize.py derives (the fp32
                    source coordinate is a rounding or two away from exact: a weight error <= 2^-23·in_size on a
                    corner spread <= 2·max|a|; a few roundings in the blend), in_size = max(Hi, Wi)
  resize backward   the same form summed over the destination taps of a source element:
                    2^-24·(8·Σ w|dy| + 4·in_size·Σ_taps|dy|) (+ 2^-23·|old| when it accumulates)
  upsample_bwd      1e-5·(1 + max|ref|), the gate of test_gpu_ops.test_upsample_bwd
  convt prep        the space-to-depth map bit for bit; the bias sums 2^-20·Σ|terms| (see test_convt_bwd_prep)"""

import math

import numpy as np
import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
ERR_ARG = 1001
U24 = 2.0 ** -24
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


# ---- unet_resize_nchw / unet_resize_nchw_bwd ---------------------------------------------------------

# (Hi, Wi, Ho, Wo): x2, x4, x8, the attention gate's odd ratio, identity, a source of size 1 in one axis (scale 0),
# an output of size 1, a downsample
RESIZE_GEO = [(8, 12, 16, 24), (8, 12, 32, 48), (8, 12, 64, 96), (7, 9, 15, 17), (9, 11, 9, 11), (1, 5, 8, 10),
              (5, 7, 1, 1), (9, 11, 4, 5)]


def _resize_fwd(x, Ho, Wo):
    L, R = _lr()
    NC, Hi, Wi = x.shape
    y = torch.full((NC, Ho, Wo), NAN, device=DEV)
    L.call("unet_resize_nchw", NC, Hi, Wi, Ho, Wo, R.up_scale(Hi, Ho), R.up_scale(Wi, Wo), R.vp(x), R.vp(y), R.stream())
    torch.cuda.synchronize()
    t = RO.resize_terms(x.unsqueeze(0), Ho, Wo)
    tol = U24 * (8 * t.sum_w[0] + 4 * max(Hi, Wi) * t.max_a[0])
    return y, RO.resize(x.unsqueeze(0), Ho, Wo)[0], tol


def _resize_bwd(dy, Hi, Wi, accum):
    L, R = _lr()
    NC, Ho, Wo = dy.shape
    dx = torch.full((NC, Hi, Wi), 1.5 if accum else NAN, device=DEV)
    L.call("unet_resize_nchw_bwd", NC, Hi, Wi, Ho, Wo, R.up_scale(Hi, Ho), R.up_scale(Wi, Wo), R.vp(dy), R.vp(dx), accum,
           R.stream())
    torch.cuda.synchronize()
    t = RO.resize_bwd_terms(dy.unsqueeze(0), Hi, Wi)
    tol = U24 * (8 * t.sum_w[0] + 4 * max(Hi, Wi) * t.sum_a[0]) + (2 * U24 * 1.5 if accum else 0.0)
    old = torch.full((1, NC, Hi, Wi), 1.5, device=DEV) if accum else None
    return dx, RO.resize_bwd(dy.unsqueeze(0), Hi, Wi, old)[0], tol


def _within(got, ref, tol, what):
    assert torch.isfinite(got).all(), (what, "not finite")
    err = (got.double() - ref).abs()
    assert (err <= tol).all(), (what,) + RO._worst(err, tol)


@pytest.mark.parametrize("NC", [1, 6])
@pytest.mark.parametrize("geo", RESIZE_GEO, ids=lambda g: "x".join(map(str, g)))
def test_resize_nchw(geo, NC):
    """forward against F.interpolate, backward (storing and accumulating) against its autograd adjoint, and
    ⟨resize(x), dy⟩ = ⟨x, resize_bwd(dy)⟩ on the kernels' outputs, in fp64, to the sum of the two bounds"""
    Hi, Wi, Ho, Wo = geo
    torch.manual_seed(41)
    x, dy = torch.randn(NC, Hi, Wi, device=DEV), torch.randn(NC, Ho, Wo, device=DEV)
    y, ref, tol = _resize_fwd(x, Ho, Wo)
    _within(y, ref, tol, "resize")
    for accum in (0, 1):
        dx, refb, tolb = _resize_bwd(dy, Hi, Wi, accum)
        _within(dx, refb, tolb, ("resize_bwd", accum))
    lhs, rhs = float((y.double() * dy.double()).sum()), float((x.double() * (dx.double() - 1.5)).sum())
    gate = float((tol * dy.double().abs()).sum() + (tolb * x.double().abs()).sum())
    assert abs(lhs - rhs) <= gate, (lhs, rhs, gate)


def test_resize_nchw_beyond_the_block_cap():
    """6 x (75, 75) -> (600, 600) is 2160000 > 8192·256 output elements for the forward; the backward of the
    matching downsample writes as many: both grid-stride loops run a second trip"""
    torch.manual_seed(42)
    NC = 6
    assert NC * 600 * 600 > 8192 * 256
    y, ref, tol = _resize_fwd(torch.randn(NC, 75, 75, device=DEV), 600, 600)
    _within(y, ref, tol, "resize")
    for accum in (0, 1):
        dx, refb, tolb = _resize_bwd(torch.randn(NC, 75, 75, device=DEV), 600, 600, accum)
        _within(dx, refb, tolb, ("resize_bwd", accum))


# ---- unet_upsample_bwd -----------------------------------------------------------------------------------

UPB_J, UPB_VMAX = 16, 56


def _upb_kernel(C, up_h, up_w, sh, sw, tile_env=True):
    """the kernel unet_upsample_bwd launches (csrc/misc.hip): the window test in fp32, as the host forms it"""
    def span(sc, up):
        return int(math.floor(np.float32(2.0) / np.float32(sc))) + 3 if sc > 0 else up + 8
    if C % 4:
        return "scalar"
    if span(sh, up_h) <= 8 and span(sw, up_w) <= 8:
        vspan = int(math.floor(np.float32(UPB_J + 1) / np.float32(sw))) + 4
        return "tile" if tile_env and vspan <= UPB_VMAX else "4w"
    return "bwd4"


# (N, C, Hs, Ws, up_h, up_w, pad_t, pad_l, Hp, Wp, kernel)
UPB_CASES = [
    (2, 1, 7, 9, 14, 18, 1, 2, 17, 22, "scalar"),          # C % 4 != 0
    (1, 6, 7, 9, 15, 17, 0, 0, 15, 17, "scalar"),
    (1, 6, 1, 5, 8, 10, 2, 0, 11, 10, "scalar"),           # a source row of its own: scale 0
    (2, 8, 5, 5, 16, 16, 0, 1, 16, 18, "bwd4"),            # ratio 5 -> 16: a window wider than 8
    (1, 8, 1, 6, 4, 12, 1, 0, 6, 12, "bwd4"),              # Hs = 1
    (2, 4, 6, 1, 12, 3, 0, 2, 12, 6, "bwd4"),              # Ws = 1
    (1, 8, 7, 9, 15, 17, 0, 0, 15, 17, "tile"),            # the gate's ratio, no pads
    (2, 16, 7, 9, 14, 18, 1, 2, 18, 20, "tile"),           # x2, pads 1 / 3 and 2 / 0
    (1, 80, 5, 40, 10, 80, 0, 3, 11, 83, "tile"),          # two channel tiles (the second partial), three column tiles
]


def _upb_run(case, accum, g):
    L, R = _lr()
    N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, _ = case
    dx = torch.full((N, Hs, Ws, C), 1.5 if accum else NAN, device=DEV)
    L.call("unet_upsample_bwd", N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, R.up_scale(Hs, up_h), R.up_scale(Ws, up_w),
           R.vp(g), R.vp(dx), accum, R.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    return dx.double() - (1.5 if accum else 0.0)


def _upb_input(case):
    N, C, Hs, Ws, up_h, up_w, pt, pl, Hp, Wp, _ = case
    torch.manual_seed(9)
    g = torch.randn(N, Hp, Wp, C, device=DEV)
    return g, RO.upsample_bwd(g, Hs, Ws, up_h, up_w, pt, pl)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("case", UPB_CASES, ids=lambda c: "x".join(map(str, c)))
def test_upsample_bwd_kernels(case, accum, monkeypatch):
    """the scalar kernel, upsample_bwd4_kernel and the tiled kernel, each on geometry that reaches it (asserted
    through the mirror of the host's dispatch), against the fp64 adjoint of interpolate + pad"""
    L, R = _lr()
    monkeypatch.delenv("UNET_UPB_TILE", raising=False)
    N, C, Hs, Ws, up_h, up_w = case[:6]
    assert _upb_kernel(C, up_h, up_w, R.up_scale(Hs, up_h), R.up_scale(Ws, up_w)) == case[-1]
    g, ref = _upb_input(case)
    got = _upb_run(case, accum, g)
    err = float((got - ref).abs().max())
    assert err <= 1e-5 * (1 + float(ref.abs().max())), err


def _x2(N, h, w, Hp, Wp, C):
    return (N, C, h, w, 2 * h, 2 * w, (Hp - 2 * h) // 2, (Wp - 2 * w) // 2, Hp, Wp, "tile")


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("case", [_x2(2, 7, 9, 14, 18, 8), _x2(1, 13, 37, 27, 75, 48), UPB_CASES[6], UPB_CASES[7]],
                         ids=lambda c: "x".join(map(str, c)))
def test_upsample_bwd_4w_and_tiled_agree(case, accum, monkeypatch):
    """upsample_bwd4w_kernel (UNET_UPB_TILE=0) against the fp64 adjoint, and against the tiled kernel on the same
    input: both within 1e-5·(1 + max|ref|) of the reference and of each other"""
    L, R = _lr()
    N, C, Hs, Ws, up_h, up_w = case[:6]
    sh, sw = R.up_scale(Hs, up_h), R.up_scale(Ws, up_w)
    assert _upb_kernel(C, up_h, up_w, sh, sw, True) == "tile" and _upb_kernel(C, up_h, up_w, sh, sw, False) == "4w"
    g, ref = _upb_input(case)
    gate = 1e-5 * (1 + float(ref.abs().max()))
    monkeypatch.setenv("UNET_UPB_TILE", "0")
    w4 = _upb_run(case, accum, g)
    monkeypatch.setenv("UNET_UPB_TILE", "1")
    tiled = _upb_run(case, accum, g)
    assert float((w4 - ref).abs().max()) <= gate and float((tiled - ref).abs().max()) <= gate
    assert float((w4 - tiled).abs().max()) <= gate


# ---- unet_convt_bwd_prep -----------------------------------------------------------------------------------

def _prep(prec, N, h, w, Ct, Hp, Wp, pt, pl, d_up, rows):
    L, R = _lr()
    out = torch.full((N, h, w, 4 * Ct), NAN, dtype=DT[prec], device=DEV)
    part = torch.full((rows, Ct), NAN, device=DEV)
    rc = L.load().unet_convt_bwd_prep(R._PRECISIONS[prec].code, N, h, w, Ct, Hp, Wp, pt, pl, R.vp(d_up), R.vp(out),
                                      R.vp(part), R.stream())
    torch.cuda.synchronize()
    return rc, out, part


@pytest.mark.parametrize("Ct", [1, 3, 16, 96, 256, 300, 1024])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_convt_bwd_prep(prec, Ct):
    """dy_s2d equals the round-to-nearest cast of the addressed d_up element bit for bit (d_up is random in the
    padding too, so a wrong offset shows); the partial rows, summed by unet_colsum, are the bias gradient.
    Ct = 1, 3, 96 (pixel lanes, idle ones for 3 and 96), 256, 300 and 1024 (channel chunks k >= 1); 1, 70 and 1025
    pixels (2 partial rows); pads (0, 0) and (1, 2) in a frame larger than needed.
    Bias gate 2^-20·Σ|terms|, derived: a lane adds at most 1024 pixels x 4 values one after the other in fp32, then
    a tree over the pixel lanes and an fp64 column sum.  Add i rounds by <= 2^-24·|s_i|; for the zero-mean d_up
    drawn here |s_i| ~ sqrt(i)·σ, so even with every rounding in one direction the error stays below
    2^-24·(2/3)·n^1.5·σ against Σ|terms| ~ 0.8·n·σ: 2^-24·0.84·sqrt(n) <= 2^-24·54 at n = 4096, and for roundings of
    random sign about 2^-24.  2^-20 = 16·2^-24 lies between the two; a skipped chunk, lane, row or tap leaves out a
    fixed share of the terms and cannot hide under it."""
    L, R = _lr()
    dt = DT[prec]
    for N, h, w in ((1, 1, 1), (2, 5, 7), (1, 25, 41)):
        rows = L.load().unet_convt_bwd_rows(N * h * w)
        assert rows == (2 if N * h * w > 1024 else 1)
        for pt, pl in ((0, 0), (1, 2)):
            Hp, Wp = 2 * h + pt + 1, 2 * w + pl + 2
            torch.manual_seed(Ct + h)
            d_up = torch.randn(N, Hp, Wp, Ct, device=DEV)
            rc, out, part = _prep(prec, N, h, w, Ct, Hp, Wp, pt, pl, d_up, rows)
            assert rc == 0
            ref = RO.convt_bwd_prep(d_up, h, w, pt, pl)
            want = ref.s2d.float().to(dt)
            bits = torch.int32 if dt == torch.float32 else torch.int16
            assert torch.equal(out.view(bits), want.view(bits)), (N, h, w, pt, pl)
            assert torch.isfinite(part).all()
            bias = torch.full((Ct,), NAN, device=DEV)
            L.call("unet_colsum", R.vp(part), rows, Ct, R.vp(bias), 0, R.stream())
            torch.cuda.synchronize()
            err, tol = (bias.double() - ref.bias).abs(), 2.0 ** -20 * ref.abs_bias
            assert (err <= tol).all(), (N, h, w, pt, pl) + RO._worst(err, tol)


@pytest.mark.parametrize("bad", ["Ct", "pad_t", "pad_l", "Hp", "Wp"])
def test_convt_bwd_prep_refusals(bad):
    """Ct = 1025, a negative pad and pad + 2h > Hp (pad + 2w > Wp): UNET_ERR_ARG, nothing written"""
    N, h, w, Ct, pt, pl = 1, 3, 4, 8, 1, 1
    Hp, Wp = 2 * h + pt, 2 * w + pl
    d_up = torch.randn(N, Hp + 2, Wp + 2, 1025, device=DEV)
    if bad == "Ct":
        Ct = 1025
    elif bad == "pad_t":
        pt = -1
    elif bad == "pad_l":
        pl = -1
    elif bad == "Hp":
        Hp -= 1
    else:
        Wp -= 1
    rc, out, part = _prep("bf16", N, h, w, Ct, Hp, Wp, pt, pl, d_up, 1)
    assert rc == ERR_ARG
    assert bool(out.isnan().all()) and bool(part.isnan().all())
