"""GPU op-level numerics of the multi-class OutConv (9..16 classes on MFMA, csrc/outconv_mc.hip) through the C-ABI,
against the fp64 references of tests/ref_ops.py.  Operands as test_gpu_outconv_ops.py draws them (negative BN scales
on a quarter of the channels, biased y), with w already rounded to the operand type so the reference and the kernel
see the same weights.  Output buffers are NaN (or known values where the call accumulates) and must come back
finite.  Gates: one operand rounding per activation term (EPS16: a rounding plus a flip) on top of the fp32 gate
2e-5; the weight gradient has two rounded operands."""

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PRECS = ["bf16", "fp16", "fp32"]
NAN = float("nan")
ERR_UNSUPPORTED = 1002      # UNET_ERR_UNSUPPORTED, include/unet_hip.h
# one 16-channel sub-chunk; the full tile; a C % 32 != 0 tail with odd K; a deep-supervision head width
CKS = [(16, 9), (64, 16), (40, 13), (512, 12)]
# a single pixel; odd H·W with tiles straddling images; several row tiles
GEOS = [(1, 1, 1), (2, 7, 9), (3, 37, 50)]
ids_ck, ids_geo = (lambda s: f"C{s[0]}K{s[1]}"), (lambda g: "x".join(map(str, g)))


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _code(prec):
    return _lr()[1]._PRECISIONS[prec].code


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _tol(prec, n_rounded=1):
    return n_rounded * RO.EPS16.get(prec, 0.0) + 2e-5


def _operands(prec, N, H, W, C, K):
    y = (torch.randn(N, H, W, C, device=DEV) * 1.5 + 0.3).to(DT[prec])
    sign = torch.where(torch.rand(C, device=DEV) < 0.25, -1.0, 1.0)
    scale, shift = (torch.rand(C, device=DEV) + 0.5) * sign, torch.randn(C, device=DEV) * 0.4
    w, b = (torch.randn(K, C, device=DEV) * 0.1).to(DT[prec]).float(), torch.randn(K, device=DEV)
    dl = torch.randn(N, K, H, W, device=DEV)
    return y, scale, shift, w, b, dl


@pytest.mark.parametrize("geo", GEOS, ids=ids_geo)
@pytest.mark.parametrize("ck", CKS, ids=ids_ck)
@pytest.mark.parametrize("prec", PRECS)
def test_outconv_mc_fwd(prec, ck, geo):
    """unet_outconv_mc_fwd: logits = b + W·relu?(y·scale + shift) with and without the ReLU and the affine, gated at
    (EPS16 + 2e-5)·(|b_k| + Σ_c|w·a|) (2e-5 in fp32)."""
    L, R = _lr()
    (C, K), (N, H, W) = ck, geo
    torch.manual_seed(61)
    y, scale, shift, w, b, _ = _operands(prec, N, H, W, C, K)
    for relu, affine in ((1, True), (0, True), (1, False), (0, False)):
        sc, sf = (scale, shift) if affine else (None, None)
        out = _nan(N, K, H, W)
        L.call("unet_outconv_mc_fwd", _code(prec), N, H, W, C, K, R.vp(y), R.vp(sc), R.vp(sf), relu, R.vp(w), R.vp(b),
               R.vp(out), R.stream())
        torch.cuda.synchronize()
        ref = RO.outconv_fwd(y, sc, sf, relu, w, b)
        assert torch.isfinite(out).all(), (relu, affine)
        err, tol = (out.double() - ref.logits).abs(), _tol(prec) * ref.abs_terms
        assert (err <= tol).all(), (relu, affine, float((err - tol).max()))


def _bwd(prec, C, K, N, H, W, relu, accum, ops, old):
    L, R = _lr()
    y, scale, shift, w, _, dl = ops
    rows = L.load().unet_outconv_rows(N * H * W)
    part = _nan(rows, K + 1, C)
    da = old.clone() if accum else _nan(N, H, W, C)
    L.call("unet_outconv_mc_bwd", _code(prec), N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), relu, R.vp(w),
           R.vp(dl), R.vp(da), accum, R.vp(part), R.stream())
    dw, db = _nan(K, C), _nan(K)
    L.call("unet_outconv_bwd_finalize", R.vp(part), rows, C, K, R.vp(dw), R.vp(db), 0, R.stream())
    torch.cuda.synchronize()
    return da, dw, db


@pytest.mark.parametrize("geo", GEOS, ids=ids_geo)
@pytest.mark.parametrize("ck", CKS, ids=ids_ck)
@pytest.mark.parametrize("prec", PRECS)
def test_outconv_mc_bwd(prec, ck, geo):
    """unet_outconv_mc_bwd + unet_outconv_bwd_finalize against fp64: da = Wᵀ·dl (stored / accumulated) within
    tol·Σ_k|w_k·dl_k| (dl is the rounded operand), dW within (2·EPS16 + 2e-5)·Σ_px|dl·a| (two rounded operands),
    db = Σ dl of the unrounded gradient within check_sums' 2e-5·Σ|dl|."""
    (C, K), (N, H, W) = ck, geo
    torch.manual_seed(63)
    ops = _operands(prec, N, H, W, C, K)
    y, scale, shift, w, _, dl = ops
    old = torch.randn(N, H, W, C, device=DEV)
    abs_da = torch.einsum("nkhw,kc->nhwc", dl.double().abs(), w.double().abs())
    for relu, accum in ((1, 0), (0, 1), (1, 1), (0, 0)):
        da, dw, db = _bwd(prec, C, K, N, H, W, relu, accum, ops, old)
        ref = RO.outconv_bwd(y, scale, shift, relu, w, dl)
        for t in (da, dw, db):
            assert torch.isfinite(t).all(), (relu, accum)
        err = (da.double() - (old.double() if accum else 0) - ref.da).abs()
        tol = _tol(prec) * abs_da
        assert (err <= tol).all(), ("da", relu, accum, float((err - tol).max()))
        abs_dw = torch.einsum("nkhw,nhwc->kc", dl.double().abs(), RO.act(y, scale, shift, relu).abs())
        err, tol = (dw.double() - ref.dw).abs(), _tol(prec, 2) * abs_dw
        assert (err <= tol).all(), ("dW", relu, accum, float((err - tol).max()))
        RO.check_sums(db, ref.db, dl.double().abs().sum((0, 2, 3)), ("db", relu, accum))


def test_outconv_mc_bwd_deterministic():
    """no floating-point atomics: two runs are bit-identical"""
    C, K, N, H, W = 40, 13, 3, 37, 50
    torch.manual_seed(64)
    ops = _operands("bf16", N, H, W, C, K)
    a, b = (_bwd("bf16", C, K, N, H, W, 1, 0, ops, None) for _ in range(2))
    assert all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("ck", [(64, 17), (20, 12), (8, 9), (64, 8)], ids=ids_ck)
def test_outconv_mc_refuses(ck):
    """outside unet_outconv_mc_ok (9 <= K <= 16, C % 8 == 0, C >= 16) both entry points return
    UNET_ERR_UNSUPPORTED before a launch and leave the outputs untouched"""
    L, R = _lr()
    C, K = ck
    N, H, W = 1, 4, 6
    torch.manual_seed(65)
    y, scale, shift, w, b, dl = _operands("bf16", N, H, W, C, K)
    rows = L.load().unet_outconv_rows(N * H * W)
    out, da, part = _nan(N, K, H, W), _nan(N, H, W, C), _nan(rows, K + 1, max(C, K))
    assert L.load().unet_outconv_mc_ok(L.BF16, C, K) == 0
    rc1 = L.load().unet_outconv_mc_fwd(L.BF16, N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(w), R.vp(b),
                                       R.vp(out), R.stream())
    rc2 = L.load().unet_outconv_mc_bwd(L.BF16, N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(w), R.vp(dl),
                                       R.vp(da), 0, R.vp(part), R.stream())
    torch.cuda.synchronize()
    assert rc1 == ERR_UNSUPPORTED and rc2 == ERR_UNSUPPORTED
    assert torch.isnan(out).all() and torch.isnan(da).all() and torch.isnan(part).all()
