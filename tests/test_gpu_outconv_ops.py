"""GPU op-level numerics of OutConv (1x1 conv + bias over a BN + ReLU source, csrc/misc.hip): the forward, the
backward and the backward fused with the BatchNorm backward of its input, through the C-ABI, against the fp64
references of tests/ref_ops.py.  Output buffers are filled with NaN (or a known value where the call accumulates)
before the launch and must come back finite.  The ReLU masks are exact: the kernels evaluate the pre-activation as
one fmaf(y, scale, shift), whose sign is the exact value's.  Gates: see tests/test_gpu_bn_gate_ops.py."""

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PRECS = ["bf16", "fp16", "fp32"]
NAN = float("nan")
ERR_UNSUPPORTED = 1002      # UNET_ERR_UNSUPPORTED, include/unet_hip.h


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _code(prec):
    _, R = _lr()
    return R._PRECISIONS[prec].code


def _nan(*shape, dt=torch.float32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _operands(prec, N, H, W, C, K):
    y = (torch.randn(N, H, W, C, device=DEV) * 1.5 + 0.3).to(DT[prec])
    sign = torch.where(torch.rand(C, device=DEV) < 0.25, -1.0, 1.0)
    scale, shift = (torch.rand(C, device=DEV) + 0.5) * sign, torch.randn(C, device=DEV) * 0.4
    w, b = torch.randn(K, C, device=DEV) * 0.1, torch.randn(K, device=DEV)
    dl = torch.randn(N, K, H, W, device=DEV)
    return y, scale, shift, w, b, dl


GEOS = [(1, 1, 1), (2, 7, 9), (3, 37, 50)]     # N > 1 with odd H·W: the pixel -> (n, hw) split matters
# K = 2 with C/8 a power of two <= 64: the vec kernel (G = 1, 8, 64); everything else: the shared-memory kernel
FWD_CK = [(8, 2), (64, 2), (512, 2), (1024, 2), (20, 2), (64, 1), (64, 3), (16, 8)]


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("ck", FWD_CK, ids=lambda s: f"C{s[0]}K{s[1]}")
@pytest.mark.parametrize("prec", PRECS)
def test_outconv_fwd(prec, ck, geo):
    """unet_outconv_fwd: logits [N,K,H,W] = b + W·relu?(y·scale + shift), with and without the ReLU and with the
    affine absent (both NULL), gated at 2e-5·(|b_k| + Σ_c|w·a|)."""
    L, R = _lr()
    (C, K), (N, H, W) = ck, geo
    torch.manual_seed(51)
    y, scale, shift, w, b, _ = _operands(prec, N, H, W, C, K)
    for relu, affine in ((1, True), (0, True), (1, False), (0, False)):
        sc, sf = (scale, shift) if affine else (None, None)
        out = _nan(N, K, H, W)
        L.call("unet_outconv_fwd", _code(prec), N, H, W, C, K, R.vp(y), R.vp(sc), R.vp(sf), relu, R.vp(w), R.vp(b),
               R.vp(out), R.stream())
        torch.cuda.synchronize()
        ref = RO.outconv_fwd(y, sc, sf, relu, w, b)
        assert torch.isfinite(out).all(), (relu, affine)
        err, tol = (out.double() - ref.logits).abs(), 2e-5 * ref.abs_terms
        assert (err <= tol).all(), (relu, affine, float((err - tol).max()))


def test_outconv_fwd_refuses_nine_classes():
    L, R = _lr()
    torch.manual_seed(52)
    y, scale, shift, w, b, _ = _operands("bf16", 1, 4, 4, 16, 9)
    out = _nan(1, 9, 4, 4)
    rc = L.load().unet_outconv_fwd(L.BF16, 1, 4, 4, 16, 9, R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(w), R.vp(b),
                                   R.vp(out), R.stream())
    torch.cuda.synchronize()
    assert rc == ERR_UNSUPPORTED and torch.isnan(out).all()


# K = 2 with 16-bit operands and C/8 a power of two <= 256: the vec kernel (G = 2, 8, 256); K = 3, C = 20 and
# every fp32 run: the per-channel kernel
BWD_CK = [(16, 2), (64, 2), (2048, 2), (64, 3), (20, 3)]


@pytest.mark.parametrize("geo", [(1, 37, 50), (2, 7, 9)], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("ck", BWD_CK, ids=lambda s: f"C{s[0]}K{s[1]}")
@pytest.mark.parametrize("prec", PRECS)
def test_outconv_bwd(prec, ck, geo):
    """unet_outconv_bwd + unet_outconv_bwd_finalize: da = W^T dl (stored / accumulated), dW, db against fp64, with
    the gates of test_gpu_ops.py::test_outconv_bwd_vec."""
    L, R = _lr()
    (C, K), (N, H, W) = ck, geo
    torch.manual_seed(53)
    y, scale, shift, w, _, dl = _operands(prec, N, H, W, C, K)
    rows = L.load().unet_outconv_rows(N * H * W)
    old = torch.randn(N, H, W, C, device=DEV)
    for relu, accum in ((1, 0), (0, 1), (1, 1), (0, 0)):
        part = _nan(rows, K + 1, C)
        da = old.clone() if accum else _nan(N, H, W, C)
        L.call("unet_outconv_bwd", _code(prec), N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), relu, R.vp(w), R.vp(dl),
               R.vp(da), accum, R.vp(part), R.stream())
        dw, db = (torch.full((K, C), 3.0, device=DEV), torch.full((K,), -2.0, device=DEV)) if accum else (_nan(K, C), _nan(K))
        L.call("unet_outconv_bwd_finalize", R.vp(part), rows, C, K, R.vp(dw), R.vp(db), accum, R.stream())
        torch.cuda.synchronize()
        ref = RO.outconv_bwd(y, scale, shift, relu, w, dl)
        for t in (da, dw, db):
            assert torch.isfinite(t).all(), (relu, accum)
        got_da = da.double() - (old.double() if accum else 0)
        assert (got_da - ref.da).abs().max() <= 1e-5 * (1 + ref.da.abs().max()), (relu, accum)
        assert ((dw.double() - 3.0 * accum) - ref.dw).abs().max() <= 1e-4 * (1 + ref.dw.abs().max()), (relu, accum)
        assert ((db.double() + 2.0 * accum) - ref.db).abs().max() <= 1e-4 * (1 + ref.db.abs().max()), (relu, accum)


@pytest.mark.parametrize("geo", [(1, 3, 5), (2, 37, 50)], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("C", [8, 64, 2048])
@pytest.mark.parametrize("prec", PRECS)
def test_outconv_bwd_bn_fused(prec, C, geo):
    """unet_outconv_bwd_bn + unet_bn_bwd_finalize + unet_bn_bwd_apply_oc (n_classes = 2): OutConv's dW, db, the
    BatchNorm-backward sums Σg_m, Σg_m·x̂ of g = W^T dl (never stored) and dy, against fp64.  dy is compared with the
    reference evaluated on the coefficients the apply kernel was handed (the finalize's output, itself gated: A at
    rtol 1e-6, B and Cc at what the partial-sum gate allows, A·invstd·δ(Σg·x̂)/M and A·δ(Σg)/M + |mean|·δB).
    Changed scale (fp32 dy only): g = w_0·dl_0 + w_1·dl_1 is recomputed here and its two terms may cancel, so
    1e-5·(|A·g| + |B·y| + |Cc|) is missed by fp32 itself: plain fp32 torch against fp64 on these inputs reaches
    1.95e-5 of that scale (C = 2048, 2x37x50, ReLU on; 8.7e-6 at C = 64, 7.4e-6 at C = 8).  With A·g's term expanded
    to |A|·Σ_k|w_k·dl_k| (ref_ops.outconv_bn_apply) fp32 torch stays at 2.4e-7 of the scale, and the 1e-5 holds."""
    L, R = _lr()
    N, H, W = geo
    K, P = 2, N * H * W
    torch.manual_seed(54)
    y, scale, shift, w, _, dl = _operands(prec, N, H, W, C, K)
    mean, invstd = torch.randn(C, device=DEV) * 0.3 + 0.3, torch.rand(C, device=DEV) * 1.5 + 0.5
    gamma = torch.randn(C, device=DEV) * 0.3 + 1.0
    rows = L.load().unet_outconv_rows(P)
    for relu in (1, 0):
        part, bpart = _nan(rows, K + 1, C), _nan(2, rows, C)
        L.call("unet_outconv_bwd_bn", _code(prec), N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), relu, R.vp(w),
               R.vp(dl), R.vp(mean), R.vp(invstd), R.vp(part), R.vp(bpart), R.stream())
        dw, db = _nan(K, C), _nan(K)
        L.call("unet_outconv_bwd_finalize", R.vp(part), rows, C, K, R.vp(dw), R.vp(db), 0, R.stream())
        dg, dbeta, coef = _nan(C), _nan(C), _nan(3, C)
        L.call("unet_bn_bwd_finalize", R.vp(bpart[0]), R.vp(bpart[1]), rows, C, P, R.vp(gamma), R.vp(mean), R.vp(invstd),
               R.vp(dg), R.vp(dbeta), 0, R.vp(coef), R.stream())
        dy = _nan(N, H, W, C, dt=DT[prec])
        L.call("unet_bn_bwd_apply_oc", _code(prec), N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), relu, R.vp(w),
               R.vp(dl), R.vp(coef), R.vp(dy), R.stream())
        torch.cuda.synchronize()
        ref = RO.outconv_bwd_bn(y, scale, shift, relu, w, dl, mean, invstd)
        assert torch.isfinite(bpart).all() and torch.isfinite(dw).all() and torch.isfinite(db).all(), relu
        assert (dw.double() - ref.dw).abs().max() <= 1e-4 * (1 + ref.dw.abs().max()), relu
        assert (db.double() - ref.db).abs().max() <= 1e-4 * (1 + ref.db.abs().max()), relu
        got = bpart.double().sum(1)
        RO.check_sums(got[0], ref.bn.sum_g, ref.bn.abs_g, ("Σg", relu))
        RO.check_sums(got[1], ref.bn.sum_gx, ref.bn.abs_gx, ("Σg·x̂", relu))
        RO.check_sums(dbeta, ref.bn.sum_g, ref.bn.abs_g, ("dbeta", relu))
        RO.check_sums(dg, ref.bn.sum_gx, ref.bn.abs_gx, ("dgamma", relu))
        rc = RO.bn_bwd_coef(ref.bn.sum_g, ref.bn.sum_gx, P, gamma, mean, invstd)
        A = rc.coef[0].abs()
        dB = A * invstd.double() * (2e-5 * ref.bn.abs_gx + 1e-6) / P
        RO.check_fin(coef[0], rc.coef[0], ("coef A", relu))
        assert ((coef[1].double() - rc.coef[1]).abs() <= dB + 1e-6 * rc.coef[1].abs()).all(), ("coef B", relu)
        dC = A * (2e-5 * ref.bn.abs_g + 1e-6) / P + mean.double().abs() * dB + 1e-6 * rc.abs_cc
        assert ((coef[2].double() - rc.coef[2]).abs() <= dC).all(), ("coef Cc", relu)
        ra = RO.outconv_bn_apply(y, scale, shift, relu, w, dl, coef)
        RO.check_elem(dy, ra.dy, ra.abs_terms, prec, ("dy", relu))


@pytest.mark.parametrize("ck", [(64, 3), (12, 2)], ids=lambda s: f"C{s[0]}K{s[1]}")
def test_outconv_bwd_bn_refuses(ck):
    """the fused form serves n_classes == 2 with C % 8 == 0, C/8 a power of two: anything else is refused with
    UNET_ERR_UNSUPPORTED before a launch (both entry points)"""
    L, R = _lr()
    C, K = ck
    N, H, W = 1, 4, 6
    torch.manual_seed(55)
    y, scale, shift, w, _, dl = _operands("bf16", N, H, W, C, K)
    mean, invstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    rows = L.load().unet_outconv_rows(N * H * W)
    part, bpart, dy = _nan(rows, K + 1, C), _nan(2, rows, C), _nan(N, H, W, C, dt=torch.bfloat16)
    coef = torch.ones(3, C, device=DEV)
    rc1 = L.load().unet_outconv_bwd_bn(L.BF16, N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(w), R.vp(dl),
                                       R.vp(mean), R.vp(invstd), R.vp(part), R.vp(bpart), R.stream())
    rc2 = L.load().unet_bn_bwd_apply_oc(L.BF16, N, H, W, C, K, R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(w), R.vp(dl),
                                        R.vp(coef), R.vp(dy), R.stream())
    torch.cuda.synchronize()
    assert rc1 == ERR_UNSUPPORTED and rc2 == ERR_UNSUPPORTED
    assert torch.isnan(part).all() and torch.isnan(bpart).all() and torch.isnan(dy).all()
