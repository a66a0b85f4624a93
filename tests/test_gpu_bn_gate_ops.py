"""GPU op-level numerics of the BatchNorm statistics / backward (csrc/bn.hip) and the AttentionGate passes
(csrc/gate.hip): every entry point, through the C-ABI, against the fp64 references of tests/ref_ops.py (proved
against autograd in tests/test_ref_ops_cpu.py) — never against another form of the same kernel.

Activations are drawn in the operand type, so what is left is fp32 evaluation and the output rounding.  Every
output buffer is filled with NaN (or a known value where the call accumulates) before the launch and must come
back finite, so an unwritten tail shows.  Gates (ref_ops.check_*):
  partial sums      |got − ref| <= 2e-5·Σ|terms| + 1e-6 per channel (the partial table reduced in fp64)
  finalize outputs  rtol 1e-6 (fp64 arithmetic rounded once), relative to the largest term where one cancels
  16-bit outputs    eps·|ref| + eps·1e-3·max|ref|, eps = 2^-8 (bf16) / 2^-11 (fp16); fp32: 1e-5·Σ|terms|
  p, dq             2e-5·Σ_c|term_c|;  dx: rtol 1e-6, atol 1e-6
ReLU masks: the BN kernels evaluate the pre-activation as one fmaf(y, scale, shift), whose sign is the exact
value's, so the fp64 mask is exact.  The gate kernels' g·gs + gb + x·xs + xb has an unspecified contraction; its
operands are drawn on binary grids (gate_operands) on which every partial result is exact in fp32, so the fp32
and fp64 values of a are bit-equal (asserted), zeros included."""

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PRECS = ["bf16", "fp16", "fp32"]
EPS = 1e-5
NAN = float("nan")


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _code(prec):
    _, R = _lr()
    return R._PRECISIONS[prec].code


def _nan(*shape, dt=torch.float32):
    return torch.full(shape, NAN, dtype=dt, device=DEV)


def _randn(*shape, scale=1.0, shift=0.0, dt=torch.float32):
    return (torch.randn(*shape, device=DEV) * scale + shift).to(dt)


def _rand(*shape, lo=0.5, hi=1.5):
    return torch.rand(*shape, device=DEV) * (hi - lo) + lo


# ---- unet_bn_finalize / unet_bn_eval_affine / unet_colsum ------------------------------------------------

FIN_CASES = [(1, 2048, 4 * 512 * 512), (3, 7, 100), (64, 4097, 10 ** 6), (5, 1, 1)]


def _fwd_stats(C, rows, count):
    """a [2][C][rows] table of partial (Σx, Σx²) of a plausible activation; the last channel (C > 1) has
    Σx² slightly below count·mean², so its variance comes out negative and the clamp runs"""
    mu, sd = _randn(C, 1, scale=1.5).double(), _rand(C, 1).double()
    n = count / rows
    s0 = (n * mu * (1 + 0.1 * _randn(C, rows).double())).float()
    s1 = (n * (sd * sd + mu * mu) * (1 + 0.01 * _randn(C, rows).double())).float()
    if C > 1:
        m = s0[-1].double().sum() / count
        s1[-1] = (count * m * m * (1 - 1e-4) / rows).float()
    return torch.stack([s0, s1]).contiguous()


@pytest.mark.parametrize("running", [True, False], ids=["running", "norunning"])
@pytest.mark.parametrize("momentum", [0.1, -1.0])
@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_finalize(case, momentum, running):
    """unet_bn_finalize: mean, invstd, scale, shift, the running statistics (unbiased variance; count == 1 keeps
    the biased one; momentum < 0 = cumulative average with num_batches_tracked = 3) and num_batches_tracked + 1,
    at 1 row, a few rows and 4097 rows (1024 threads: one 4-per-trip round plus a remainder)."""
    L, R = _lr()
    C, rows, count = case
    torch.manual_seed(11)
    stats = _fwd_stats(C, rows, count)
    gamma, beta = _randn(C, shift=1.0, scale=0.3), _randn(C)
    rm0, rv0 = _randn(C), _rand(C)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor([3], dtype=torch.int64, device=DEV)
    out = [_nan(C) for _ in range(4)]
    L.call("unet_bn_finalize", R.vp(stats), rows, C, count, R.vp(gamma), R.vp(beta), R.vp(rm) if running else None,
           R.vp(rv) if running else None, R.vp(nbt) if running else None, momentum, EPS, *(R.vp(t) for t in out),
           R.stream())
    torch.cuda.synchronize()
    ref = RO.bn_finalize(stats, count, gamma, beta, rm0 if running else None, rv0 if running else None,
                         3 if running else None, momentum, EPS)
    if C > 1:   # the clamp ran on the last channel
        st = stats.double()
        assert float(st[1, -1].sum() / count - (st[0, -1].sum() / count) ** 2) < 0 and float(ref.var[-1]) == 0.0
    RO.check_fin(out[0], ref.mean, "mean")
    RO.check_fin(out[1], ref.invstd, "invstd")
    RO.check_fin(out[2], ref.scale, "scale")
    RO.check_fin(out[3], ref.shift, "shift", beta.double().abs() + (ref.mean * ref.scale).abs())
    if running:
        RO.check_fin(rm, ref.running_mean, "running_mean", ref.abs_running_mean)
        RO.check_fin(rv, ref.running_var, "running_var")
        assert int(nbt) == 4 == ref.nbt
    else:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt) == 3


@pytest.mark.parametrize("with_stats", [True, False])
def test_bn_eval_affine(with_stats):
    L, R = _lr()
    C = 300      # two blocks, the second partial
    torch.manual_seed(12)
    gamma, beta, rm, rv = _randn(C, shift=1.0, scale=0.3), _randn(C), _randn(C), _rand(C, lo=0.01, hi=2.0)
    scale, shift, mean, invstd = (_nan(C) for _ in range(4))
    L.call("unet_bn_eval_affine", C, R.vp(gamma), R.vp(beta), R.vp(rm), R.vp(rv), EPS, R.vp(scale), R.vp(shift),
           R.vp(mean) if with_stats else None, R.vp(invstd) if with_stats else None, R.stream())
    torch.cuda.synchronize()
    ref = RO.bn_eval_affine(gamma, beta, rm, rv, EPS)
    RO.check_fin(scale, ref.scale, "scale")
    RO.check_fin(shift, ref.shift, "shift", beta.double().abs() + (ref.mean * ref.scale).abs())
    if with_stats:
        assert torch.equal(mean, rm)
        RO.check_fin(invstd, ref.invstd, "invstd")
    else:
        assert torch.isnan(mean).all() and torch.isnan(invstd).all()


@pytest.mark.parametrize("accum", [0, 1])
def test_colsum(accum):
    L, R = _lr()
    rows, C = 1000, 37
    torch.manual_seed(13)
    part = _randn(rows, C, scale=2.0)
    old = _randn(C, scale=5.0)
    out = old.clone() if accum else _nan(C)
    L.call("unet_colsum", R.vp(part), rows, C, R.vp(out), accum, R.stream())
    torch.cuda.synchronize()
    s = part.double().sum(0)
    RO.check_fin(out, s + old.double() * accum, "colsum", torch.maximum(s.abs(), old.double().abs() * accum))


# ---- unet_bn_bwd_reduce / _finalize / _apply ------------------------------------------------------------

# (prec, 16-bit da): da is fp32, or of the operand type in 16-bit runs
BN_TYPES = [("bf16", False), ("bf16", True), ("fp16", False), ("fp16", True), ("fp32", False)]
BN_TYPE_IDS = ["bf16-da32", "bf16-da16", "fp16-da32", "fp16-da16", "fp32"]
# vectorised form: C % 8 == 0, C/8 a power of two (R = 256/(C/8) pixel rows per block: 256, 32, 2, 1); the
# per-channel form: 1, 3, 24 (a multiple of 8, not a power of two), 100 (two channel blocks, one partial)
BN_C = [8, 64, 1024, 2048, 1, 3, 24, 100]
# + one multi-block case per form with an uneven last block / empty trailing blocks (40003 x 1024: the 2048-row cap)
BN_SHAPES = [(P, C) for C in BN_C for P in (1, 63, 4099)] + [(70001, 64), (40003, 1024), (70001, 100)]


def _bn_operands(prec, da16, P, C):
    dt = DT[prec]
    y = _randn(P, C, scale=1.5, shift=0.3, dt=dt)
    da = _randn(P, C, dt=dt if da16 else torch.float32)
    sign = torch.where(torch.rand(C, device=DEV) < 0.25, -1.0, 1.0)
    scale, shift = _rand(C) * sign, _randn(C, scale=0.4)
    mean, invstd = _randn(C, scale=0.3, shift=0.3), _rand(C, lo=0.5, hi=2.0)
    return y, da, scale, shift, mean, invstd


@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("types", BN_TYPES, ids=BN_TYPE_IDS)
def test_bn_bwd_reduce(types, shape):
    """unet_bn_bwd_reduce alone: the [2][rows][C] partial table, reduced in fp64, against Σg and Σg·x̂ of fp64
    (g = da where y·scale + shift > 0), with and without the ReLU."""
    L, R = _lr()
    prec, da16 = types
    P, C = shape
    torch.manual_seed(21)
    y, da, scale, shift, mean, invstd = _bn_operands(prec, da16, P, C)
    rows = L.load().unet_bn_bwd_reduce_rows(P, C)
    for relu in (1, 0):
        part = _nan(2, rows, C)
        L.call("unet_bn_bwd_reduce", _code(prec), _code(prec) if da16 else L.F32, P, C, R.vp(da), R.vp(y), R.vp(scale),
               R.vp(shift), relu, R.vp(mean), R.vp(invstd), R.vp(part), R.stream())
        torch.cuda.synchronize()
        assert torch.isfinite(part).all(), ("unwritten partial rows", relu, rows)
        ref = RO.bn_bwd_sums(da, y, scale, shift, relu, mean, invstd)
        got = part.double().sum(1)
        RO.check_sums(got[0], ref.sum_g, ref.abs_g, ("Σg", relu, rows))
        RO.check_sums(got[1], ref.sum_gx, ref.abs_gx, ("Σg·x̂", relu, rows))


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("count", [4 * 512 * 512, 0])
@pytest.mark.parametrize("case", [(1, 2048), (3, 7), (64, 4097), (100, 33)], ids=lambda c: "x".join(map(str, c)))
def test_bn_bwd_finalize(case, count, accum):
    """unet_bn_bwd_finalize alone on a random partial table: dγ, dβ (stored / accumulated) and coef = (A, B, Cc);
    count == 0 (eval mode) gives (γ·invstd, 0, 0); without coef the sums alone."""
    L, R = _lr()
    C, rows = case
    torch.manual_seed(22)
    part = _randn(2, rows, C, scale=3.0)
    gamma, mean, invstd = _randn(C, shift=1.0, scale=0.3), _randn(C), _rand(C, lo=0.5, hi=2.0)
    old = _randn(2, C, scale=4.0)
    ref = RO.bn_bwd_coef(part[0].double().sum(0), part[1].double().sum(0), count, gamma, mean, invstd)
    for with_coef in (True, False):
        dg, db = (old[0].clone(), old[1].clone()) if accum else (_nan(C), _nan(C))
        coef = _nan(3, C)
        L.call("unet_bn_bwd_finalize", R.vp(part[0]), R.vp(part[1]), rows, C, count, R.vp(gamma), R.vp(mean), R.vp(invstd),
               R.vp(dg), R.vp(db), accum, R.vp(coef) if with_coef else None, R.stream())
        torch.cuda.synchronize()
        # the sums are fp64, rounded once: relative to the result itself; accumulated, to the fp32 add's larger term
        o = old.double() * accum
        RO.check_fin(dg, ref.dgamma + o[0], "dgamma", torch.maximum(ref.dgamma.abs(), o[0].abs()))
        RO.check_fin(db, ref.dbeta + o[1], "dbeta", torch.maximum(ref.dbeta.abs(), o[1].abs()))
        if with_coef:
            RO.check_fin(coef[0], ref.coef[0], "coef A")
            RO.check_fin(coef[1], ref.coef[1], "coef B")
            RO.check_fin(coef[2], ref.coef[2], "coef Cc", ref.abs_cc)
            if count == 0:
                assert float(coef[1:].abs().max()) == 0.0
        else:
            assert torch.isnan(coef).all()


@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("types", BN_TYPES, ids=BN_TYPE_IDS)
def test_bn_bwd_apply(types, shape):
    """unet_bn_bwd_apply alone: dy = A·g + B·y + Cc with random coefficients, element by element."""
    L, R = _lr()
    prec, da16 = types
    P, C = shape
    torch.manual_seed(23)
    y, da, scale, shift, mean, invstd = _bn_operands(prec, da16, P, C)
    coef = torch.stack([_rand(C), _randn(C, scale=0.3), _randn(C, scale=0.2)]).contiguous()
    for relu in (1, 0):
        dy = _nan(P, C, dt=DT[prec])
        L.call("unet_bn_bwd_apply", _code(prec), _code(prec) if da16 else L.F32, P, C, R.vp(da), R.vp(y), R.vp(scale),
               R.vp(shift), relu, R.vp(coef), R.vp(dy), R.stream())
        torch.cuda.synchronize()
        g = RO.bn_bwd_sums(da, y, scale, shift, relu, mean, invstd).g
        ref = RO.bn_bwd_apply(g, y, coef)
        RO.check_elem(dy, ref.dy, ref.abs_terms, prec, ("dy", relu))


@pytest.mark.parametrize("shape", [(4099, 64), (4099, 100), (63, 8)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("types", BN_TYPES, ids=BN_TYPE_IDS)
def test_bn_bwd_chain_vs_autograd(types, shape):
    """reduce -> finalize -> apply on the batch statistics of y (taken in fp64 and handed to the kernels) against
    torch autograd of BatchNorm + ReLU in fp64 on the same y: dy, dγ, dβ.  The ReLU mask of the reference is the
    exact one of the fp32 affine the kernels are handed (an fp64 BatchNorm is a rounding away from it).
    dγ, dβ: the partial-sum gate.  dy: the element-wise gate, 16-bit eps; fp32 on the scale |A·g| + |B·y| + |Cc|.
    Measured gate (fp32 dy only): in a channel whose Σg and Σg·x̂ nearly cancel, B and Cc are small against the fp32
    noise of those sums, and 1e-5 of that scale is missed by fp32 itself: plain fp32 torch autograd against fp64
    autograd on these inputs reaches 4.79e-6 (4099x64), 7.96e-6 (4099x100) and 3.24e-7 (63x8) of the scale.  The
    gate is 4 x 7.96e-6 = 3.2e-5."""
    L, R = _lr()
    prec, da16 = types
    P, C = shape
    torch.manual_seed(24)
    y = _randn(P, C, scale=1.5, shift=0.3, dt=DT[prec])
    da = _randn(P, C, dt=DT[prec] if da16 else torch.float32)
    gamma = _randn(C, shift=1.0, scale=0.3)
    beta = _randn(C, scale=0.4)
    yd = y.double()
    mean64, var64 = yd.mean(0), yd.var(0, unbiased=False)
    inv64 = 1.0 / torch.sqrt(var64 + EPS)
    mean, invstd = mean64.float(), inv64.float()
    scale = (gamma.double() * inv64).float()
    shift = (beta.double() - mean64 * gamma.double() * inv64).float()
    gcode = _code(prec) if da16 else L.F32
    rows = L.load().unet_bn_bwd_reduce_rows(P, C)
    part, dg, db, coef, dy = _nan(2, rows, C), _nan(C), _nan(C), _nan(3, C), _nan(P, C, dt=DT[prec])
    L.call("unet_bn_bwd_reduce", _code(prec), gcode, P, C, R.vp(da), R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(mean),
           R.vp(invstd), R.vp(part), R.stream())
    L.call("unet_bn_bwd_finalize", R.vp(part[0]), R.vp(part[1]), rows, C, P, R.vp(gamma), R.vp(mean), R.vp(invstd),
           R.vp(dg), R.vp(db), 0, R.vp(coef), R.stream())
    L.call("unet_bn_bwd_apply", _code(prec), gcode, P, C, R.vp(da), R.vp(y), R.vp(scale), R.vp(shift), 1, R.vp(coef),
           R.vp(dy), R.stream())
    torch.cuda.synchronize()
    mask = (yd * scale.double() + shift.double() > 0).double()
    yl, gl, bl = yd.clone().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    out = torch.nn.functional.batch_norm(yl, None, None, gl, bl, True, 0.0, EPS) * mask
    (out * da.double()).sum().backward()
    s = RO.bn_bwd_sums(da, y, scale, shift, 1, mean, invstd)
    RO.check_sums(dg, gl.grad, s.abs_gx, "dgamma")
    RO.check_sums(db, bl.grad, s.abs_g, "dbeta")
    c = RO.bn_bwd_coef(s.sum_g, s.sum_gx, P, gamma, mean64, inv64)
    RO.check_elem(dy, yl.grad, RO.bn_bwd_apply(s.g, y, c.coef).abs_terms, prec, "dy", rel32=3.2e-5)


# ---- attention gate ----------------------------------------------------------------------------------

GATE_P = [1, 37, 2049]


def gate_operands(prec, P, Ci):
    """gw, xw on a 2^-5 grid within ±(4 − 2^-5) (representable in bf16 and fp16), the BN scales on a 2^-4 grid in
    [0.5, 2], the BN shifts on a 2^-6 grid: g·gs + gb + x·xs + xb is then exact in fp32 in any evaluation order"""
    lim = 4 - 2.0 ** -5
    gw = ((torch.randn(P, Ci, device=DEV) * 1.5 * 32).round() / 32).clamp(-lim, lim).to(DT[prec])
    xw = ((torch.randn(P, Ci, device=DEV) * 1.2 * 32).round() / 32).clamp(-lim, lim).to(DT[prec])
    gab = torch.stack([(_rand(Ci, lo=0.5, hi=2.0) * 16).round() / 16, (_randn(Ci, scale=0.3) * 64).round() / 64])
    xab = torch.stack([(_rand(Ci, lo=0.5, hi=2.0) * 16).round() / 16, (_randn(Ci, scale=0.3) * 64).round() / 64])
    return gw, xw, gab.contiguous(), xab.contiguous()


def assert_a_exact(gw, xw, gab, xab):
    """the fp32 value of a, evaluated two ways, equals the fp64 one bit for bit (zeros included)"""
    g, x = gw.float(), xw.float()
    a64 = RO.gate_act(gw, xw, gab, xab)
    a1 = (g * gab[0] + gab[1] + x * xab[0] + xab[1]).clamp_min(0)
    a2 = (torch.addcmul(gab[1], g, gab[0]) + torch.addcmul(xab[1], x, xab[0])).clamp_min(0)
    assert torch.equal(a1.double(), a64) and torch.equal(a2.double(), a64)
    return a64


@pytest.mark.parametrize("P", GATE_P + [70003])        # 70003: past the 2048-row cap (35 pixels per block)
@pytest.mark.parametrize("Ci", [8, 32, 256, 512, 4, 24, 100])   # vec (G = 1, 4, 32, 64) / scalar
@pytest.mark.parametrize("prec", PRECS)
def test_gate_psi(prec, Ci, P):
    """unet_gate_psi: p = Σ_c wpsi_c·a_c per pixel and the partial Σp, Σp²."""
    L, R = _lr()
    torch.manual_seed(31)
    gw, xw, gab, xab = gate_operands(prec, P, Ci)
    assert_a_exact(gw, xw, gab, xab)
    wpsi = _randn(Ci, scale=0.5)
    rows = L.load().unet_gate_psi_rows(P)
    p, part = _nan(P), _nan(2, rows)
    L.call("unet_gate_psi", _code(prec), P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(wpsi), R.vp(p), R.vp(part),
           R.stream())
    torch.cuda.synchronize()
    ref = RO.gate_psi(gw, xw, gab, xab, wpsi)
    assert torch.isfinite(p).all() and torch.isfinite(part).all()
    err, tol = (p.double() - ref.p).abs(), 2e-5 * ref.abs_p
    assert (err <= tol).all(), ("p", float((err - tol).max()))
    got = part.double().sum(1)
    RO.check_sums(got[0], ref.sum_p, ref.abs_sum_p, "Σp")
    RO.check_sums(got[1], ref.sum_pp, ref.sum_pp, "Σp²")


@pytest.mark.parametrize("P", GATE_P + [70003])
@pytest.mark.parametrize("Cx", [8, 64, 512, 20, 1024])          # vec (G = 1, 8, 64) / scalar
@pytest.mark.parametrize("prec", PRECS)
def test_gate_bwd1(prec, Cx, P):
    """unet_gate_bwd1: dx (absent, stored, accumulated onto a known tensor), dq and the partial Σdq, Σdq·p̂;
    |p·pa + pb| <= 6, so s(1 − s) does not cancel under the fast exponential."""
    L, R = _lr()
    torch.manual_seed(32)
    dxs = _randn(P, Cx)
    yx = _randn(P, Cx, dt=DT[prec])
    sx, bx = _rand(Cx), _randn(Cx, scale=0.3)
    p = _randn(P, scale=1.3).clamp(-4, 4)
    psi_ab = torch.tensor([[1.3], [-0.4]], device=DEV)          # |q| <= 5.6
    pm, pi = torch.tensor([0.15], device=DEV), torch.tensor([0.8], device=DEV)
    rows = L.load().unet_gate_psi_rows(P)
    old = _randn(P, Cx, scale=2.0)
    for mode, relu in (("null", 1), ("store", 0), ("accum", 1), ("store", 1)):
        dx = {"null": None, "store": _nan(P, Cx), "accum": old.clone()}[mode]
        # dq and the partial table sit inside one buffer of 7s: the padding before, between and after them
        # must come back untouched (with dx absent, the only outputs there are)
        PAD = 64
        buf = torch.full((3 * PAD + P + 2 * rows,), 7.0, device=DEV)
        dq, part = buf[PAD:PAD + P], buf[2 * PAD + P:2 * PAD + P + 2 * rows].view(2, rows)
        dq.fill_(NAN)
        part.fill_(NAN)
        L.call("unet_gate_bwd1", _code(prec), P, Cx, R.vp(dxs), R.vp(yx), R.vp(sx), R.vp(bx), relu, R.vp(p), R.vp(psi_ab),
               R.vp(pm), R.vp(pi), R.vp(dx), int(mode == "accum"), R.vp(dq), R.vp(part), R.stream())
        torch.cuda.synchronize()
        ref = RO.gate_bwd1(dxs, yx, sx, bx, relu, p, psi_ab, pm, pi, dx_old=old if mode == "accum" else None)
        assert float(ref.s.min()) > 0.003 and float(ref.s.max()) < 0.997
        assert torch.isfinite(dq).all() and torch.isfinite(part).all()
        err, tol = (dq.double() - ref.dq).abs(), 2e-5 * ref.abs_dq
        assert (err <= tol).all(), ("dq", mode, relu, float((err - tol).max()))
        got = part.double().sum(1)
        RO.check_sums(got[0], ref.sum_dq, ref.abs_sum_dq, ("Σdq", mode, relu))
        RO.check_sums(got[1], ref.sum_dqp, ref.abs_sum_dqp, ("Σdq·p̂", mode, relu))
        pads = torch.cat([buf[:PAD], buf[PAD + P:2 * PAD + P], buf[2 * PAD + P + 2 * rows:]])
        assert bool((pads == 7.0).all()), ("a write outside dq / partial", mode)
        if dx is not None:
            assert torch.isfinite(dx).all()
            assert torch.allclose(dx.double(), ref.dx, rtol=1e-6, atol=1e-6), (mode, float((dx.double() - ref.dx).abs().max()))


# (Ci, UNET_NO_GATE_VEC): the vec kernels (G = 1, 4, 32), the same sizes through the per-channel kernels, and the
# sizes that only the per-channel kernels serve (512: G = 64 > 32)
GATE23 = [(8, False), (32, False), (256, False), (8, True), (32, True), (256, True), (4, False), (24, False), (100, False),
          (512, False)]


@pytest.mark.parametrize("P", GATE_P + [33001])
@pytest.mark.parametrize("form", GATE23, ids=lambda f: f"{f[0]}{'-novec' if f[1] else ''}")
@pytest.mark.parametrize("prec", PRECS)
def test_gate_bwd2_bwd3(prec, form, P, monkeypatch):
    """unet_gate_bwd2: the four [rows][Ci] partial sums (Σdz, Σdz·ĝ, Σdz·x̂, Σdp·a); unet_gate_bwd3: dgw, dxw.
    Both forms (vectorised, per-channel) are held to fp64 separately."""
    L, R = _lr()
    Ci, novec = form
    if novec:
        monkeypatch.setenv("UNET_NO_GATE_VEC", "1")
    else:
        monkeypatch.delenv("UNET_NO_GATE_VEC", raising=False)
    torch.manual_seed(33)
    gw, xw, gab, xab = gate_operands(prec, P, Ci)
    assert_a_exact(gw, xw, gab, xab)
    wpsi = _randn(Ci, scale=0.5)
    gm, gi, xm, xi = _randn(Ci, scale=0.3), _rand(Ci), _randn(Ci, scale=0.3), _rand(Ci)
    dq, p = _randn(P, scale=0.3), _randn(P)
    pcoef = torch.tensor([0.8, -0.11, 0.05], device=DEV)
    gcoef = torch.stack([_rand(Ci), _randn(Ci, scale=0.3), _randn(Ci, scale=0.2)]).contiguous()
    xcoef = torch.stack([_rand(Ci), _randn(Ci, scale=0.3), _randn(Ci, scale=0.2)]).contiguous()
    rows = L.load().unet_gate_bwd2_rows(P, Ci)
    part = _nan(4, rows, Ci)
    L.call("unet_gate_bwd2", _code(prec), P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(gm), R.vp(gi), R.vp(xm),
           R.vp(xi), R.vp(wpsi), R.vp(dq), R.vp(p), R.vp(pcoef), R.vp(part), R.stream())
    dgw, dxw = _nan(P, Ci, dt=DT[prec]), _nan(P, Ci, dt=DT[prec])
    L.call("unet_gate_bwd3", _code(prec), P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(wpsi), R.vp(dq), R.vp(p),
           R.vp(pcoef), R.vp(gcoef), R.vp(xcoef), R.vp(dgw), R.vp(dxw), R.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(part).all(), ("unwritten partial rows", rows)
    r2 = RO.gate_bwd2(gw, xw, gab, xab, gm, gi, xm, xi, wpsi, dq, p, pcoef)
    got = part.double().sum(1)
    for f, name in enumerate(("Σdz", "Σdz·ĝ", "Σdz·x̂", "Σdp·a")):
        RO.check_sums(got[f], r2.sums[f], r2.abs_sums[f], (name, rows))
    r3 = RO.gate_bwd3(gw, xw, gab, xab, wpsi, dq, p, pcoef, gcoef, xcoef)
    RO.check_elem(dgw, r3.dgw, r3.abs_dgw, prec, "dgw")
    RO.check_elem(dxw, r3.dxw, r3.abs_dxw, prec, "dxw")


@pytest.mark.parametrize("shape", [(2049, 64, 32), (4099, 24, 4)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prec", PRECS)
def test_gate_chain_vs_autograd(prec, shape):
    """psi -> bn_finalize (C = 1) -> bwd1 -> bn_bwd_finalize (C = 1) -> bwd2 -> bn_bwd_finalize_multi (two BN jobs
    and the column sum, as GateStage.backward builds it) -> bwd3, every stage fed with the previous kernels' outputs,
    against torch autograd of the whole gate in fp64 (ref_ops.gate_autograd, proved in test_ref_ops_cpu.py).
    The batch statistics of gw / xw are taken in fp64; γ, β are chosen so that γ·invstd and β − mean·γ·invstd fall
    on the grids of gate_operands, and the kernels are handed those affine pairs.
    Gates: all parameter gradients and dwpsi at the partial-sum gate, 2e-5·Σ|terms| + 1e-6 (psi's dγ / dβ against
    Σ|terms| too: they cancel); dx at rtol 1e-6, atol 1e-6; 16-bit dgw / dxw at the eps gate.
    Measured gate (fp32 dgw / dxw only).  Two things defeat 1e-5·(|A·dz| + |B·g| + |Cc|) here, both in fp32 itself:
    dp = pA·dq + pB·p + pCc cancels (psi's BatchNorm backward), so the scale expands dz's own terms
    (ref_ops.gate_bwd3 wide_*: |A·wpsi|·(|pA·dq| + |pB·p| + |pCc|) in place of |A·dz|); and in a channel whose sums
    nearly cancel, B and Cc are small against the fp32 noise of those sums.  Plain fp32 torch autograd against fp64
    autograd on these inputs reaches 2.83e-5 (dgw) / 2.74e-5 (dxw) of the issue's scale at 2049x64x32 and 2.59e-5 /
    2.52e-5 at 4099x24x4; of the expanded scale 6.44e-6 / 1.29e-5 and 3.21e-6 / 3.10e-6.  The gate is
    4 x 1.29e-5 = 5.2e-5 of the expanded scale."""
    L, R = _lr()
    P, Cx, Ci = shape
    code = _code(prec)
    torch.manual_seed(41)
    gw, xw, gab, xab = gate_operands(prec, P, Ci)
    a64 = assert_a_exact(gw, xw, gab, xab)
    wpsi = _randn(Ci, scale=0.5)
    dout = _randn(P, Cx)
    yx = _randn(P, Cx, dt=DT[prec])
    sx, bx = _rand(Cx), _randn(Cx, scale=0.3)

    def stats(t, ab):
        td = t.double()
        mean, inv = td.mean(0), 1.0 / torch.sqrt(td.var(0, unbiased=False) + EPS)
        gamma = ab[0].double() / inv
        return mean, inv, (gamma, ab[1].double() + mean * ab[0].double())

    gm64, gi64, bn_g = stats(gw, gab)
    xm64, xi64, bn_x = stats(xw, xab)
    gm, gi, xm, xi = gm64.float(), gi64.float(), xm64.float(), xi64.float()
    gamma_g, gamma_x = bn_g[0].float(), bn_x[0].float()
    pref = RO.gate_psi(gw, xw, gab, xab, wpsi)
    ph = (pref.p - pref.p.mean()) / pref.p.std(unbiased=False)
    gamma_p = torch.tensor([min(1.2, 5.0 / float(ph.abs().max()))], device=DEV)     # |q| <= 5.3
    beta_p = torch.tensor([0.3], device=DEV)

    # forward
    rows1 = L.load().unet_gate_psi_rows(P)
    p, part = _nan(P), _nan(2, rows1)
    L.call("unet_gate_psi", code, P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(wpsi), R.vp(p), R.vp(part), R.stream())
    psi_ab, psi_mean, psi_inv = _nan(2, 1), _nan(1), _nan(1)
    L.call("unet_bn_finalize", R.vp(part), rows1, 1, P, R.vp(gamma_p), R.vp(beta_p), None, None, None, 0.1, EPS,
           R.vp(psi_mean), R.vp(psi_inv), R.vp(psi_ab[0]), R.vp(psi_ab[1]), R.stream())
    # backward
    dx, dq, part1 = _nan(P, Cx), _nan(P), _nan(2, rows1)
    L.call("unet_gate_bwd1", code, P, Cx, R.vp(dout), R.vp(yx), R.vp(sx), R.vp(bx), 1, R.vp(p), R.vp(psi_ab), R.vp(psi_mean),
           R.vp(psi_inv), R.vp(dx), 0, R.vp(dq), R.vp(part1), R.stream())
    dgp, dbp, pcoef = _nan(1), _nan(1), _nan(3)
    L.call("unet_bn_bwd_finalize", R.vp(part1[0]), R.vp(part1[1]), rows1, 1, P, R.vp(gamma_p), R.vp(psi_mean), R.vp(psi_inv),
           R.vp(dgp), R.vp(dbp), 0, R.vp(pcoef), R.stream())
    rows2 = L.load().unet_gate_bwd2_rows(P, Ci)
    part2 = _nan(4, rows2, Ci)
    L.call("unet_gate_bwd2", code, P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(gm), R.vp(gi), R.vp(xm), R.vp(xi),
           R.vp(wpsi), R.vp(dq), R.vp(p), R.vp(pcoef), R.vp(part2), R.stream())
    dgg, dbg, gcoef, dgx, dbx, xcoef, dwpsi = _nan(Ci), _nan(Ci), _nan(3, Ci), _nan(Ci), _nan(Ci), _nan(3, Ci), _nan(Ci)
    jobs = []
    for sgx, gamma, mean, inv, dg, db, coef in ((part2[1], gamma_g, gm, gi, dgg, dbg, gcoef),
                                                (part2[2], gamma_x, xm, xi, dgx, dbx, xcoef),
                                                (None, None, None, None, None, dwpsi, None)):
        j = L.BnBwdFinJob()
        j.sum_g, j.sum_gx, j.rows, j.C = R.vp(part2[0] if coef is not None else part2[3]), R.vp(sgx), rows2, Ci
        j.count = P if coef is not None else 0
        j.gamma, j.mean, j.invstd = R.vp(gamma), R.vp(mean), R.vp(inv)
        j.dgamma, j.dbeta, j.accum, j.coef = R.vp(dg), R.vp(db), 0, R.vp(coef)
        jobs.append(j)
    L.call("unet_bn_bwd_finalize_multi", len(jobs), (L.BnBwdFinJob * len(jobs))(*jobs), R.stream())
    dgw, dxw = _nan(P, Ci, dt=DT[prec]), _nan(P, Ci, dt=DT[prec])
    L.call("unet_gate_bwd3", code, P, Ci, R.vp(gw), R.vp(xw), R.vp(gab), R.vp(xab), R.vp(wpsi), R.vp(dq), R.vp(p), R.vp(pcoef),
           R.vp(gcoef), R.vp(xcoef), R.vp(dgw), R.vp(dxw), R.stream())
    torch.cuda.synchronize()

    x64 = RO.act(yx, sx, bx, 1)
    ref = RO.gate_autograd(gw, xw, x64, dout, wpsi, bn_g, bn_x, (gamma_p, beta_p), EPS, mask=a64 > 0)
    assert float(ref.q.abs().max()) <= 6.0
    # the natural scales, from the fp64 chain of the references
    pm64, pi64 = pref.p.mean(), 1.0 / torch.sqrt(pref.p.var(unbiased=False) + EPS)
    pab64 = torch.stack([gamma_p.double() * pi64, beta_p.double() - pm64 * gamma_p.double() * pi64])
    b1 = RO.gate_bwd1(dout, yx, sx, bx, 1, pref.p, pab64, pm64, pi64)
    pc = RO.bn_bwd_coef(b1.sum_dq.reshape(1), b1.sum_dqp.reshape(1), P, gamma_p, pm64, pi64)
    b2 = RO.gate_bwd2(gw, xw, gab, xab, gm64, gi64, xm64, xi64, wpsi, b1.dq, pref.p, pc.coef)
    gc = RO.bn_bwd_coef(b2.sums[0], b2.sums[1], P, bn_g[0], gm64, gi64)
    xc = RO.bn_bwd_coef(b2.sums[0], b2.sums[2], P, bn_x[0], xm64, xi64)
    b3 = RO.gate_bwd3(gw, xw, gab, xab, wpsi, b1.dq, pref.p, pc.coef, gc.coef, xc.coef)

    for t in (p, dq, dx, dgw, dxw):
        assert torch.isfinite(t).all()
    assert torch.allclose(dx.double(), ref.d_x, rtol=1e-6, atol=1e-6), ("dx", float((dx.double() - ref.d_x).abs().max()))
    RO.check_sums(dgp, ref.d_psi_gamma.reshape(1), b1.abs_sum_dqp.reshape(1), "psi dgamma")
    RO.check_sums(dbp, ref.d_psi_beta.reshape(1), b1.abs_sum_dq.reshape(1), "psi dbeta")
    RO.check_sums(dbg, ref.d_g_beta, b2.abs_sums[0], "W_g dbeta")
    RO.check_sums(dgg, ref.d_g_gamma, b2.abs_sums[1], "W_g dgamma")
    RO.check_sums(dbx, ref.d_x_beta, b2.abs_sums[0], "W_x dbeta")
    RO.check_sums(dgx, ref.d_x_gamma, b2.abs_sums[2], "W_x dgamma")
    RO.check_sums(dwpsi, ref.d_wpsi, b2.abs_sums[3], "dwpsi")
    RO.check_elem(dgw, ref.d_gw, b3.wide_dgw, prec, "dgw", rel32=5.2e-5)
    RO.check_elem(dxw, ref.d_xw, b3.wide_dxw, prec, "dxw", rel32=5.2e-5)
