"""GPU op-level numerics of the fused loss (csrc/loss.hip): the six unet_loss_* entry points called directly
through the C-ABI, each pass on its own, against the fp64 references of tests/ref_ops.py (proved against the
oracle's loss functions and torch autograd in tests/test_ref_ops_cpu.py).

Every output is filled with NaN before the launch and must come back finite wherever the contract writes; a
refused call must leave the NaN in place.

Gates
  counts (n0, n1, T_c)   exact
  partial sums           |got − ref| <= GATE_FIELD · Σ|terms| per field and row (the terms are >= 0, so a field is
                         its own scale, except S0 / S1 = Σ(lse − z_t), scale Σ(|lse| + |z_t|))
  finalize outputs       fp64 arithmetic rounded once to fp32: rtol 1e-6 (ref_ops.check_fin), the scalar relative
                         to its largest term
  dz, element-wise       |got − ref| <= GATE_DZ · |gout|·(|w_t|(p_k + [k=t]) + |G_k p_k| + p_k Σ_c|G_c p_c|)
  outer limits           the module-level gates of the loss: 1e-5·(1 + |loss|), 1e-6 + 1e-4·max|dz|
GATE_FIELD and GATE_DZ are measured, not derived: on the same inputs the same quantity formed in plain fp32 torch
(ref_ops with dtype=float32: softmax / logsumexp / autograd in fp32) is compared with fp64, and the gate is 4 times
the largest ratio over the cases of this file, for the kernels' fast __expf / __logf and their different
summation order.  Each test prints its own ratio (pytest -s).  The measured values stand in the docstrings of
test_loss_reduce and test_loss_grad."""

import numpy as np
import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = 1001, 1002
KS = [1, 2, 3, 5, 16]
HWS = [1, 255, 1024, 1025, 37 * 41, 3000]
GATE_FIELD = 4 * 5.2e-7      # test_loss_reduce
GATE_DZ = 4 * 1.21e-6        # test_loss_grad
FLUSH = 1e-30                # fp32 flushes terms below 1.2e-38 to 0


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _f32(v):
    return float(np.float32(v))


def _cfg(ce_w=1.0, dice_w=1.0, class_w=0.5, ce_smooth=1e-6, dice_smooth=1.0, ignore_bg=1, reduction=0):
    """the configuration as the entry points receive it: floats"""
    return RO.loss_cfg(_f32(ce_w), _f32(dice_w), _f32(class_w), _f32(ce_smooth), _f32(dice_smooth), ignore_bg, reduction)


CFGS = [_cfg(), _cfg(0.8, 1.3, 0.3, 1e-3, 0.7, 0, 1), _cfg(0.0, 1.0, 0.5, 1e-6, 1.0, 1, 2),
        _cfg(0.0, 1.0, 0.5, 1e-6, 0.25, 0, 2), _cfg(1.7, 0.6, 0.9, 0.5, 2.0, 0, 0), _cfg(1.0, 1.0, 0.5, 1e-6, 1.0, 1, 1)]


def _targets(N, K, HW, gen):
    """random labels with −1, K and 255 mixed in; with three images, the second is all 0 and the third all 1"""
    t = torch.randint(0, K, (N, HW), generator=gen, device=DEV)
    bad = torch.tensor([-1, K, 255], device=DEV)
    pos = torch.arange(HW, device=DEV)
    t[:, ::7] = bad[(pos[::7] // 7) % 3]
    if N >= 3:
        t[1] = 0
        t[2] = 1
    return t.contiguous()


def _logits(S, N, K, HW, gen, saturated=False):
    z = [torch.randn(N, K, HW, generator=gen, device=DEV) * 2 for _ in range(S)]
    if saturated:    # |z| up to 80, the classes more than 100 apart, on every other pixel
        for zz in z:
            mag = 50 + 30 * torch.rand(N, K, HW, generator=gen, device=DEV)
            sign = torch.where(torch.randint(0, K, (N, 1, HW), generator=gen, device=DEV)
                               == torch.arange(K, device=DEV).view(1, K, 1), 1.0, -1.0)
            zz[..., ::2] = (mag * sign)[..., ::2]
    return [zz.contiguous() for zz in z]


def _ptrs(L, ts):
    return (L.c_vp * len(ts))(*[t.data_ptr() for t in ts])


def _reduce(S, N, K, HW, z, t, part):
    L, R = _lr()
    if S == 1:
        L.call("unet_loss_reduce", N, K, HW, R.vp(z[0]), R.vp(t), R.vp(part), R.stream())
    else:
        L.call("unet_loss_reduce_multi", S, N, K, HW, _ptrs(L, z), R.vp(t), R.vp(part), R.stream())


def _finalize(S, part, rows, N, K, cfg, weights, loss, coef):
    """returns the entry point's code (0, or a refusal)"""
    L, R = _lr()
    lib = L.load()
    tail = (N, K, cfg.ce_w, cfg.dice_w, cfg.class_w, cfg.ce_smooth, cfg.dice_smooth, cfg.ignore_bg, cfg.reduction,
            R.vp(loss), R.vp(coef), R.stream())
    if weights is None:
        return lib.unet_loss_finalize(R.vp(part), rows, *tail)
    return lib.unet_loss_finalize_multi(R.vp(part), rows, S, (L.c_float * S)(*weights), *tail)


def _grad(S, N, K, HW, z, t, coef, gout, per_elem, ignore_bg, dz):
    L, R = _lr()
    if S == 1:
        L.call("unet_loss_grad", N, K, HW, R.vp(z[0]), R.vp(t), R.vp(coef), R.vp(gout), per_elem, ignore_bg,
               R.vp(dz[0]), R.stream())
    else:
        L.call("unet_loss_grad_multi", S, N, K, HW, _ptrs(L, z), R.vp(t), R.vp(coef), R.vp(gout), per_elem, ignore_bg,
               _ptrs(L, dz), R.stream())


def _ratio(err, scale):
    m = scale > 1e-20          # below, the flush-to-zero term of the gate decides
    return float((err[m] / scale[m]).max()) if bool(m.any()) else 0.0


def _check_partial(got, z, t, rows, K, what):
    """one set's table [N, rows, F] against the fp64 sums of each row's pixel range; returns the fp32-torch ratio"""
    ref = RO.loss_partial(z, t, rows)
    got = got.double()
    assert torch.isfinite(got).all(), (what, "not finite")
    counts = [0, 1] + [4 + 3 * c + 2 for c in range(K)]
    assert torch.equal(got[..., counts], ref.part[..., counts]), (what, "counts")
    err, tol = (got - ref.part).abs(), GATE_FIELD * ref.abs_terms + FLUSH
    assert (err <= tol).all(), (what,) + RO._worst(err, tol)
    f32 = RO.loss_partial(z, t, rows, torch.float32).part.double()
    return _ratio((f32 - ref.part).abs(), ref.abs_terms), _ratio(err, ref.abs_terms)


def _expected_rows(HW):
    return min(1024, max(1, -(-HW // 1024)))


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("K", KS)
def test_loss_reduce(K, HW):
    """unet_loss_reduce (S = 1) and unet_loss_reduce_multi (S = 4), N = 1 and 3: every field of every partial row
    against the fp64 sums of that row's ceil(HW / rows) pixels; labels −1, K and 255, an all-0 and an all-1 image.
    Measured on these inputs (MI355X): fp32 torch is within 5.2e-7·Σ|terms| of fp64 (the largest over the cases: K = 16
    at HW = 1; 0.9e-7 to 1.8e-7 at HW >= 255) and the kernel within 6.6e-7; GATE_FIELD = 4 × 5.2e-7 = 2.1e-6."""
    L, _ = _lr()
    rows = L.load().unet_loss_rows(HW)
    assert rows == _expected_rows(HW)
    worst = (0.0, 0.0)
    for N, S in ((1, 1), (3, 1), (1, 4), (3, 4)):
        gen = torch.Generator(device=DEV).manual_seed(1000 * K + HW + N + S)
        z, t = _logits(S, N, K, HW, gen), _targets(N, K, HW, gen)
        part = _nan(S, N, rows, 4 + 3 * K)
        _reduce(S, N, K, HW, z, t, part)
        torch.cuda.synchronize()
        for s in range(S):
            worst = tuple(map(max, worst, _check_partial(part[s], z[s], t, rows, K, (N, S, s))))
    print(f"\nreduce K={K} HW={HW}: fp32 torch / kernel error over the natural scale {worst[0]:.3e} / {worst[1]:.3e}")


def test_loss_reduce_row_cap():
    """HW = 1025² > 1024·1024: the row count stops at 1024 and every row covers ceil(HW / 1024) = 1027 pixels"""
    L, _ = _lr()
    N, K, HW = 1, 2, 1025 * 1025
    rows = L.load().unet_loss_rows(HW)
    assert rows == 1024
    gen = torch.Generator(device=DEV).manual_seed(77)
    z, t = _logits(1, N, K, HW, gen), _targets(N, K, HW, gen)
    part = _nan(1, N, rows, 4 + 3 * K)
    _reduce(1, N, K, HW, z, t, part)
    torch.cuda.synchronize()
    r = _check_partial(part[0], z[0], t, rows, K, "cap")
    assert float(part[0, 0, :, 4 + 2::3].sum(-1).max()) <= 1027
    print(f"\nreduce row cap: fp32 torch / kernel error over the natural scale {r[0]:.3e} / {r[1]:.3e}")


def test_loss_reduce_refuses_17_classes():
    L, R = _lr()
    z, t = torch.zeros(1, 17, 8, device=DEV), torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    part = _nan(1, 1, 4 + 3 * 17)
    assert L.load().unet_loss_reduce(1, 17, 8, R.vp(z), R.vp(t), R.vp(part), R.stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(part.isnan().all())


# ---- finalize -------------------------------------------------------------------------------------------

def _table(S, N, rows, K, gen):
    """a partial table the test writes itself: plausible counts and sums"""
    def u(*s):
        return torch.rand(*s, generator=gen, device=DEV)
    T = torch.randint(0, 60, (S, N, rows, K), generator=gen, device=DEV).float()
    T[:] = T[0]                                   # the sets share the targets
    P = u(S, N, rows, K) * 60
    I = u(S, N, rows, K) * torch.minimum(P, T)
    n0 = T[..., 0]
    n1 = T[..., 1] if K > 1 else torch.zeros_like(n0)
    tab = torch.cat([torch.stack([n0, n1, u(S, N, rows) * 2 * n0, u(S, N, rows) * 2 * n1], -1),
                     torch.stack([I, P, T], -1).reshape(S, N, rows, 3 * K)], -1)
    return tab.contiguous()


def _finalize_ref(tab, K, cfg, weights):
    S, N = tab.shape[:2]
    fields = tab.double().sum(2)
    if cfg.reduction == 2:
        v = RO.loss_value(fields[0], K, cfg)
        loss, scale = v.loss, v.abs
    else:
        vs = [RO.loss_value(fields[s], K, cfg) for s in range(S)]
        loss = sum(w * v.loss for w, v in zip(weights, vs))
        scale = sum(abs(w) * v.abs for w, v in zip(weights, vs))
    return loss, scale, torch.stack([RO.loss_coef(fields[s], K, cfg, weights[s]) for s in range(S)])


FIN_CASES = [(1, 2, 1), (3, 2, 65), (2, 5, 200), (4, 16, 3), (3, 1, 64), (2, 3, 1024), (576, 2, 2)]


@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_loss_finalize(case):
    """unet_loss_finalize on a table of the test's own: the loss (scalar for mean / sum, [N][nd] for none) and the
    coefficient table [N][2 + 2K] for ignore_bg 0 / 1, the three reductions and non-default ce_w, dice_w, class_w,
    ce_smooth, dice_smooth; 1 row, 64, 65 and 200 rows (the 64-lane row sum wraps), 1024 rows (that the sum is
    carried in fp64: test_loss_finalize_row_sum_in_fp64); N = 576 is the
    largest batch the 60000-byte LDS limit admits at K = 2.  fp64 arithmetic rounded once: rtol 1e-6."""
    N, K, rows = case
    gen = torch.Generator(device=DEV).manual_seed(7 + rows)
    tab = _table(1, N, rows, K, gen)
    for cfg in CFGS:
        nd = K - (1 if cfg.ignore_bg and K > 1 else 0)
        loss = _nan(N, nd) if cfg.reduction == 2 else _nan(1)
        coef = _nan(N, 2 + 2 * K)
        assert _finalize(1, tab, rows, N, K, cfg, None, loss, coef) == 0
        torch.cuda.synchronize()
        ref_loss, scale, ref_coef = _finalize_ref(tab, K, cfg, [1.0])
        RO.check_fin(loss, ref_loss, ("loss", cfg), scale)
        RO.check_fin(coef, ref_coef[0], ("coef", cfg))
        assert abs(float(loss.double().sum() - ref_loss.sum())) <= 1e-5 * (1 + abs(float(ref_loss.sum())))


def _lane_sum_fp32(col):
    """what the finalize's row sum would give with an fp32 accumulator: lane l adds rows l, l + 64, ... one after the
    other, then the xor tree over the 64 lanes"""
    rows = col.numel()
    a = torch.nn.functional.pad(col.float(), [0, -rows % 64]).view(-1, 64)
    acc = torch.zeros(64, dtype=torch.float32, device=col.device)
    for r in range(a.shape[0]):
        acc = acc + a[r]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[torch.arange(64, device=col.device) ^ o]
    return float(acc[0])


@pytest.mark.parametrize("rows", [65, 200, 1024])
def test_loss_finalize_row_sum_in_fp64(rows):
    """The finalize adds the partial rows in fp64.  Image 0, every class: I_c and T_c hold A = 2^26 in row 0 and 0
    elsewhere, P_c holds A in row 0 and 3.5 in every other row.  The fp32 spacing at 2^26 is 8, so an fp32 accumulator
    absorbs each 3.5 that meets A.  With reduction none the loss is 1 − D = (P + T − 2I)/(P + T + ds) = 3.5·(rows − 1)/
    (2A + ...): the small terms alone, which an fp32 row sum gets wrong by a percent or more (emulated here and
    asserted to lie outside the gate, so the check cannot pass for a sum carried in fp32).  fp64 arithmetic, then
    one rounding to fp32: rtol 1e-6 of 1 − D itself; gA, gB within 2^-23.  Nothing goes through n0 / n1, which
    the finalize rounds to fp32 as the module does."""
    N, K, A = 2, 3, 2.0 ** 26
    gen = torch.Generator(device=DEV).manual_seed(70 + rows)
    tab = _table(1, N, rows, K, gen)
    tab[0, 0, :, 4:] = 0.0
    tab[0, 0, 0, 4:] = A                       # I, P, T of every class
    tab[0, 0, 1:, 5::3] = 3.5                  # P
    cfg = CFGS[3]                              # Dice alone, ignore_bg 0, reduction none, dice_smooth 0.25
    loss, coef = _nan(N, K), _nan(N, 2 + 2 * K)
    assert _finalize(1, tab, rows, N, K, cfg, None, loss, coef) == 0
    torch.cuda.synchronize()
    ref_loss, _, ref_coef = _finalize_ref(tab, K, cfg, [1.0])
    want = 3.5 * (rows - 1) / (2 * A + 3.5 * (rows - 1) + cfg.dice_smooth)
    assert abs(float(ref_loss[0, 0]) / want - 1) <= 1e-9       # 1 − D cancels: 2^-53 / 2.7e-5 in fp64
    assert torch.isfinite(loss).all() and torch.isfinite(coef).all()
    err = (loss.double() - ref_loss).abs()
    assert (err <= 1e-6 * ref_loss.abs()).all(), (loss, ref_loss)
    RO.check_fin(coef[:, 2:], ref_coef[0][:, 2:], "gA, gB", rtol=2.0 ** -23)
    # an fp32 accumulator on the same column
    p32 = _lane_sum_fp32(tab[0, 0, :, 5])
    lost = (p32 + A - 2 * A) / (p32 + A + cfg.dice_smooth)
    assert abs(lost - want) > 1e-3 * want, (p32, lost, want)


@pytest.mark.parametrize("case", [(1, 2, 1), (3, 2, 130), (2, 5, 7)], ids=lambda c: "x".join(map(str, c)))
def test_loss_finalize_multi(case):
    """unet_loss_finalize_multi, S = 4 (and S = 2) with set weights: Σ_s w_s·loss_s and per-set coefficients
    already scaled by w_s; mean and sum"""
    N, K, rows = case
    gen = torch.Generator(device=DEV).manual_seed(17 + rows)
    for S, weights in ((4, [1.0, 0.4, 0.2, 0.1]), (2, [0.75, 1.5])):
        weights = [_f32(w) for w in weights]
        tab = _table(S, N, rows, K, gen)
        for cfg in (CFGS[0], CFGS[1], CFGS[4], CFGS[5]):
            loss, coef = _nan(1), _nan(S, N, 2 + 2 * K)
            assert _finalize(S, tab, rows, N, K, cfg, weights, loss, coef) == 0
            torch.cuda.synchronize()
            ref_loss, scale, ref_coef = _finalize_ref(tab, K, cfg, weights)
            RO.check_fin(loss, ref_loss, ("loss", S, cfg), scale)
            RO.check_fin(coef, ref_coef, ("coef", S, cfg))


def test_loss_finalize_refusals():
    """S > 1 with reduction none: UNET_ERR_ARG; N = 577 at K = 2 (60008 bytes of LDS): UNET_ERR_UNSUPPORTED; the
    NaN-filled outputs stay untouched"""
    gen = torch.Generator(device=DEV).manual_seed(3)
    tab = _table(4, 2, 3, 2, gen)
    loss, coef = _nan(2, 1), _nan(4, 2, 6)
    assert _finalize(4, tab, 3, 2, 2, CFGS[2], [1.0, 0.4, 0.2, 0.1], loss, coef) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(loss.isnan().all()) and bool(coef.isnan().all())
    tab = _table(1, 577, 2, 2, gen)
    loss, coef = _nan(1), _nan(577, 6)
    assert _finalize(1, tab, 2, 577, 2, CFGS[0], None, loss, coef) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(loss.isnan().all()) and bool(coef.isnan().all())


# ---- grad -----------------------------------------------------------------------------------------------

# (cfg, gout): scalars 1, 0.37 and 65536; per-element [N][nd] with reduction none
GRAD_CFGS = [(CFGS[0], 1.0), (CFGS[1], 0.37), (CFGS[5], 65536.0), (CFGS[4], 0.37), (CFGS[2], None), (CFGS[3], None)]


def _check_dz(got, z, t, cfg, gout, set_w, what):
    """one set's dz against fp64 autograd, element-wise over the natural scale (from the coefficient formula) and
    by the outer gate; returns the fp32-torch and the kernel's ratio"""
    K = z.shape[1]
    ref = RO.loss_dz(z, t, cfg, gout, set_w)
    coef = RO.loss_coef(RO.loss_fields(z, t), K, cfg, set_w)
    terms = RO.loss_dz_terms(z, t, coef, gout, cfg.reduction == 2, cfg.ignore_bg).abs_terms
    got = got.double()
    assert torch.isfinite(got).all(), (what, "not finite")
    gmax = float(torch.as_tensor(gout).abs().max())
    err, tol = (got - ref).abs(), GATE_DZ * terms + FLUSH * max(1.0, gmax)
    assert (err <= tol).all(), (what,) + RO._worst(err, tol)
    assert float(err.max()) <= 1e-6 + 1e-4 * float(ref.abs().max()), what
    f32 = RO.loss_dz(z, t, cfg, gout, set_w, torch.float32).double()
    return _ratio((f32 - ref).abs(), terms), _ratio(err, terms)


def _ref_coef(z, t, K, cfg, weights):
    """the reference's coefficients, rounded to the fp32 table the grad pass reads"""
    return torch.stack([RO.loss_coef(RO.loss_fields(zz, t), K, cfg, w) for zz, w in zip(z, weights)]).float().contiguous()


def _gout(cfg, N, K, g, gen):
    if cfg.reduction != 2:
        return torch.tensor([g], device=DEV)
    nd = K - (1 if cfg.ignore_bg and K > 1 else 0)
    return (torch.rand(N, nd, generator=gen, device=DEV) * 3 - 1).contiguous()


@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("K", KS)
def test_loss_grad(K, HW):
    """unet_loss_grad with the reference's coefficients (a finalize error cannot mask a grad error): scalar gout 1,
    0.37 and 65536, per-element gout [N][nd] with reduction none, ignore_bg 0 and 1, N = 3 (an all-0 and an all-1
    image, out-of-range labels).  Measured on these inputs (MI355X): fp32 autograd through the reference is within
    1.21e-6·Σ|terms| of fp64 (the largest over the cases: K = 16 at HW = 1024) and the kernel within 1.55e-6;
    GATE_DZ = 4 × 1.21e-6 = 4.84e-6.  The saturated regime of test_loss_chain is held to the same gate."""
    N = 3
    gen = torch.Generator(device=DEV).manual_seed(2000 * K + HW)
    z, t = _logits(1, N, K, HW, gen), _targets(N, K, HW, gen)
    worst = (0.0, 0.0)
    for cfg, g in GRAD_CFGS:
        gout = _gout(cfg, N, K, g, gen)
        coef = _ref_coef(z, t, K, cfg, [1.0])
        dz = [_nan(N, K, HW)]
        _grad(1, N, K, HW, z, t, coef, gout, int(cfg.reduction == 2), cfg.ignore_bg, dz)
        torch.cuda.synchronize()
        go = gout if cfg.reduction == 2 else float(gout)
        worst = tuple(map(max, worst, _check_dz(dz[0], z[0], t, cfg, go, 1.0, (cfg, g))))
    print(f"\ngrad K={K} HW={HW}: fp32 torch / kernel error over the natural scale {worst[0]:.3e} / {worst[1]:.3e}")


def test_loss_grad_multi_wraps_the_grid():
    """unet_loss_grad_multi, S = 4, N = 3, HW = 175003: S·N·HW = 2100036 > 8192·256 elements, so the grid-stride
    loop runs a second trip, and a trip crosses set boundaries"""
    S, N, K, HW = 4, 3, 2, 175003
    assert S * N * HW > 8192 * 256
    weights = [1.0, _f32(0.4), _f32(0.2), _f32(0.1)]
    gen = torch.Generator(device=DEV).manual_seed(5)
    z, t = _logits(S, N, K, HW, gen), _targets(N, K, HW, gen)
    cfg, gout = CFGS[0], torch.tensor([0.37], device=DEV)
    coef = _ref_coef(z, t, K, cfg, weights)
    dz = [_nan(N, K, HW) for _ in range(S)]
    _grad(S, N, K, HW, z, t, coef, gout, 0, cfg.ignore_bg, dz)
    torch.cuda.synchronize()
    for s in range(S):
        _check_dz(dz[s], z[s], t, cfg, float(gout), weights[s], ("set", s))


# ---- the three passes in a row --------------------------------------------------------------------------

@pytest.mark.parametrize("saturated", [False, True], ids=["randn2", "saturated"])
@pytest.mark.parametrize("S", [1, 4])
def test_loss_chain(S, saturated):
    """reduce -> finalize -> grad on the device's own intermediates, at logits randn·2 and in a saturated regime
    (|z| up to 80, the classes more than 100 apart, on every other pixel): nothing NaN or inf, the scalar within
    1e-5·(1 + |loss|) of the fp64 loss, the partial sums within their per-field gate, dz within the element gate
    and 1e-6 + 1e-4·max|dz|"""
    L, _ = _lr()
    N, K, HW = 3, 3, 37 * 41
    weights = [1.0, _f32(0.4), _f32(0.2), _f32(0.1)][:S]
    gen = torch.Generator(device=DEV).manual_seed(31 + S)
    z, t = _logits(S, N, K, HW, gen, saturated), _targets(N, K, HW, gen)
    if saturated:
        assert float(z[0].abs().max()) > 75 and float((z[0][..., ::2].amax(1) - z[0][..., ::2].amin(1)).min()) > 100
    rows = L.load().unet_loss_rows(HW)
    for cfg in (CFGS[0], CFGS[1]):
        part, loss, coef = _nan(S, N, rows, 4 + 3 * K), _nan(1), _nan(S, N, 2 + 2 * K)
        _reduce(S, N, K, HW, z, t, part)
        assert _finalize(S, part, rows, N, K, cfg, weights if S > 1 else None, loss, coef) == 0
        gout = torch.tensor([0.37], device=DEV)
        dz = [_nan(N, K, HW) for _ in range(S)]
        _grad(S, N, K, HW, z, t, coef, gout, 0, cfg.ignore_bg, dz)
        torch.cuda.synchronize()
        assert torch.isfinite(part).all() and torch.isfinite(coef).all() and torch.isfinite(loss).all()
        vs = [RO.loss_value(RO.loss_fields(zz, t), K, cfg) for zz in z]
        ref = float(sum(w * v.loss for w, v in zip(weights, vs)))
        scale = float(sum(abs(w) * v.abs for w, v in zip(weights, vs)))
        err = abs(float(loss) - ref)
        assert err <= 1e-5 * (1 + abs(ref)), (err, ref, scale)
        r = (0.0, 0.0)
        for s in range(S):
            _check_partial(part[s], z[s], t, rows, K, ("part", s))
            r = tuple(map(max, r, _check_dz(dz[s], z[s], t, cfg, 0.37, weights[s], ("dz", s))))
        print(f"\nchain S={S} saturated={saturated}: loss err {err:.3e} (ref {ref:.6f}); dz fp32 torch / kernel "
              f"{r[0]:.3e} / {r[1]:.3e}")
