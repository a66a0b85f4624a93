"""GPU numerics of the multi-class loss (csrc/loss_ce.hip) through its public classes: CrossEntropyLoss, DiceCELoss
and DeepSupervisionLoss over them, against plain torch in fp64 on the CPU (F.cross_entropy; the DiceLoss formula
written inline with invalid pixels masked out of the softmax and of the one-hot), gradients from torch.autograd.grad
of that reference with a non-unit upstream factor.

Targets: about 20 % ignore_index, with N = 3 the second image entirely ignored, and a few labels >= K, which must
behave as ignored (the reference sees them rewritten to ignore_index).

Gates
  loss scalar            1e-5·(1 + |loss|)             (the module-level gate of tests/test_gpu_loss_ops.py)
  dz                     1e-6 + 1e-4·max|dz|           (likewise); exactly 0 at invalid pixels
  'none' map, and the    not bounded there: |got − ref| <= GATE·a + one fp32 ulp of |ref|, a the sum of the absolute
  scalar with smoothing  terms (1−ε)·w_t·(|lse| + |z_t| + 1) + (ε/K)·Σ_k w_k·(|lse| + |z_k| + 1) of the pixel (of all
                         valid pixels, over Wsum for 'mean').  The 1: lse = max + log(se) with se = Σ exp(z − max) in
                         [1, K] rounded to fp32, and d log(se) = d se / se, so the logarithm carries an absolute error
                         of up to 2^-24 however small lse − z_t is (a pixel whose own class dominates).
                         GATE = 2 × the largest such ratio of torch's own fp32 F.cross_entropy on the GPU over the
                         cases of test_cross_entropy, the factor for the different summation order (1024-pixel fp32
                         rows, then fp64, against torch's tree).
Measured (MI355X; each test prints its own, pytest -s): the 'none' map: torch fp32 1.84e-7, the kernel 1.71e-7,
GATE_MAP = 3.68e-7; the scalar with smoothing: torch fp32 7.63e-8, the kernel 9.19e-8, GATE_SMOOTH = 1.53e-7."""

import itertools

import pytest
import torch
import torch.nn.functional as F

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV, IGN = "cuda", -100
KS = [2, 4, 5, 8, 9, 16]                              # both sides of every padded-class bucket (4, 8, 16)
SHAPES = [(7, 9), (32, 32), (36, 36), (33, 31)]       # scalar path below one row; one row; a row + a partial; unaligned tail
GATE_MAP = 2 * 1.84e-7       # measured: torch fp32 1.84e-7, the kernel 1.71e-7 (both at K = 16, 32 x 32)
GATE_SMOOTH = 2 * 7.63e-8    # measured: torch fp32 7.63e-8 (K = 9, 33 x 31, 'sum'), the kernel 9.19e-8 (K = 16, 33 x 31, 'mean')


def _case(N, K, H, W, weighted, all_ignored=False):
    """logits, the targets as given (with labels >= K), the targets the reference sees, the weights (or None)"""
    g = torch.Generator().manual_seed(1000 * K + 10 * H + N)
    z = torch.randn(N, K, H, W, generator=g) * 2
    t = torch.randint(0, K, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.2] = IGN
    if N > 1:
        t[1] = IGN
    if all_ignored:
        t[:] = IGN
    t_ref = t.clone()
    t.view(-1)[5::97] = K
    t.view(-1)[11::89] = K + 250
    t_ref.view(-1)[5::97] = IGN
    t_ref.view(-1)[11::89] = IGN
    w = None
    if weighted:
        w = torch.rand(K, generator=g) + 0.25
        w[K // 2] = 0.0
    return z, t, t_ref, w


ALL = list(itertools.product((1, 3), (False, True), (0.0, 0.1)))      # N x weighted x label smoothing
CASES = [(K, hw, red, ALL, False) for K in KS for hw in SHAPES for red in ("mean", "sum", "none")]
# 1 x 2 x 1028 x 1024: unet_loss_rows stops at 1024 rows, so every block strides to a second trip of 4 pixels
CASES.append((2, (1028, 1024), "mean", [(1, True, 0.1)], False))
# every pixel ignored: NaN for 'mean' like torch, 0 for 'sum'
CASES += [(4, (7, 9), red, [(3, True, 0.1), (1, False, 0.0)], True) for red in ("mean", "sum")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"K{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}" + ("-ignored" * c[4]))
def test_cross_entropy(case):
    """CrossEntropyLoss against F.cross_entropy in fp64, loss (scalar or map) and dz, for N in {1, 3} x (no weights |
    random positive weights with one class at 0) x label smoothing in {0, 0.1}"""
    from unet.utils.loss import CrossEntropyLoss
    K, hw, reduction, combos, all_ignored = case
    worst, bad = (0.0, 0.0), []
    for N, weighted, eps in combos:
        z, t, t_ref, w = _case(N, K, *hw, weighted, all_ignored)
        wd = None if w is None else w.double()
        zr = z.double().requires_grad_()
        ref = F.cross_entropy(zr, t_ref, wd, ignore_index=IGN, label_smoothing=eps, reduction=reduction)
        up = torch.rand(ref.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64) + 2.5
        crit = CrossEntropyLoss(weight=w, ignore_index=IGN, reduction=reduction, label_smoothing=eps).to(DEV)
        zg = z.to(DEV).requires_grad_()
        got = crit(zg, t.to(DEV))
        (dz,) = torch.autograd.grad((got * up.to(DEV).float()).sum(), zg)
        got, dz = got.detach().double().cpu(), dz.double().cpu()
        assert not dz.transpose(0, 1)[:, t_ref == IGN].any(), "an invalid pixel got a gradient"
        if all_ignored:
            assert torch.isnan(ref) and torch.isnan(got) if reduction == "mean" else float(got) == float(ref.detach()) == 0.0
            continue
        (dref,) = torch.autograd.grad((ref * up).sum(), zr)
        assert float((dz - dref).abs().max()) <= 1e-6 + 1e-4 * float(dref.abs().max())
        ref = ref.detach()
        err = (got - ref).abs()
        if reduction != "none" and eps == 0:
            assert float(err) <= 1e-5 * (1 + abs(float(ref))), (float(got), float(ref))
            continue
        # the absolute terms (1−ε)·w_t·(|lse| + |z_t| + 1) + (ε/K)·Σ_k w_k·(|lse| + |z_k| + 1) of every valid pixel
        zd, valid = z.double(), t_ref != IGN
        a = (torch.logsumexp(zd, 1, keepdim=True).abs() + zd.abs() + 1) * (1.0 if w is None else wd.view(1, K, 1, 1))
        a = ((1 - eps) * a.gather(1, t_ref.clamp(min=0).unsqueeze(1)).squeeze(1) + eps / K * a.sum(1)) * valid
        if reduction != "none":
            wsum = valid.sum().double() if w is None else wd[t_ref[valid]].sum()
            a = a.sum() / (wsum if reduction == "mean" else 1.0)
        tol = (GATE_MAP if reduction == "none" else GATE_SMOOTH) * a + RO.ulp(ref, torch.float32)
        if not bool((err <= tol).all()):
            bad.append((N, weighted, eps) + RO._worst(err, tol))
        t32 = F.cross_entropy(z.to(DEV), t_ref.to(DEV), None if w is None else w.to(DEV), ignore_index=IGN,
                              label_smoothing=eps, reduction=reduction).double().cpu()
        m = a > 0
        worst = (max(worst[0], float(((t32 - ref).abs() / a)[m].max())), max(worst[1], float((err / a)[m].max())))
    print(f"\nce {case[:3]}: fp32 torch / kernel error over the natural scale {worst[0]:.3e} / {worst[1]:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("K", KS)
def test_dice_ce(K, hw):
    """DiceCELoss (weights, smoothing 0.1, ce / dice weights 0.7 / 1.3, Dice smooth 0.5, with and without the
    background class) against the fp64 sum of the two terms; with dice_weight = 0 the same bits as CrossEntropyLoss"""
    from unet.utils.loss import CrossEntropyLoss, DiceCELoss
    z, t, t_ref, w = _case(3, K, *hw, True)
    zg, tg = z.to(DEV).requires_grad_(), t.to(DEV)
    for ignore_bg in (True, False):
        zr = z.double().requires_grad_()
        valid = (t_ref != IGN).unsqueeze(1)
        oh = F.one_hot(t_ref.clamp(min=0), K).permute(0, 3, 1, 2).double() * valid
        p = torch.softmax(zr, 1) * valid
        D = (2 * (p * oh).sum((2, 3)) + 0.5) / (p.sum((2, 3)) + oh.sum((2, 3)) + 0.5)
        ref = (0.7 * F.cross_entropy(zr, t_ref, w.double(), ignore_index=IGN, label_smoothing=0.1)
               + 1.3 * (1 - D[:, int(ignore_bg):].mean()))
        (dref,) = torch.autograd.grad(3 * ref, zr)
        crit = DiceCELoss(0.7, 1.3, w.tolist(), IGN, 0.1, smooth=0.5, ignore_background=ignore_bg).to(DEV)
        got = crit(zg, tg)
        (dz,) = torch.autograd.grad(3 * got, zg)
        assert abs(float(got) - float(ref)) <= 1e-5 * (1 + abs(float(ref))), (float(got), float(ref))
        assert float((dz.double().cpu() - dref).abs().max()) <= 1e-6 + 1e-4 * float(dref.abs().max())
        assert not dz.transpose(0, 1)[:, (t_ref == IGN).to(DEV)].any()
    a = DiceCELoss(1.0, 0.0, w.tolist(), IGN, 0.1).to(DEV)(zg, tg)
    b = CrossEntropyLoss(weight=w, ignore_index=IGN, label_smoothing=0.1).to(DEV)(zg, tg)
    assert torch.equal(a, b)
    assert torch.equal(torch.autograd.grad(a, zg)[0], torch.autograd.grad(b, zg)[0])


@pytest.mark.parametrize("base", ["ce_mean", "ce_sum", "dice_ce"])
@pytest.mark.parametrize("S", [2, 4])
def test_deep_supervision_multi(S, base):
    """S sets through one launch of each pass equal Σ w_s·loss_s of the single-set path: the loss within
    1e-5·(1 + |loss|); every dz within 8 fp32 roundings of max|dz| (the set weight enters the coefficients before
    their rounding on one side and multiplies the upstream gradient on the other)"""
    from unet.utils.loss import CrossEntropyLoss, DeepSupervisionLoss, DiceCELoss
    z, t, _, w = _case(3, 5, 33, 31, True)
    crit = {"ce_mean": CrossEntropyLoss(weight=w, label_smoothing=0.1), "ce_sum": CrossEntropyLoss(reduction="sum"),
            "dice_ce": DiceCELoss(class_weights=w.tolist(), label_smoothing=0.1)}[base].to(DEV)
    g = torch.Generator().manual_seed(S)
    zs = [(z + torch.randn(z.shape, generator=g)).to(DEV).requires_grad_() for _ in range(S)]
    ws = [1.0, 0.4, 0.2, 0.1][:S]
    multi = DeepSupervisionLoss(crit, ws)(zs, t.to(DEV))
    single = sum(wt * crit(zz, t.to(DEV)) for wt, zz in zip(ws, zs))
    assert abs(float(multi) - float(single)) <= 1e-5 * (1 + abs(float(single)))
    for dm, ds in zip(torch.autograd.grad(3 * multi, zs), torch.autograd.grad(3 * single, zs)):
        assert float((dm - ds).abs().max()) <= 8 * 2.0 ** -23 * float(ds.abs().max())


def test_two_runs_are_bit_identical():
    from unet.utils.loss import DeepSupervisionLoss, DiceCELoss
    z, t, _, w = _case(3, 9, 36, 36, True)
    crit = DeepSupervisionLoss(DiceCELoss(class_weights=w.tolist(), label_smoothing=0.1).to(DEV), [1.0, 0.4])
    runs = []
    for _ in range(2):
        zs = [z.to(DEV).requires_grad_(), (z * 0.5).to(DEV).requires_grad_()]
        loss = crit(zs, t.to(DEV))
        runs.append((loss.detach(), *torch.autograd.grad(loss, zs)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("kind", ["cpu", "probabilities", "17_classes"])
def test_fallbacks_are_torch_bit_for_bit(kind):
    from unet.utils.loss import CrossEntropyLoss
    K = 17 if kind == "17_classes" else 5
    z, _, t, w = _case(2, K, 7, 9, True)
    if kind == "probabilities":
        t = torch.softmax(torch.randn(2, K, 7, 9, generator=torch.Generator().manual_seed(1)), 1)
    if kind != "cpu":
        z, t, w = z.to(DEV), t.to(DEV), w.to(DEV)
    kw = dict(weight=w, label_smoothing=0.1, ignore_index=IGN)
    assert torch.equal(CrossEntropyLoss(**kw)(z, t), torch.nn.CrossEntropyLoss(**kw)(z, t))


def test_factory_builds_the_new_losses():
    from unet.utils import CrossEntropyLoss, DiceCELoss, create_loss_function
    crit = create_loss_function("dice_ce", ce_weight=0.5, dice_weight=2.0, class_weights=[1.0, 2.0, 3.0])
    assert isinstance(crit, DiceCELoss) and (crit.ce_weight, crit.dice_weight) == (0.5, 2.0)
    assert crit.weight.tolist() == [1.0, 2.0, 3.0]
    assert type(create_loss_function("ce", class_weights=[1.0, 2.0])) is CrossEntropyLoss
