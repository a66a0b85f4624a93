"""GPU: the device training augmentation (csrc/augment.hip, GpuTrainAugment) against the fp64 restatement of
its semantics (tests/aug_ref.py).

Shapes are the smallest at which the kernels can still go wrong: S = 64 from 64x64 (no resize pass), S = 48
from 50x70 (both resize passes, non-square mask tables), S = 96 with the default sigma = 10 (R = 40: the
reflect border is hit on both sides of every row and column, two vertical-pass row tiles), S = 40 with
sigma = 3, and S = 45 (not a multiple of 4: the scalar-store form of the apply kernel).  N = 5 per case.

Image tolerances: for each (case, transform) the largest |fp32 restatement - fp64 restatement| over these very
inputs, computed on the CPU, times 4 (the device contracts multiply-adds and its logf / cosf differ from
numpy's by ulps).  None is derived from device output.  Masks are exact except at pixels whose fp64 source
coordinate has a fractional part within 1e-3 of 0.5 in either axis (aug_ref.tie_pixels), whose share is
capped at 1 % per case."""

import functools

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu

N = 5
CASES = {
    "s64": dict(S=64, h=64, w=64, sigma=10.0, seed=1),
    "s48": dict(S=48, h=50, w=70, sigma=10.0, seed=2),
    "s96": dict(S=96, h=96, w=96, sigma=10.0, seed=3),
    "s40": dict(S=40, h=40, w=40, sigma=3.0, seed=4),
    "s45": dict(S=45, h=45, w=45, sigma=3.0, seed=5),
}
KINDS = {"affine": R.AFFINE, "grid": R.GRID, "elastic": R.ELASTIC, "brightness": R.BRIGHTNESS, "noise": R.NOISE,
         "all": R.ALL_FLAGS, "mixed": None}

# 4 x max |fp32 restatement - fp64 restatement| of the normalised image over the case's 5 samples (measured value
# in the comment), from tools/augment_tolerances.py on the CPU
TOL = {
    ("s64", "affine"): 4.959e-05,   # measured 1.240e-05; ties 0.49%
    ("s64", "grid"): 2.813e-05,   # measured 7.033e-06; ties 0.62%
    ("s64", "elastic"): 1.907e-05,   # measured 4.768e-06; ties 0.39%
    ("s64", "brightness"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s64", "noise"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s64", "all"): 5.245e-05,   # measured 1.311e-05; ties 0.40%
    ("s64", "mixed"): 4.435e-05,   # measured 1.109e-05; ties 0.34%
    ("s48", "affine"): 2.122e-05,   # measured 5.305e-06; ties 0.49%
    ("s48", "grid"): 2.384e-05,   # measured 5.960e-06; ties 0.00%
    ("s48", "elastic"): 1.335e-05,   # measured 3.338e-06; ties 0.38%
    ("s48", "brightness"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s48", "noise"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s48", "all"): 5.198e-05,   # measured 1.299e-05; ties 0.43%
    ("s48", "mixed"): 3.839e-05,   # measured 9.596e-06; ties 0.36%
    ("s96", "affine"): 7.677e-05,   # measured 1.919e-05; ties 0.40%
    ("s96", "grid"): 8.106e-05,   # measured 2.027e-05; ties 0.62%
    ("s96", "elastic"): 4.101e-05,   # measured 1.025e-05; ties 0.46%
    ("s96", "brightness"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s96", "noise"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s96", "all"): 1.364e-04,   # measured 3.409e-05; ties 0.32%
    ("s96", "mixed"): 1.247e-04,   # measured 3.117e-05; ties 0.30%
    ("s40", "affine"): 2.694e-05,   # measured 6.735e-06; ties 0.41%
    ("s40", "grid"): 1.860e-05,   # measured 4.649e-06; ties 0.00%
    ("s40", "elastic"): 2.527e-05,   # measured 6.318e-06; ties 0.35%
    ("s40", "brightness"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s40", "noise"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s40", "all"): 5.722e-05,   # measured 1.431e-05; ties 0.36%
    ("s40", "mixed"): 3.171e-05,   # measured 7.927e-06; ties 0.26%
    ("s45", "affine"): 3.529e-05,   # measured 8.821e-06; ties 0.47%
    ("s45", "grid"): 1.431e-05,   # measured 3.576e-06; ties 0.00%
    ("s45", "elastic"): 2.337e-05,   # measured 5.841e-06; ties 0.34%
    ("s45", "brightness"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s45", "noise"): 4.768e-07,   # measured 1.192e-07; ties 0.00%
    ("s45", "all"): 6.747e-05,   # measured 1.687e-05; ties 0.37%
    ("s45", "mixed"): 3.958e-05,   # measured 9.894e-06; ties 0.20%
}
# the same for the elastic displacement field (pixels)
FIELD_TOL = {
    "s64": 9.633e-06,   # measured 2.408e-06 px
    "s48": 1.674e-05,   # measured 4.184e-06 px
    "s96": 7.211e-06,   # measured 1.803e-06 px
    "s40": 1.411e-05,   # measured 3.527e-06 px
    "s45": 1.210e-05,   # measured 3.025e-06 px
}


@functools.lru_cache(maxsize=None)
def inputs(case):
    c = CASES[case]
    rng = np.random.default_rng(100 + c["seed"])
    h, w = c["h"], c["w"]
    imgs = rng.integers(0, 256, (N, h, w), dtype=np.uint8)
    masks = np.zeros((N, h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for i in range(N):
        cy, cx, r = rng.integers(h // 4, 3 * h // 4), rng.integers(w // 4, 3 * w // 4), rng.integers(5, h // 3)
        masks[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
        masks[i][rng.random((h, w)) < 0.01] = 128          # values either side of the > 127 cut
    return imgs, masks


def table(case, kind):
    """5 drawn rows with the flags of `kind` forced: one transform alone, all of them, the flips, the dropout,
    or 'mixed' = the drawn flags, except sample 0 with none set and sample 1 with all set"""
    from unet.utils.gpu_pipeline import draw_train_augment
    c = CASES[case]
    tab = draw_train_augment(N, c["S"], np.random.default_rng(c["seed"]), p_flip=0.5, p_vflip=0.5, p_affine=0.5,
                             p_elastic=0.5, p_grid=0.5, p_brightness=0.5, p_noise=0.5, p_dropout=0.5)
    if kind == "mixed":
        tab["flags"][0], tab["flags"][1] = 0, R.ALL_FLAGS
    elif kind == "flips":
        tab["flags"] = [R.HFLIP, R.VFLIP, R.HFLIP | R.VFLIP, 0, R.HFLIP]
    elif kind == "dropout":
        tab["flags"] = R.DROPOUT
    else:
        tab["flags"] = KINDS[kind]
    return tab


@functools.lru_cache(maxsize=None)
def reference(case, kind, dtype=np.float64):
    """fp64 restatement of every sample: (images (N, S, S) fp32, masks (N, S, S), tie pixels (N, S, S))"""
    c = CASES[case]
    imgs, masks = inputs(case)
    tab = table(case, kind)
    out = [R.train_augment(imgs[i], masks[i], c["S"], tab[i], sigma=c["sigma"], dtype=dtype) for i in range(N)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.stack([R.tie_pixels(*o[2]) for o in out]))


def device(case, kind):
    from unet.utils.gpu_pipeline import GpuTrainAugment
    c = CASES[case]
    imgs, masks = inputs(case)
    aug = GpuTrainAugment(img_size=c["S"], sigma=c["sigma"])
    tab = None if kind is None else table(case, kind)
    img, mask = aug(torch.from_numpy(imgs), torch.from_numpy(masks), tab)
    torch.cuda.synchronize()
    assert img.shape == (N, 1, c["S"], c["S"]) and img.dtype == torch.float32
    assert mask.shape == (N, c["S"], c["S"]) and mask.dtype == torch.int64
    return img[:, 0].cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_params_none_equals_slice_transform(case):
    from unet.utils.gpu_pipeline import GpuSliceTransform
    c = CASES[case]
    imgs, masks = inputs(case)
    ri, rm = GpuSliceTransform(img_size=c["S"])(torch.from_numpy(imgs), torch.from_numpy(masks), flips=None)
    img, mask = device(case, None)
    assert np.array_equal(img, ri[:, 0].cpu().numpy()) and np.array_equal(mask, rm.cpu().numpy())
    from unet.utils.gpu_pipeline import GpuTrainAugment
    only, none = GpuTrainAugment(img_size=c["S"])(torch.from_numpy(imgs))        # no masks
    assert none is None and np.array_equal(only[:, 0].cpu().numpy(), img)


@pytest.mark.parametrize("case", list(CASES))
def test_flips_only_bit_exact(case):
    ri, rm, tie = reference(case, "flips")
    img, mask = device(case, "flips")
    assert not tie.any()
    assert np.array_equal(img, ri) and np.array_equal(mask, rm)
    assert not np.array_equal(img[0], img[3])


@pytest.mark.parametrize("case", list(CASES))
def test_dropout_only(case):
    c = CASES[case]
    tab = table(case, "dropout")
    plain, pmask = device(case, None)
    img, mask = device(case, "dropout")
    hole = np.zeros(img.shape, bool)
    for i in range(N):
        assert 1 <= tab["n_holes"][i] <= 4
        for x0, y0, x1, y1 in tab["holes"][i][:tab["n_holes"][i]]:
            hole[i, y0:y1, x0:x1] = True
    assert hole.any(axis=(1, 2)).all()
    fill = (np.float32(0) - np.float32(0.5)) / np.float32(0.5)
    assert np.all(img[hole] == fill)
    assert np.array_equal(img[~hole], plain[~hole])
    assert np.array_equal(mask, pmask)                       # the mask is left untouched
    assert np.array_equal(img, reference(case, "dropout")[0])


@pytest.mark.parametrize("case", list(CASES))
def test_elastic_field(case):
    from unet.utils.gpu_pipeline import GpuTrainAugment
    c = CASES[case]
    S = c["S"]
    tab = table(case, "mixed")
    rows = np.array([3, 1, 4], np.int32)                     # a compact list, not in table order
    aug = GpuTrainAugment(img_size=S, sigma=c["sigma"])
    f = aug.elastic_fields(torch.from_numpy(tab.view(np.uint8)).cuda(), torch.from_numpy(rows).cuda(), N)
    torch.cuda.synchronize()
    assert f.shape == (3, 2, S, S)
    f = f.cpu().numpy()
    worst = 0.0
    for j, i in enumerate(rows):
        ref = R.elastic_field(S, tab["key"][i], 50.0, c["sigma"])
        worst = max(worst, float(np.abs(f[j] - ref).max()))
        assert 0.2 < ref.std() and np.abs(ref).max() < 50.0
    print(f"\nelastic field {case}: max|device - fp64| {worst:.3e} px (tolerance {FIELD_TOL[case]:.3e})")
    assert worst <= FIELD_TOL[case]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", list(CASES))
def test_transform_against_fp64(case, kind):
    ri, rm, tie = reference(case, kind)
    img, mask = device(case, kind)
    err = float(np.abs(img - ri).max())
    share = float(tie.mean())
    wrong = (mask != rm) & ~tie
    print(f"\n{case} {kind}: image max|device - fp64| {err:.3e} (tolerance {TOL[case, kind]:.3e}); mask: "
          f"{int((mask != rm).sum())} differ, all on the {share:.2%} tie pixels" if not wrong.any() else
          f"\n{case} {kind}: image {err:.3e}; {int(wrong.sum())} mask pixels differ off the ties")
    assert share <= 0.01, share
    assert not wrong.any(), int(wrong.sum())
    assert err <= TOL[case, kind], (err, TOL[case, kind])
    if kind in ("affine", "grid", "elastic", "all"):         # the transform did something
        plain = reference(case, "flips")[0][3]               # sample 3 of 'flips' has no flag set
        assert np.abs(ri[3] - plain).max() > 0.1


def test_noise_statistics():
    """sigma = 0.02 on a constant mid-grey image (no clipping within 20 sigma): mean, std, keys, repeatability"""
    from unet.utils.gpu_pipeline import AUG_DTYPE, GpuTrainAugment
    S, n = 64, 4
    tab = np.zeros(n, AUG_DTYPE)
    tab["flags"], tab["noise_sigma"] = R.NOISE, 0.02
    tab["key"] = [[1, 2], [3, 4], [0xFFFFFFFF, 0], [1, 2]]
    grey = torch.full((n, S, S), 128, dtype=torch.uint8)
    aug = GpuTrainAugment(img_size=S)
    a = aug(grey, None, tab)[0][:, 0].cpu().numpy()
    b = aug(grey, None, tab)[0][:, 0].cpu().numpy()
    assert np.array_equal(a, b)                              # the same keys reproduce bit for bit
    assert np.array_equal(a[0], a[3]) and not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    sigma = float(np.float32(0.02))
    for i in range(n):
        d = a[i].astype(np.float64) * 0.5 + 0.5 - 128.0 / 255.0
        print(f"\nnoise sample {i}: mean {d.mean():+.3e} (bound {4 * sigma / np.sqrt(d.size):.3e}), std/sigma {d.std() / sigma:.4f}")
        assert abs(d.mean()) <= 4 * sigma / np.sqrt(d.size)
        assert abs(d.std() / sigma - 1) <= 0.03


def test_argument_errors_launch_nothing():
    from unet._hip import lib as L
    from unet._hip.runtime import stream, vp
    from unet.utils.gpu_pipeline import AUG_DTYPE, GpuTrainAugment
    S, n = 32, 2
    dev = torch.device("cuda")
    r = torch.zeros(n, S, S, dtype=torch.uint8, device=dev)
    tab = torch.zeros(n * AUG_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    out = torch.full((n, 1, S, S), 7.0, device=dev)

    def apply(img, table, table_len, o, field=None, n_el=0):
        L.call("unet_aug_apply", n, S, vp(img), 0, 0, None, None, None, vp(table), table_len, vp(field), n_el, 0.5, 0.5,
               vp(o), None, stream())

    for args in ((None, tab, n, out), (r, None, n, out), (r, tab, n, None), (r, tab, n + 1, out), (r, tab, n - 1, out)):
        with pytest.raises(RuntimeError, match="unet_aug_apply"):
            apply(*args)
    with pytest.raises(RuntimeError, match="unet_aug_apply"):
        apply(r, tab, n, out, None, 1)                       # elastic slots without a field buffer
    taps = torch.ones(81, device=dev)
    slots = torch.zeros(1, dtype=torch.int32, device=dev)
    buf = torch.full((2, 1, 2, S, S), 7.0, device=dev)

    def field(S_, R_, t, tb, sl, tmp, f):
        L.call("unet_aug_elastic_field", 1, S_, 50.0, R_, vp(t), n, vp(tb), vp(sl), vp(tmp), vp(f), stream())

    with pytest.raises(RuntimeError, match="exceed the Gaussian radius"):
        field(S, 40, taps, tab, slots, buf[0], buf[1])       # S <= R
    with pytest.raises(RuntimeError, match="exceed the Gaussian radius"):
        field(S, S, taps, tab, slots, buf[0], buf[1])
    for args in ((S, 3, None, tab, slots, buf[0], buf[1]), (S, 3, taps, None, slots, buf[0], buf[1]),
                 (S, 3, taps, tab, None, buf[0], buf[1]), (S, 3, taps, tab, slots, None, buf[1]),
                 (S, 3, taps, tab, slots, buf[0], None)):
        with pytest.raises(RuntimeError, match="unet_aug_elastic_field"):
            field(*args)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 7.0).all())   # nothing was launched
    # the same through the class
    aug = GpuTrainAugment(img_size=S)                        # sigma = 10: R = 40 >= 32
    imgs = torch.zeros(n, S, S, dtype=torch.uint8)
    rows = np.zeros(n, AUG_DTYPE)
    with pytest.raises(RuntimeError, match="parameter rows"):
        aug(imgs, None, np.zeros(n + 1, AUG_DTYPE))
    rows["flags"] = R.ELASTIC
    with pytest.raises(RuntimeError, match="img_size >"):
        aug(imgs, None, rows)
    rows["flags"] = R.AFFINE | R.NOISE                       # and without the elastic flag the same object works
    rows["inv_affine"] = [1, 0, 0, 0, 1, 0]
    assert aug(imgs, None, rows)[0].shape == (n, 1, S, S)
