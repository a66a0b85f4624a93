"""CPU: the host side of the device training augmentation — the fp64 restatement (tests/aug_ref.py) against
scipy, Pillow and the slice-pipeline restatement, the Philox known answers, the host-side parameter draw
(draw_train_augment) and the YAML front end (create_train_transform)."""

import numpy as np
import pytest
import scipy.ndimage as ndi

import aug_ref as R
from oracle import pipeline_oracle as PO


def _slice(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    mask[(yy - h // 2) ** 2 + (xx - w // 3) ** 2 <= (h // 5) ** 2] = 255
    mask[rng.random((h, w)) < 0.01] = 128
    return img, mask


def _row(S, seed=0, flags=0):
    from unet.utils.gpu_pipeline import draw_train_augment
    row = draw_train_augment(1, S, np.random.default_rng(seed))[0].copy()
    row["flags"] = flags
    return row


def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10"""
    z = [int(v) for v in R.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert z == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    o = [int(v) for v in R.philox4x32_10(f, f, f, f, f, f)]
    assert o == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_affine_only_equals_scipy_map_coordinates():
    S = 48
    img, mask = _slice(50, 70, 1)
    row = _row(S, 3, R.AFFINE)
    out, _, (cx, cy) = R.train_augment(img, mask, S, row)
    r, _ = R.resized_inputs(img, mask, S)
    ref = ndi.map_coordinates(r.astype(np.float64) / 255.0, [cy, cx], order=1, mode="grid-constant", cval=0.0)
    assert (cx.min() < -1) or (cx.max() > S)                # the zero border is exercised
    v = out.astype(np.float64) * 0.5 + 0.5
    assert np.abs(v - ref).max() <= 2e-7                     # fp32 rounding of the output stage only
    # and before that rounding: to 1e-15
    t = np.zeros((S + 2, S + 2))
    t[1:-1, 1:-1] = r / 255.0
    x0, y0 = np.floor(cx).astype(int), np.floor(cy).astype(int)
    fx, fy = cx - x0, cy - y0
    g = lambda xi, yi: t[np.clip(yi, -1, S) + 1, np.clip(xi, -1, S) + 1]
    mine = (g(x0, y0) * (1 - fx) + g(x0 + 1, y0) * fx) * (1 - fy) + (g(x0, y0 + 1) * (1 - fx) + g(x0 + 1, y0 + 1) * fx) * fy
    assert np.abs(mine - ref).max() <= 1e-15


@pytest.mark.parametrize("S,sigma", [(96, 10.0), (40, 3.0)])
def test_elastic_field_equals_scipy_gaussian_filter(S, sigma):
    key = (123456789, 987654321)
    d = R.elastic_field(S, key, 50.0, sigma)
    for comp in range(2):
        u = R.field_uniform(S, key, comp)
        assert u.min() >= -1.0 and u.max() < 1.0 and np.array_equal(u, u.astype(np.float32))
        ref = 50.0 * ndi.gaussian_filter(u, sigma, mode="mirror", truncate=4.0)
        assert np.abs(d[comp] - ref).max() <= 1e-13
    assert np.abs(d).max() < 50.0 and d.std() > 0


@pytest.mark.parametrize("h,w,S", [(64, 64, 64), (50, 70, 48)])
def test_all_off_equals_training_slice_and_flips_equal_np_flip(h, w, S):
    img, mask = _slice(h, w, S)
    ri, rm = PO.training_slice(img, mask, S, flip=False)
    ri, rm = ri[0].numpy(), rm.numpy()
    out, m, _ = R.train_augment(img, mask, S, _row(S, 1, 0))
    assert np.array_equal(out, ri) and np.array_equal(m, rm)
    for flags, axes in ((R.HFLIP, (1,)), (R.VFLIP, (0,)), (R.HFLIP | R.VFLIP, (0, 1))):
        out, m, _ = R.train_augment(img, mask, S, _row(S, 1, flags))
        assert np.array_equal(out, np.flip(ri, axes)) and np.array_equal(m, np.flip(rm, axes)), flags


def test_fp32_mode_stays_close_to_fp64():
    S = 48
    img, mask = _slice(50, 70, 2)
    row = _row(S, 5, R.ALL_FLAGS)
    a, _, _ = R.train_augment(img, mask, S, row)
    b, _, _ = R.train_augment(img, mask, S, row, dtype=np.float32)
    assert 0 < np.abs(a - b).max() < 1e-3


# ---- draw_train_augment ------------------------------------------------------------------------

def test_draw_is_deterministic_and_row_independent_of_n():
    from unet.utils.gpu_pipeline import AUG_DTYPE, draw_train_augment
    a = draw_train_augment(16, 512, np.random.default_rng(7))
    b = draw_train_augment(16, 512, np.random.default_rng(7))
    assert a.dtype == AUG_DTYPE and a.tobytes() == b.tobytes()
    c = draw_train_augment(5, 512, np.random.default_rng(7))
    assert c.tobytes() == a[:5].tobytes()
    assert draw_train_augment(16, 512, np.random.default_rng(8)).tobytes() != a.tobytes()


def test_draw_ranges_and_affine_inverse():
    from unet._hip import lib as L
    from unet.utils.gpu_pipeline import affine_matrices, draw_train_augment
    S, n = 512, 4000
    tab, raw = draw_train_augment(n, S, np.random.default_rng(11), return_raw=True)
    assert np.abs(raw["theta"]).max() <= 15 and np.abs(raw["theta"]).max() > 14
    for k in ("sx", "sy"):
        assert raw[k].min() >= 0.85 and raw[k].max() <= 1.15
    for k in ("tx", "ty"):
        assert np.abs(raw[k]).max() <= 0.1 * S
    assert abs(np.corrcoef(raw["sx"], raw["sy"])[0, 1]) < 0.1          # drawn independently
    for i in range(0, n, 40):
        r = raw[i]
        A, Ai = affine_matrices(r["theta"], r["sx"], r["sy"], r["tx"], r["ty"], S)
        assert np.abs(A @ Ai - np.eye(3)).max() <= 1e-12
        assert np.array_equal(tab["inv_affine"][i], Ai[:2].reshape(6).astype(np.float32))
        c = (S - 1) / 2                                                 # the centre moves by t
        assert np.allclose(A @ [c, c, 1], [c + r["tx"], c + r["ty"], 1], atol=1e-9)
    for g in (tab["gx"], tab["gy"]):
        assert np.all(g[:, 0] == 0) and np.all(g[:, 5] == S)
        steps = np.diff(g.astype(np.float64), axis=1) / (S / 5)
        assert steps.min() >= 0.8 / 1.2 - 1e-6 and steps.max() <= 1.2 / 0.8 + 1e-6   # (1 +- 0.2) after the rescale
    assert tab["contrast"].min() >= 0.85 and tab["contrast"].max() <= 1.15
    assert np.abs(tab["brightness"]).max() <= 0.15
    assert tab["noise_sigma"].min() >= 0.01 and tab["noise_sigma"].max() <= np.float32(0.02)
    assert tab["n_holes"].min() == 1 and tab["n_holes"].max() == 4
    h = tab["holes"].astype(np.int64)
    side = np.concatenate([(h[..., 2] - h[..., 0]).ravel(), (h[..., 3] - h[..., 1]).ravel()])
    assert side.min() >= round(0.03 * S) and side.max() <= round(0.06 * S)
    assert h[..., :2].min() >= 0 and h[..., 2:].max() <= S
    assert len(np.unique(tab["key"][:, 0])) > n - 5
    el = (tab["flags"] & L.AUG_ELASTIC) != 0
    assert np.array_equal(tab["elastic_slot"][el], np.arange(el.sum())) and np.all(tab["elastic_slot"][~el] == -1)


def test_draw_flag_frequencies():
    """each flag fires with its probability (within 4 binomial standard deviations over 4000 samples); the
    defaults are the reference's, and p_rotate is accepted and ignored"""
    from unet._hip import lib as L
    from unet.utils.gpu_pipeline import draw_train_augment
    n = 4000
    expect = {L.AUG_HFLIP: 0.5, L.AUG_VFLIP: 0.3, L.AUG_AFFINE: 0.5, L.AUG_ELASTIC: 0.3, L.AUG_GRID: 0.3,
              L.AUG_BRIGHTNESS: 0.3, L.AUG_NOISE: 0.2, L.AUG_DROPOUT: 0.1}
    tab = draw_train_augment(n, 256, np.random.default_rng(3), p_rotate=0.0)
    for bit, p in expect.items():
        f = float(((tab["flags"] & bit) != 0).mean())
        assert abs(f - p) <= 4 * np.sqrt(p * (1 - p) / n), (bit, f, p)
    tab = draw_train_augment(n, 256, np.random.default_rng(3), p_flip=0.1, p_elastic=0.6, p_brightness=0.9)
    for bit, p in {L.AUG_HFLIP: 0.1, L.AUG_ELASTIC: 0.6, L.AUG_BRIGHTNESS: 0.9}.items():
        f = float(((tab["flags"] & bit) != 0).mean())
        assert abs(f - p) <= 4 * np.sqrt(p * (1 - p) / n), (bit, f, p)


def test_table_layout_matches_the_c_struct():
    import ctypes
    from unet._hip import lib as L
    from unet.utils.gpu_pipeline import AUG_DTYPE
    assert AUG_DTYPE.itemsize == ctypes.sizeof(L.AugParams) == 168
    for name, _ in L.AugParams._fields_:
        assert AUG_DTYPE.fields[name][1] == getattr(L.AugParams, name).offset, name


def test_create_train_transform_maps_yaml_keys():
    import yaml
    from unet.utils import create_train_transform
    from unet.utils.gpu_pipeline import GpuTrainAugment
    cfg = yaml.safe_load("""
data: {img_size: 512}
augmentation:
  enabled: true
  horizontal_flip: 0.4
  rotation_limit: 20
  elastic: 0.25
  brightness_contrast: 0.35
""")
    tf = create_train_transform(cfg, device="cpu")     # the constructor touches no device
    assert isinstance(tf, GpuTrainAugment) and tf.img_size == 512 and tf.radius == 40
    assert tf.draw_options == {"p_flip": 0.4, "rotation_limit": 20, "p_elastic": 0.25, "p_brightness": 0.35}
    tab, raw = tf.draw(500, np.random.default_rng(0)), None
    from unet.utils.gpu_pipeline import draw_train_augment
    ref, raw = draw_train_augment(500, 512, np.random.default_rng(0), p_flip=0.4, rotation_limit=20, p_elastic=0.25,
                                  p_brightness=0.35, return_raw=True)
    assert tab.tobytes() == ref.tobytes() and 15 < np.abs(raw["theta"]).max() <= 20
    dflt = create_train_transform({"data": {"img_size": 256}}, device="cpu")      # train.py's defaults
    assert dflt.draw_options == {"p_flip": 0.5, "rotation_limit": 15, "p_elastic": 0.3, "p_brightness": 0.3}
    cfg["augmentation"]["enabled"] = False
    assert create_train_transform(cfg) is None
    with pytest.raises(TypeError):
        GpuTrainAugment(img_size=64, device="cpu", p_shear=0.5)


def test_no_cpu_fallback_for_the_augmentation():
    import torch
    from unet.utils.gpu_pipeline import GpuTrainAugment
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        GpuTrainAugment(img_size=32, device="cpu")(torch.zeros(1, 32, 32, dtype=torch.uint8))
