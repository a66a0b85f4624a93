"""Device-side slice preprocessing (the GPU input pipeline).

The reference prepares every training slice on the CPU in a DataLoader worker
(`LungTumorDataset.__getitem__`, unet/data/dataset.py:133-171, and the albumentations-free fallback
`apply_basic_transforms`, unet/data/augmentations.py:119-171): PIL decode, a float round trip
(u8 / 255 * 255 -> uint8), `Image.resize(BILINEAR)` of the image and `NEAREST` of the mask, a random
horizontal flip, /255 and (x - mean) / std, mask > 127 -> int64.  At ~1,000 img/s per node, 4 CPU
workers per GPU cannot keep up.  Here only the PNG decode stays on the host: a batch of decoded 8-bit
slices is uploaded once and every other step runs as integer/byte HIP kernels (csrc/infer.hip) with
Pillow's own resampling tables (unet.utils.pil_tables), bit-exact with the CPU path.

    tf = GpuSliceTransform(img_size=512)
    images, masks = tf(u8_slices, u8_masks, flips=draw_flips(len(u8_slices)))
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .._hip import lib as L
from .._hip.runtime import require_device, stream, vp
from .pil_tables import bilinear_tables, nearest_table


def draw_flips(n: int, rng=np.random) -> np.ndarray:
    """The reference's per-sample flip decision, `np.random.rand() > 0.5` (augmentations.py:161), drawn in
    sample order from the same global numpy stream."""
    return np.array([rng.rand() > 0.5 for _ in range(n)], dtype=bool)


class _Tables:
    def __init__(self, device):
        self.device = device
        self._cache = {}

    def bilinear(self, in_size: int, out_size: int):
        key = ("b", in_size, out_size)
        if key not in self._cache:
            b, k = bilinear_tables(in_size, out_size)
            self._cache[key] = (torch.from_numpy(b.copy()).to(self.device), torch.from_numpy(k.copy()).to(self.device),
                                k.shape[1])
        return self._cache[key]

    def nearest(self, in_size: int, out_size: int) -> torch.Tensor:
        key = ("n", in_size, out_size)
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(nearest_table(in_size, out_size).copy()).to(self.device)
        return self._cache[key]


def resize_bilinear_u8(x: torch.Tensor, out_h: int, out_w: int, tables: _Tables, roundtrip: bool) -> Tuple[torch.Tensor, bool]:
    """PIL Image.resize((out_w, out_h), BILINEAR) of a (N, h, w) uint8 device batch (horizontal pass, then
    vertical, each only when that size changes, as Pillow does).  `roundtrip` applies the dataset's
    u8 -> float -> u8 truncation to the source pixels of the first pass; returns (result, still_pending)."""
    N, h, w = x.shape
    cur, rt = x, roundtrip
    if w != out_w:
        b, k, ks = tables.bilinear(w, out_w)
        out = torch.empty(N, h, out_w, dtype=torch.uint8, device=x.device)
        L.call("unet_resample_u8", 1, N, h, w, out_w, vp(cur), int(rt), vp(b), vp(k), ks, vp(out), stream())
        cur, rt = out, False
    if h != out_h:
        b, k, ks = tables.bilinear(h, out_h)
        out = torch.empty(N, out_h, out_w, dtype=torch.uint8, device=x.device)
        L.call("unet_resample_u8", 0, N, h, out_w, out_h, vp(cur), int(rt), vp(b), vp(k), ks, vp(out), stream())
        cur, rt = out, False
    return cur, rt


class GpuSliceTransform:
    """`apply_basic_transforms(image, mask, img_size, mean, std, is_train)` (augmentations.py:119-171) for a
    batch of decoded slices, on the GPU.  images / masks: uint8 (N, h, w) (host or device; the 8-bit
    'L' decode of the PNGs, as dataset.py:146-147 reads them); flips: bool (N,) or None (no flip: the
    validation path)."""

    def __init__(self, img_size: int = 256, mean: float = 0.5, std: float = 0.5, device="cuda"):
        self.img_size = int(img_size)
        self.mean, self.std = float(mean), float(std)
        self.device = torch.device(device)
        self.tables = _Tables(self.device)

    def __call__(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None,
                 flips: Optional[Sequence[bool]] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        x = torch.as_tensor(images)
        if x.dim() == 2:
            x = x[None]
        if x.dtype != torch.uint8 or x.dim() != 3:
            raise RuntimeError(f"expected uint8 images (N, H, W), got {x.dtype} {tuple(x.shape)}")
        x = x.to(self.device, non_blocking=True).contiguous()
        require_device(x, "images")
        N, h, w = x.shape
        S = self.img_size
        r, pending = resize_bilinear_u8(x, S, S, self.tables, roundtrip=True)
        fl = None
        if flips is not None:
            fl = torch.as_tensor(np.asarray(flips, dtype=np.uint8)).to(self.device, non_blocking=True)
            if fl.numel() != N:
                raise RuntimeError(f"{fl.numel()} flip flags for {N} images")
        img = torch.empty(N, 1, S, S, dtype=torch.float32, device=self.device)
        mk, mask_out, yt, xt, mh, mw = None, None, None, None, 0, 0
        if masks is not None:
            mk = torch.as_tensor(masks)
            if mk.dim() == 2:
                mk = mk[None]
            if mk.dtype != torch.uint8 or mk.shape[0] != N:
                raise RuntimeError(f"expected uint8 masks (N, H, W), got {mk.dtype} {tuple(mk.shape)}")
            mk = mk.to(self.device, non_blocking=True).contiguous()
            mh, mw = mk.shape[1], mk.shape[2]
            yt, xt = self.tables.nearest(mh, S), self.tables.nearest(mw, S)
            mask_out = torch.empty(N, S, S, dtype=torch.int64, device=self.device)
        L.call("unet_slice_finish", N, S, S, vp(r), int(pending), mh, mw, vp(mk), vp(yt), vp(xt), vp(fl), self.mean,
               self.std, vp(img), vp(mask_out), stream())
        return img, mask_out


# ------------------------------------------------------------------------------------------------
# training augmentation (csrc/augment.hip)
# ------------------------------------------------------------------------------------------------

# one row per sample; the byte layout of `unet_aug_params` (include/unet_hip.h), uploaded as it is
AUG_DTYPE = np.dtype([("flags", "<u4"), ("inv_affine", "<f4", (6,)), ("gx", "<f4", (6,)), ("gy", "<f4", (6,)),
                      ("contrast", "<f4"), ("brightness", "<f4"), ("noise_sigma", "<f4"), ("key", "<u4", (2,)),
                      ("n_holes", "<i4"), ("holes", "<i4", (4, 4)), ("elastic_slot", "<i4")])
# the raw fp64 draws behind a row's inverse affine matrix (draw_train_augment(..., return_raw=True))
AUG_RAW_DTYPE = np.dtype([("theta", "<f8"), ("sx", "<f8"), ("sy", "<f8"), ("tx", "<f8"), ("ty", "<f8")])
AUG_DRAWS = 45          # uniforms consumed per sample, whatever fires
GRID_STEPS = 5          # GridDistortion(num_steps=5)
MAX_HOLES = 4


def affine_matrices(theta_deg: float, sx: float, sy: float, tx: float, ty: float, img_size: int):
    """(A, A^-1) as fp64 3x3 matrices, A = T(c + t) R(theta) diag(sx, sy) T(-c), c = ((S-1)/2, (S-1)/2):
    rotate and scale about the frame centre, then translate by t pixels.  A maps a source position to
    where it lands in the output; the kernels walk A^-1."""
    c = (img_size - 1) / 2.0
    th = np.deg2rad(theta_deg)
    M = np.array([[np.cos(th) * sx, -np.sin(th) * sy], [np.sin(th) * sx, np.cos(th) * sy]], np.float64)
    A = np.eye(3)
    A[:2, :2] = M
    A[:2, 2] = np.array([c + tx, c + ty]) - M @ np.array([c, c])
    Mi = np.array([[M[1, 1], -M[0, 1]], [-M[1, 0], M[0, 0]]]) / (M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0])
    Ai = np.eye(3)
    Ai[:2, :2] = Mi
    Ai[:2, 2] = np.array([c, c]) - Mi @ np.array([c + tx, c + ty])
    return A, Ai


def gaussian_taps(sigma: float) -> np.ndarray:
    """fp64 taps of the normalised Gaussian of radius int(4 sigma + 0.5) (scipy gaussian_filter, truncate=4)"""
    R = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return w / w.sum()


def draw_train_augment(n: int, img_size: int, rng: np.random.Generator, p_flip: float = 0.5, p_rotate: float = 0.5,
                       rotation_limit: float = 15, p_elastic: float = 0.3, p_brightness: float = 0.3,
                       p_vflip: float = 0.3, p_affine: float = 0.5, p_grid: float = 0.3, p_noise: float = 0.2,
                       p_dropout: float = 0.1, return_raw: bool = False):
    """The random decisions of `get_train_transforms` (augmentations.py:26-89) for n samples, as one AUG_DTYPE
    row each.  Defaults are the reference's, including its quirk that `p_rotate` is accepted and ignored
    (its Affine always has p = 0.5, here `p_affine`).

    Each sample consumes exactly AUG_DRAWS = 45 uniforms `rng.random()` in this order, whether or not a
    transform fires, so a sample's row depends on the seed and its index only (not on n, not on what fired
    for other samples), and every value is stored whether or not its flag is set:
       0 horizontal flip (u < p_flip)      1 vertical flip (u < p_vflip)       2 affine (u < p_affine)
       3 theta ~ U(-rotation_limit, rotation_limit) degrees      4, 5 sx, sy ~ U(0.85, 1.15)
       6, 7 tx, ty ~ U(-0.1, 0.1) * S      8 elastic (u < p_elastic)           9 grid distortion (u < p_grid)
      10-14 / 15-19 the grid's five x / y steps S/5 * (1 + U(-0.2, 0.2)); knots = their running sum,
            rescaled so that the last one is S
      20 brightness/contrast (u < p_brightness)    21 contrast 1 + U(-0.15, 0.15)    22 brightness U(-0.15, 0.15)
      23 noise (u < p_noise)               24 noise sigma ~ U(0.01, 0.02)
      25 dropout (u < p_dropout)           26 hole count 1..4
      27-42 per hole: height, width = round(U(0.03, 0.06) * S), then top, left uniform over the positions
            that keep the hole inside the frame
      43, 44 the two Philox key words, floor(u * 2^32)
    `elastic_slot` numbers the samples whose elastic flag is set, in order (-1 otherwise)."""
    S = int(img_size)
    u = rng.random((int(n), AUG_DRAWS))
    tab = np.zeros(int(n), AUG_DTYPE)
    raw = np.zeros(int(n), AUG_RAW_DTYPE)
    uni = lambda col, lo, hi: lo + (hi - lo) * u[:, col]
    flags = np.zeros(int(n), np.uint32)
    for col, p, bit in ((0, p_flip, L.AUG_HFLIP), (1, p_vflip, L.AUG_VFLIP), (2, p_affine, L.AUG_AFFINE),
                        (8, p_elastic, L.AUG_ELASTIC), (9, p_grid, L.AUG_GRID), (20, p_brightness, L.AUG_BRIGHTNESS),
                        (23, p_noise, L.AUG_NOISE), (25, p_dropout, L.AUG_DROPOUT)):
        flags |= np.where(u[:, col] < p, np.uint32(bit), np.uint32(0))
    tab["flags"] = flags
    raw["theta"] = uni(3, -float(rotation_limit), float(rotation_limit))
    raw["sx"], raw["sy"] = uni(4, 0.85, 1.15), uni(5, 0.85, 1.15)
    raw["tx"], raw["ty"] = uni(6, -0.1, 0.1) * S, uni(7, -0.1, 0.1) * S
    for i in range(int(n)):
        r = raw[i]
        tab["inv_affine"][i] = affine_matrices(r["theta"], r["sx"], r["sy"], r["tx"], r["ty"], S)[1][:2].reshape(6)
    for name, c0 in (("gx", 10), ("gy", 15)):
        steps = S / GRID_STEPS * (1.0 + (-0.2 + 0.4 * u[:, c0:c0 + GRID_STEPS]))
        knots = np.concatenate([np.zeros((int(n), 1)), np.cumsum(steps, axis=1)], axis=1)
        tab[name] = knots * (S / knots[:, -1:])
    tab["contrast"], tab["brightness"] = 1.0 + uni(21, -0.15, 0.15), uni(22, -0.15, 0.15)
    tab["noise_sigma"] = uni(24, 0.01, 0.02)
    tab["n_holes"] = 1 + np.minimum((u[:, 26] * MAX_HOLES).astype(np.int64), MAX_HOLES - 1)
    for h in range(MAX_HOLES):
        c0 = 27 + 4 * h
        hh = np.rint(uni(c0, 0.03, 0.06) * S).astype(np.int64)
        hw = np.rint(uni(c0 + 1, 0.03, 0.06) * S).astype(np.int64)
        y0 = (u[:, c0 + 2] * (S - hh + 1)).astype(np.int64)
        x0 = (u[:, c0 + 3] * (S - hw + 1)).astype(np.int64)
        tab["holes"][:, h] = np.stack([x0, y0, x0 + hw, y0 + hh], axis=1)
    tab["key"] = np.minimum((u[:, 43:45] * 4294967296.0).astype(np.uint64), 4294967295).astype(np.uint32)
    el = (flags & L.AUG_ELASTIC) != 0
    tab["elastic_slot"] = np.where(el, np.cumsum(el) - 1, -1)
    return (tab, raw) if return_raw else tab


class GpuTrainAugment:
    """`get_train_transforms(img_size, mean, std, ...)` (augmentations.py:26-89) for a batch of decoded slices,
    on the GPU: resize, two flips, affine, elastic, grid distortion, brightness/contrast, Gaussian noise,
    coarse dropout, normalise.  images / masks: uint8 (N, h, w) as for GpuSliceTransform; params: the
    AUG_DTYPE table of draw_train_augment (one row per image), or None = every augmentation off, which
    equals GpuSliceTransform(...)(images, masks, flips=None) bit for bit.  Only the PNG decode and the
    random draws stay on the host; the device work is deterministic given the table.

        aug = GpuTrainAugment(img_size=512)
        images, masks = aug(u8_slices, u8_masks, aug.draw(len(u8_slices), rng))

    Semantics (tests/aug_ref.py restates them in fp64):

    * Resize: the image goes to S x S through resize_bilinear_u8 (PIL's 8-bit BILINEAR, exact); the mask is
      read through the PIL NEAREST tables and never materialised at S x S.  The reference resizes with OpenCV
      in float, so for h, w != S results differ from it by the 8-bit quantisation of this step.
    * One resample for the whole geometric chain.  The reference applies flips, Affine, ElasticTransform and
      GridDistortion one after another, each resampling (image bilinear, mask nearest); here they are
      composed into one coordinate map with one bilinear image fetch and one nearest mask fetch (sharper
      than three interpolations: a stated difference).  For output pixel p = (x, y):
        1. grid distortion q = (gx(x), gy(y)): separable, piecewise linear, knots at output positions
           k S/5, k = 0..5, source knots from the table (off: identity);
        2. elastic r = q + d(q): the sample's field (dx, dy), fetched bilinearly at q with coordinates
           clamped to the frame (off: d = 0);
        3. affine s = A^-1 r, the table's fp32 2x3 matrix (off: identity);
        4. flips: the vertical, then the horizontal flip mirror s exactly (x -> S-1-x); the reference runs
           them before the affine, which makes them innermost here;
        5. image: a bilinear sample of the resized u8 image / 255 at s, taps outside the frame contribute 0
           (scipy map_coordinates(order=1, mode='grid-constant', cval=0));
        6. mask: mask[ytab[iy]][xtab[ix]] > 127 at (ix, iy) = floor(s + 0.5); 0 outside [0, S).
      No intermediate frame clipping: the image is zero outside its frame throughout the chain.
    * Elastic field: d = alpha * G_sigma * u, u i.i.d. uniform on [-1, 1) per pixel and component, G_sigma a
      separable normalised Gaussian of radius R = int(4 sigma + 0.5) with the reflect-101 border (scipy
      gaussian_filter(mode='mirror', truncate=4)).  Generated only for the flagged samples, as a compact
      fp32 [n_elastic][2][S][S] buffer.  Needs S > R.
    * Photometric chain on v in [0, 1], in the reference's order: v = clip(contrast v + brightness, 0, 1);
      v = clip(v + sigma n, 0, 1) with n a per-pixel standard normal; up to 4 axis-aligned holes set to 0
      (the mask is left untouched, as in the reference); (v - mean) / std in fp32.
    * Device random numbers: Philox4x32-10 keyed by the row's two key words, counter (y S + x, stream, 0, 0),
      stream 0 = noise, 1 = elastic dx, 2 = elastic dy.  u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24,
      n = sqrt(-2 ln u1) cos(2 pi u2); the field uniform is (w0 >> 8) 2^-23 - 1."""

    def __init__(self, img_size: int = 256, mean: float = 0.5, std: float = 0.5, device="cuda", alpha: float = 50.0,
                 sigma: float = 10.0, **draw_options):
        self.img_size = int(img_size)
        self.mean, self.std = float(mean), float(std)
        self.device = torch.device(device)
        self.alpha, self.sigma = float(alpha), float(sigma)
        self.radius = int(4.0 * self.sigma + 0.5)
        self.draw_options = dict(draw_options)
        draw_train_augment(0, self.img_size, np.random.default_rng(0), **self.draw_options)   # rejects unknown options
        self.tables = _Tables(self.device)
        self._taps = None

    def draw(self, n: int, rng: np.random.Generator) -> np.ndarray:
        """draw_train_augment with this transform's size, probabilities and limits"""
        return draw_train_augment(n, self.img_size, rng, **self.draw_options)

    def elastic_fields(self, table_dev: torch.Tensor, slots_dev: torch.Tensor, n_rows: int) -> torch.Tensor:
        """fp32 [len(slots)][2][S][S] displacement fields of the table rows listed in slots_dev"""
        S, R = self.img_size, self.radius
        if S <= R:
            raise RuntimeError(f"elastic transform needs img_size > int(4 sigma + 0.5) = {R}, got {S}")
        if self._taps is None:
            self._taps = torch.from_numpy(gaussian_taps(self.sigma).astype(np.float32)).to(self.device)
        ne = slots_dev.numel()
        buf = torch.empty(2, ne, 2, S, S, dtype=torch.float32, device=self.device)
        L.call("unet_aug_elastic_field", ne, S, self.alpha, R, vp(self._taps), n_rows, vp(table_dev), vp(slots_dev),
               vp(buf[0]), vp(buf[1]), stream())
        return buf[1]

    def __call__(self, images: torch.Tensor, masks: Optional[torch.Tensor] = None,
                 params: Optional[np.ndarray] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        x = torch.as_tensor(images)
        if x.dim() == 2:
            x = x[None]
        if x.dtype != torch.uint8 or x.dim() != 3:
            raise RuntimeError(f"expected uint8 images (N, H, W), got {x.dtype} {tuple(x.shape)}")
        N, S = x.shape[0], self.img_size
        if params is None:
            tab = np.zeros(N, AUG_DTYPE)
        else:
            tab = np.array(params, dtype=AUG_DTYPE, copy=True).reshape(-1)
            if tab.shape[0] != N:
                raise RuntimeError(f"{tab.shape[0]} parameter rows for {N} images")
        el = np.nonzero(tab["flags"] & L.AUG_ELASTIC)[0].astype(np.int32)
        if el.size and S <= self.radius:
            raise RuntimeError(f"elastic transform needs img_size > int(4 sigma + 0.5) = {self.radius}, got {S}")
        tab["elastic_slot"] = -1
        tab["elastic_slot"][el] = np.arange(el.size, dtype=np.int32)
        x = x.to(self.device, non_blocking=True).contiguous()
        require_device(x, "images")
        # the table and the compact elastic sample list travel in one H2D copy
        host = np.concatenate([tab.view(np.uint8), el.view(np.uint8)])
        dev = torch.from_numpy(host).to(self.device, non_blocking=True)
        table_dev, slots_dev = dev[:tab.nbytes], dev[tab.nbytes:]
        r, _ = resize_bilinear_u8(x, S, S, self.tables, roundtrip=False)
        field = self.elastic_fields(table_dev, slots_dev.view(torch.int32), N) if el.size else None
        img = torch.empty(N, 1, S, S, dtype=torch.float32, device=self.device)
        mk, mask_out, yt, xt, mh, mw = None, None, None, None, 0, 0
        if masks is not None:
            mk = torch.as_tensor(masks)
            if mk.dim() == 2:
                mk = mk[None]
            if mk.dtype != torch.uint8 or mk.dim() != 3 or mk.shape[0] != N:
                raise RuntimeError(f"expected uint8 masks (N, H, W), got {mk.dtype} {tuple(mk.shape)}")
            mk = mk.to(self.device, non_blocking=True).contiguous()
            mh, mw = mk.shape[1], mk.shape[2]
            yt, xt = self.tables.nearest(mh, S), self.tables.nearest(mw, S)
            mask_out = torch.empty(N, S, S, dtype=torch.int64, device=self.device)
        L.call("unet_aug_apply", N, S, vp(r), mh, mw, vp(mk), vp(yt), vp(xt), vp(table_dev), N, vp(field), int(el.size),
               self.mean, self.std, vp(img), vp(mask_out), stream())
        return img, mask_out


assert AUG_DTYPE.itemsize == ctypes.sizeof(L.AugParams)
