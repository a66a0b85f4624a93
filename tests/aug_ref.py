"""CPU restatement of the device training augmentation (TEST INFRASTRUCTURE ONLY): numpy + Pillow, written
from the semantics in GpuTrainAugment's docstring / DESIGN.md §10, from a parameter-table row.

* `philox4x32_10`: Philox4x32-10 in numpy (uint64 arithmetic).
* `elastic_field`, `train_augment`: the chain in `dtype` arithmetic.  dtype=np.float64 is the reference the
  kernels are tested against; dtype=np.float32 does all coordinate and value arithmetic in fp32 (one
  rounding per operation, no fused multiply-add) and is used only to measure tolerances: how far fp32
  arithmetic alone moves a result from the fp64 one.
The output stage is the same in both modes and is part of the definition: v is rounded to fp32 and
(v - mean) / std is done in fp32, as apply_basic_transforms does (image_finish_kernel on the device)."""

from __future__ import annotations

import numpy as np
from PIL import Image

HFLIP, VFLIP, AFFINE, ELASTIC, GRID, BRIGHTNESS, NOISE, DROPOUT = 1, 2, 4, 8, 16, 32, 64, 128
ALL_FLAGS = 255
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 output words per counter (c0..c3 broadcastable arrays), key (k0, k1)."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK32 for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK32]
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK32, (k1 + np.uint64(_W1)) & _MASK32
    return [v.astype(np.uint32) for v in c]


def field_uniform(S: int, key, comp: int) -> np.ndarray:
    """u on [-1, 1) for displacement component comp (0 = dx, 1 = dy): exact in fp32, returned as fp64"""
    w0 = philox4x32_10(np.arange(S * S, dtype=np.uint64), 1 + comp, 0, 0, key[0], key[1])[0]
    return ((w0 >> 8).astype(np.float64) * 2.0 ** -23 - 1.0).reshape(S, S)


def noise_normal(S: int, key, dtype=np.float64) -> np.ndarray:
    F = dtype
    w = philox4x32_10(np.arange(S * S, dtype=np.uint64), 0, 0, 0, key[0], key[1])
    u1 = (((w[0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24).astype(F)      # exact in fp32
    u2 = ((w[1] >> 8).astype(np.float64) * 2.0 ** -24).astype(F)
    two_pi = F(6.2831855) if F is np.float32 else F(2.0 * np.pi)
    return (np.sqrt(F(-2.0) * np.log(u1)) * np.cos(two_pi * u2)).reshape(S, S)


def gaussian_taps(sigma: float) -> np.ndarray:
    R = int(4.0 * sigma + 0.5)
    x = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x * x)
    return w / w.sum()


def _blur_rows(a: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """sum_k taps[k] * a[:, reflect(x - R + k)], accumulated tap by tap in a's dtype"""
    R = (len(taps) - 1) // 2
    S = a.shape[1]
    p = np.pad(a, ((0, 0), (R, R)), mode="reflect")       # reflect-101
    acc = np.zeros_like(a)
    for k in range(2 * R + 1):
        acc = acc + taps[k] * p[:, k:k + S]
    return acc


def elastic_field(S: int, key, alpha: float = 50.0, sigma: float = 10.0, dtype=np.float64) -> np.ndarray:
    """(2, S, S) displacement (dx, dy) = alpha * G_sigma * u; horizontal pass first, then vertical"""
    F = dtype
    taps = gaussian_taps(sigma).astype(np.float32).astype(F) if F is np.float32 else gaussian_taps(sigma)
    assert S > (len(taps) - 1) // 2
    out = []
    for comp in range(2):
        u = field_uniform(S, key, comp).astype(F)
        h = _blur_rows(u, taps)
        v = _blur_rows(np.ascontiguousarray(h.T), taps).T
        out.append(F(alpha) * v)
    return np.stack(out)


def _grid_map(g: np.ndarray, idx: np.ndarray, S: int, F) -> np.ndarray:
    k = np.minimum(5 * idx // S, 4)
    cell = F(S) / F(5)
    t = (idx.astype(F) - k.astype(F) * cell) / cell
    return g[k] + t * (g[k + 1] - g[k])


def _bilinear_clamped(f: np.ndarray, qx: np.ndarray, qy: np.ndarray, F) -> np.ndarray:
    S = f.shape[0]
    cx, cy = np.clip(qx, F(0), F(S - 1)), np.clip(qy, F(0), F(S - 1))
    x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
    fx, fy = cx - x0.astype(F), cy - y0.astype(F)
    top = f[y0, x0] + fx * (f[y0, x1] - f[y0, x0])
    bot = f[y1, x0] + fx * (f[y1, x1] - f[y1, x0])
    return top + fy * (bot - top)


def resized_inputs(img_u8: np.ndarray, mask_u8: np.ndarray, S: int):
    """the S x S uint8 image (PIL BILINEAR) and the S x S binary mask ((mask > 127), PIL NEAREST)"""
    r = np.asarray(Image.fromarray(np.asarray(img_u8, np.uint8)).resize((S, S), Image.BILINEAR))
    m = np.asarray(Image.fromarray((np.asarray(mask_u8) > 127).astype(np.uint8)).resize((S, S), Image.NEAREST))
    return r, m.astype(np.int64)


def source_coordinates(S: int, row, field, dtype=np.float64):
    """the composed coordinate map: (sx, sy) in the resized image for every output pixel"""
    F = dtype
    flags = int(row["flags"])
    ys, xs = np.mgrid[:S, :S]
    cx, cy = xs.astype(F), ys.astype(F)
    if flags & GRID:
        cx = _grid_map(np.asarray(row["gx"]).astype(F), xs, S, F)
        cy = _grid_map(np.asarray(row["gy"]).astype(F), ys, S, F)
    if flags & ELASTIC:
        dx, dy = _bilinear_clamped(field[0], cx, cy, F), _bilinear_clamped(field[1], cx, cy, F)
        cx, cy = cx + dx, cy + dy
    if flags & AFFINE:
        a = np.asarray(row["inv_affine"]).astype(F)
        cx, cy = a[0] * cx + a[1] * cy + a[2], a[3] * cx + a[4] * cy + a[5]
    if flags & VFLIP:
        cy = F(S - 1) - cy
    if flags & HFLIP:
        cx = F(S - 1) - cx
    return cx, cy


def train_augment(img_u8: np.ndarray, mask_u8: np.ndarray, S: int, row, alpha: float = 50.0, sigma: float = 10.0,
                  mean: float = 0.5, std: float = 0.5, dtype=np.float64, field=None):
    """One sample through the chain.  Returns (image float32 (S, S), mask int64 (S, S), (sx, sy)): the source
    coordinates are what the mask comparison needs to find the pixels whose nearest fetch sits on a tie."""
    F = dtype
    flags = int(row["flags"])
    r, m = resized_inputs(img_u8, mask_u8, S)
    if flags & ELASTIC and field is None:
        field = elastic_field(S, row["key"], alpha, sigma, F)
    cx, cy = source_coordinates(S, row, field, F)

    t = np.zeros((S + 2, S + 2), F)                 # /255 image with a zero frame (constant border 0)
    t[1:-1, 1:-1] = r.astype(F) / F(255)

    def tap(xi, yi):
        return t[np.clip(yi, -1, S) + 1, np.clip(xi, -1, S) + 1]

    fx0, fy0 = np.floor(cx), np.floor(cy)
    fx, fy = cx - fx0, cy - fy0
    x0, y0 = np.clip(fx0, -2, S).astype(np.int64), np.clip(fy0, -2, S).astype(np.int64)
    top = tap(x0, y0) + fx * (tap(x0 + 1, y0) - tap(x0, y0))
    bot = tap(x0, y0 + 1) + fx * (tap(x0 + 1, y0 + 1) - tap(x0, y0 + 1))
    v = top + fy * (bot - top)

    ix = np.clip(np.floor(cx + F(0.5)), -1, S).astype(np.int64)
    iy = np.clip(np.floor(cy + F(0.5)), -1, S).astype(np.int64)
    inside = (ix >= 0) & (ix < S) & (iy >= 0) & (iy < S)
    mask = np.where(inside, m[np.clip(iy, 0, S - 1), np.clip(ix, 0, S - 1)], 0).astype(np.int64)

    if flags & BRIGHTNESS:
        v = np.clip(F(row["contrast"]) * v + F(row["brightness"]), F(0), F(1))
    if flags & NOISE:
        v = np.clip(v + F(row["noise_sigma"]) * noise_normal(S, row["key"], F), F(0), F(1))
    if flags & DROPOUT:
        for h in range(int(row["n_holes"])):
            x0h, y0h, x1h, y1h = (int(q) for q in row["holes"][h])
            v[y0h:y1h, x0h:x1h] = 0
    out = (v.astype(np.float32) - np.float32(mean)) / np.float32(std)
    return out.astype(np.float32), mask, (cx, cy)


def tie_pixels(cx: np.ndarray, cy: np.ndarray, eps: float = 1e-3) -> np.ndarray:
    """pixels whose source coordinate has a fractional part within eps of 0.5 in either axis: there the
    nearest fetch floor(s + 0.5) is decided by the last bits of s"""
    fx, fy = cx - np.floor(cx), cy - np.floor(cy)
    return (np.abs(fx - 0.5) <= eps) | (np.abs(fy - 0.5) <= eps)
