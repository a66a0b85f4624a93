"""Connected components on the device (csrc/cc.hip, unet.utils.connected_components / filter_components) against a
plain flood fill.  Every output is an integer function of the input alone (a component's id is the smallest linear
index of its pixels), so every comparison is array_equal: there is no tolerance anywhere."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(2, 3, 70, 130), (1, 16, 64, 64), (3, 4, 37, 70), (1, 2, 1, 200), (1, 2, 130, 1)]
KEYS = ("components", "areas", "classes", "count")


def reference(P, K, conn, background=0):
    """(comp, area, cls, count) by flood fill in raster order: the first pixel met is the smallest linear index."""
    N, H, W = P.shape
    cls = np.where((P >= 0) & (P < K), P, 255).astype(np.uint8)
    comp, area = np.full((N, H, W), -1, np.int32), np.zeros((N, H, W), np.int32)
    count = np.zeros((N, K), np.int64)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for n, y, x in np.ndindex(N, H, W):
        c = cls[n, y, x]
        if c == 255 or c == background or comp[n, y, x] >= 0:
            continue
        comp[n, y, x], stack = y * W + x, [(y, x)]
        while stack:
            py, px = stack.pop()
            area[n, y, x] += 1
            for dy, dx in nb:
                qy, qx = py + dy, px + dx
                if 0 <= qy < H and 0 <= qx < W and cls[n, qy, qx] == c and comp[n, qy, qx] < 0:
                    comp[n, qy, qx] = y * W + x
                    stack.append((qy, qx))
        count[n, c] += 1
    return comp, area, cls, count


def reference_filter(P, K, conn, min_size, keep_largest, background, fill):
    comp, area, cls, _ = reference(P, K, conn, background)
    out = np.full(P.shape, fill, np.int64)
    out[cls == background] = background
    for n in range(P.shape[0]):
        ids = np.flatnonzero(area[n])
        a, c = area[n].flat[ids], cls[n].flat[ids]
        keep = a >= min_size
        if keep_largest:   # the largest of the class, the smaller id on a tie (ids ascend, argmax takes the first)
            keep &= np.array([i == ids[c == k][np.argmax(a[c == k])] for i, k in zip(ids, c)], bool)
        sel = np.isin(comp[n], ids[keep])
        out[n][sel] = cls[n][sel]
    return out


def blobs(N, K, H, W, seed):
    """Nearest-neighbour-upsampled coarse random labels with a few out-of-range values."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, K, (N, -(-H // 8), -(-W // 8)))
    P = np.repeat(np.repeat(c, 8, 1), 8, 2)[:, :H, :W].copy()
    P.reshape(-1)[rng.integers(0, P.size, 5)] = rng.choice([-3, K, 255], 5)
    return P


def noise(N, K, H, W, seed):
    """Per-pixel noise at density 0.59, the site-percolation threshold: the most components, the longest chains."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((N, H, W)) < 0.59, rng.integers(1, max(K, 2), (N, H, W)) % K, 0)


def hand_built(name):
    """(P, count [class 0, class 1] for connectivity 4, the same for 8), all classes labelled (background -1)."""
    if name == "serpentine":   # width 1, (3, 4096): along row 0, down, along row 2, up: crosses every vertical seam
        x = np.arange(4096) % 8
        P = np.stack([x <= 4, x % 4 == 0, (x >= 4) | (x == 0)]).astype(np.int64)[None]
        return P, None, None
    H, W = 130, 200
    P = np.zeros((1, H, W), np.int64)
    if name == "fills_frame":
        P[:] = 1
        return P, [0, 1], [0, 1]
    if name == "checkerboard":
        P[0] = np.add.outer(np.arange(H), np.arange(W)) % 2
        return P, [H * W // 2, H * W // 2], [1, 1]
    if name == "diagonal":     # one pixel wide, through the tile corners (63, 63) -> (64, 64) and (127, 127) -> (128, 128)
        P[0, np.arange(H), np.arange(H)] = 1
        return P, [2, H], [1, 1]
    P[0, 5:100, 10] = P[0, 5:100, 150] = 1      # "u": arms in tile columns 0 and 2, joined only by the bar in tile row 1
    P[0, 100, 10:151] = 1
    return P, [1, 1], [1, 1]


def device(P, K, conn, background=0):
    from unet.utils import connected_components
    out = connected_components(torch.from_numpy(P).cuda(), K, conn, background)
    return [out[k].cpu().numpy() for k in KEYS]


def check(got, ref):
    for k, g, r in zip(KEYS, got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r), k


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("make", [blobs, noise])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_maps_match_flood_fill(shape, make, conn):
    N, K, H, W = shape
    P = make(N, K, H, W, seed=sum(shape))
    check(device(P, K, conn), reference(P, K, conn))


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["fills_frame", "checkerboard", "diagonal", "u", "serpentine"])
def test_hand_built_maps(name, conn):
    P, n4, n8 = hand_built(name)
    ref = reference(P, 2, conn, -1)
    if n4 is None:
        assert ref[3][0, 1] == 1 and ref[1].max() == (P == 1).sum()   # the serpentine is one chain
    else:
        assert ref[3].tolist() == [n4 if conn == 4 else n8]
    check(device(P, 2, conn, -1), ref)


def test_input_forms():
    """Logits with a tie (the first maximum wins), a uint8 mask (byte > 127), background -1."""
    from unet.utils import connected_components
    N, K, H, W = 2, 3, 70, 130
    P = blobs(N, K, H, W, seed=3).clip(0, K - 1)
    z = np.random.default_rng(1).standard_normal((N, K, H, W)).astype(np.float32) * 0.1
    z += 3.0 * (P[:, None] == np.arange(K)[None, :, None, None])
    z[0, :, 0, :9] = 0.25
    out = connected_components(torch.from_numpy(z).cuda(), K, 8, -1)
    assert not out["classes"][0, 0, :9].any()
    check([out[k].cpu().numpy() for k in KEYS], reference(z.argmax(1), K, 8, -1))
    m = np.random.default_rng(2).integers(0, 256, (N, H, W)).astype(np.uint8)
    out = connected_components(torch.from_numpy(m).cuda(), 2, 4)
    check([out[k].cpu().numpy() for k in KEYS], reference((m > 127).astype(np.int64), 2, 4))


@pytest.mark.parametrize("keep_largest", [False, True])
@pytest.mark.parametrize("min_size", [0, 1, 5, 10 ** 9])
def test_filter(min_size, keep_largest):
    from unet.utils import filter_components
    N, K, H, W = 2, 3, 70, 130
    P = noise(N, K, H, W, seed=7)
    P[0, :8] = 0
    P[0, 1:7, 100:110] = P[0, 1:7, 20:30] = P[1, 60:62, 2:12] = 2     # image 0: two class-2 blobs tie in area
    P[0, 1:3, 60:65] = 7                                               # no class
    for bg, fill in ((0, 0), (0, 9), (-1, 5)):
        got = filter_components(torch.from_numpy(P).cuda(), K, min_size, keep_largest, 4, bg, fill)
        ref = reference_filter(P, K, 4, min_size, keep_largest, bg, fill)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref), (bg, fill)
    if keep_largest and min_size <= 5:
        assert (ref[0, 1:7, 20:30] == 2).all() and (ref[0, 1:7, 100:110] == 5).all()   # the smaller id won
    for w in (128, 127):   # 16-byte stores, and the plain path of a size that is no multiple of 16
        m = ((P[:, :, :w] == 1) * 200).astype(np.uint8)
        got = filter_components(torch.from_numpy(m).cuda(), 2, min_size, keep_largest, 8)
        ref = reference_filter((m > 127).astype(np.int64), 2, 8, min_size, keep_largest, 0, 0)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref * 255)


def test_postprocess_masks():
    from unet.utils.inference import postprocess_masks
    z = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 2, 48, 40)).astype(np.float32)).cuda()
    z = torch.nn.functional.avg_pool2d(z, 5, 1, 2)
    plain = postprocess_masks(z, (100, 70), 0.5)
    assert torch.equal(plain, postprocess_masks(z, (100, 70), 0.5, min_size=0, keep_largest=False))
    P = (plain.cpu().numpy() > 127).astype(np.int64)
    for kw in (dict(min_size=30), dict(keep_largest=True, connectivity=4)):
        ref = reference_filter(P, 2, kw.get("connectivity", 8), kw.get("min_size", 0), "keep_largest" in kw, 0, 0)
        assert ref.any() and (ref != P).any()
        assert np.array_equal(postprocess_masks(z, (100, 70), 0.5, **kw).cpu().numpy(), ref * 255)


def test_two_calls_are_bit_identical():
    P = noise(2, 3, 70, 130, seed=11)
    for a, b in zip(device(P, 3, 8), device(P, 3, 8)):
        assert np.array_equal(a, b)
