"""Surface-distance metrics on the device (csrc/surface.hip, unet.utils.metrics.surface_distances) against a
brute-force fp64 reference: surfaces by the padded 4-neighbour test, all pairwise distances between the two
surfaces, np.max / np.percentile / mean, NaN where a surface is empty.

Tolerances.  Unit spacing: every squared distance is an exact fp32 integer, so only the fp64 sqrt,
interpolation and sum order differ: 1e-12 relative.  Anisotropic spacing: a candidate wy dy^2 + wx dx^2 carries at
most four roundings of 2^-24, the minimum and any order statistic keep that bound, so |dd| <= 2 * 2^-24 d: gate
3 * 2^-24 relative plus 1e-12."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DIST = ("hd", "hd_percentile", "assd")
UNIT, ANISO = 1e-12, 3 * 2.0 ** -24


def _surface(A, spacing):
    p = np.pad(A, 1)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return np.argwhere(A & ~inner) * np.asarray(spacing, dtype=np.float64)


def reference(P, T, K, spacing=(1.0, 1.0), q=95.0):
    N = P.shape[0]
    out = {k: np.full((N, K), np.nan) for k in DIST}
    out["n_pred"], out["n_true"] = np.zeros((N, K), np.int64), np.zeros((N, K), np.int64)
    for n in range(N):
        for c in range(K):
            a, b = _surface(P[n] == c, spacing), _surface(T[n] == c, spacing)
            out["n_pred"][n, c], out["n_true"][n, c] = len(a), len(b)
            if len(a) and len(b):
                D = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
                ab, ba = D.min(1), D.min(0)
                out["hd"][n, c] = max(ab.max(), ba.max())
                out["hd_percentile"][n, c] = max(np.percentile(ab, q), np.percentile(ba, q))
                out["assd"][n, c] = (ab.sum() + ba.sum()) / (len(a) + len(b))
    return out


def check(got, ref, rel, absolute=0.0):
    for k in ("n_pred", "n_true"):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    for k in DIST:
        g, r = got[k].cpu().numpy(), ref[k]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(r)), k
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        print(k, "max err", err.max(initial=0.0), "max rel", (err / np.maximum(r[ok], 1e-300)).max(initial=0.0))
        assert np.all(err <= rel * np.abs(r[ok]) + absolute), k


def blobs(N, K, H, W, seed):
    """Nearest-neighbour-upsampled coarse random labels (P, T); class K-1 is absent from the prediction of image 0
    when K > 2, and a few targets are out of range (255)."""
    rng = np.random.default_rng(seed)
    def up():
        c = rng.integers(0, K, (N, -(-H // 8), -(-W // 8)))
        return np.repeat(np.repeat(c, 8, 1), 8, 2)[:, :H, :W].copy()
    P, T = up(), up()
    if K > 2:
        P[0][P[0] == K - 1] = 0
    T.reshape(-1)[rng.integers(0, T.size, 5)] = 255
    return P, T


SHAPES = [(3, 4, 37, 70), (2, 16, 33, 130), (1, 2, 64, 64), (2, 5, 1, 200), (1, 3, 70, 1)]


@pytest.mark.parametrize("as_logits", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_blobs_match_bruteforce(shape, as_logits):
    from unet.utils.metrics import surface_distances
    N, K, H, W = shape
    P, T = blobs(N, K, H, W, seed=sum(shape))
    if as_logits:
        z = np.random.default_rng(1).standard_normal((N, K, H, W)).astype(np.float32) * 0.1
        z += 3.0 * (P[:, None] == np.arange(K)[None, :, None, None])
        z[0, :, 0, 0] = 0.25                      # a tie: the first maximum wins
        pred, P = torch.from_numpy(z).cuda(), z.argmax(1)
    else:
        pred = torch.from_numpy(P).cuda()
    ref = reference(P, T, K)
    assert np.isnan(ref["hd"]).any() == (K > 2) and not np.isnan(ref["hd"]).all()
    check(surface_distances(pred, torch.from_numpy(T).cuda(), K), ref, UNIT)


def _hand_built(name, H=40, W=72):
    P, T = np.zeros((1, H, W), np.int64), np.zeros((1, H, W), np.int64)
    if name == "identical":
        P[0, 5:20, 7:50] = 1
        T[:] = P
    elif name == "fills_frame":                    # class 1 everywhere in P: its surface is the frame border
        P[:] = 1
        T[0, 10:30, 20:60] = 1
    elif name == "far_corners":                    # full-width window search, percentile of one element
        P[0, 0, 0] = 1
        T[0, H - 1, W - 1] = 1
    elif name == "touching_edges":
        P[0, :, :3] = 1; P[0, :2, :] = 1; P[0, :, -1] = 1; P[0, -4:, :] = 1
        T[0, 3:, 5:] = 1
    elif name == "concentric":                     # many tied distances for the select
        P[0, 4:36, 6:66] = 1
        T[0, 12:28, 14:58] = 1
    return P, T


@pytest.mark.parametrize("name", ["identical", "fills_frame", "far_corners", "touching_edges", "concentric"])
def test_hand_built_masks(name):
    from unet.utils.metrics import surface_distances
    P, T = _hand_built(name)
    ref = reference(P, T, 2)
    assert not np.isnan(ref["hd"][:, 1]).any()
    if name == "identical":
        assert not ref["hd"].any()
    check(surface_distances(torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda(), 2), ref, UNIT)


def test_exactness_limit():
    """2 x 2048 with one surface pixel at each far corner: d^2 = 2047^2 + 1, the largest exact case."""
    from unet.utils.metrics import surface_distances
    P, T = np.full((1, 2, 2048), 7, np.int64), np.full((1, 2, 2048), 7, np.int64)
    P[0, 0, 0] = 0
    T[0, 1, 2047] = 0
    got = surface_distances(torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda(), 1)
    check(got, reference(P, T, 1), UNIT)
    assert float(got["hd"][0, 0]) == np.sqrt(np.float64(2047 ** 2 + 1))


@pytest.mark.parametrize("q", [95.0, 50.0, 100.0])
def test_anisotropic_spacing(q):
    from unet.utils.metrics import surface_distances
    P, T = blobs(3, 4, 37, 70, seed=5)
    got = surface_distances(torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda(), 4, spacing=(2.5, 0.7), percentile=q)
    check(got, reference(P, T, 4, (2.5, 0.7), q), ANISO, 1e-12)


def test_two_calls_are_bit_identical():
    from unet.utils.metrics import surface_distances
    P, T = blobs(2, 16, 33, 130, seed=9)
    p, t = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    a, b = surface_distances(p, t, 16, (2.5, 0.7)), surface_distances(p, t, 16, (2.5, 0.7))
    for k in a:
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k


def test_accumulator_means():
    """Two updates (device labels, then host logits-free labels); class 3 never predicted: NaN and left out."""
    from unet.utils.metrics import SurfaceDistanceMetrics
    K, names = 4, ["bg", "a", "b", "c"]
    batches = [blobs(2, K, 37, 70, seed=21), blobs(3, K, 37, 70, seed=22)]
    for P, _ in batches:
        P[P == 3] = 0
    m = SurfaceDistanceMetrics(K, names)
    m.update(torch.from_numpy(batches[0][0]).cuda(), torch.from_numpy(batches[0][1]).cuda())
    m.update(torch.from_numpy(batches[1][0]), torch.from_numpy(batches[1][1]))
    refs = [reference(P, T, K) for P, T in batches]
    res = m.compute()
    for key, rk in (("hd", "hd"), ("hd95", "hd_percentile"), ("assd", "assd")):
        per = np.nanmean(np.concatenate([r[rk] for r in refs])[:, :3], axis=0)
        got = res[f"class_{key}"]
        assert list(got) == names and np.isnan(got["c"])
        assert np.allclose([got[n] for n in names[:3]], per, rtol=1e-12, atol=0)
        assert res[f"mean_{key}"] == pytest.approx(per[1:].mean(), rel=1e-12)
    with_bg = SurfaceDistanceMetrics(K, names, include_background=True)
    with_bg.update(torch.from_numpy(batches[0][0]), torch.from_numpy(batches[0][1]))
    assert with_bg.compute()["mean_hd"] == pytest.approx(np.nanmean(refs[0]["hd"][:, :3], axis=0).mean(), rel=1e-12)
    m.reset()
    assert np.isnan(m.compute()["mean_assd"])
