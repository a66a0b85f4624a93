"""Time unet.utils.surface_distances at 4 x 512^2 label maps, K in {2, 16}, against the host route users have today.

Masks are blob-shaped: the argmax of smooth random fields (a 16 x 16 grid per class, bicubically upsampled); the
prediction is the target's field plus a smaller perturbation, so the two surfaces lie near each other as a trained
model's do.
  (a) device: surface_distances on device label maps, HIP events around blocks of calls, warm-up first, until over
              --seconds of timed work;
  (b) host:   .cpu(), then per image, class and direction scipy's binary_erosion + distance_transform_edt sampled on
              the other surface, max / percentile / mean, the (image, class) pairs spread over 16 worker processes
              (started before the GPU is touched); wall clock, best of --host-reps.
Per-kernel times come from the same process: torch.profiler around a block of calls after the timed section.  Writes
a JSON; needs the GPU: there is no CPU mode.

  python tools/surface_time.py [--out profiles/surface_distance_mi355x.json]"""
import argparse
import json
import multiprocessing as mp
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))


def host_pair(args):
    """One (image, class): both directed distance sets by scipy, then hd, percentile and assd."""
    from scipy import ndimage
    p, t, c, q = args
    A, B = p == c, t == c
    SA, SB = A ^ ndimage.binary_erosion(A), B ^ ndimage.binary_erosion(B)
    if not SA.any() or not SB.any():
        return (np.nan,) * 3
    ab = ndimage.distance_transform_edt(~SB)[SA]
    ba = ndimage.distance_transform_edt(~SA)[SB]
    return (max(ab.max(), ba.max()), max(np.percentile(ab, q), np.percentile(ba, q)),
            (ab.sum() + ba.sum()) / (ab.size + ba.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "surface_distance_mi355x.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per shape")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    pool = mp.get_context("fork").Pool(16)      # before the first GPU call: the workers never open the device

    import torch
    import torch.nn.functional as F
    from unet.utils import surface_distances
    if not torch.cuda.is_available():
        sys.exit("surface_time.py measures on the GPU; none is visible")
    N, H = a.batch, a.size
    gen = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "label_maps": f"{N} x {H} x {H} int64",
           "timing": "HIP events around blocks of 20 calls after 10 warm-up calls; host: wall clock, best of "
                     f"{a.host_reps}, 16 processes", "shapes": {}}
    for K in (2, 16):
        field = torch.randn(N, K, 16, 16, generator=gen)
        noise = torch.randn(N, K, 16, 16, generator=gen)
        t = F.interpolate(field, size=(H, H), mode="bicubic").argmax(1)
        p = F.interpolate(field + 0.3 * noise, size=(H, H), mode="bicubic").argmax(1)
        pd, td = p.cuda(), t.cuda()

        for _ in range(10):
            out = surface_distances(pd, td, K)
        torch.cuda.synchronize()
        ms, calls, block = 0.0, 0, 20
        while ms < a.seconds * 1e3:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                out = surface_distances(pd, td, K)
            e1.record()
            torch.cuda.synchronize()
            ms += e0.elapsed_time(e1)
            calls += block

        host_s = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            pn, tn = pd.cpu().numpy(), td.cpu().numpy()
            vals = pool.map(host_pair, [(pn[n], tn[n], c, 95.0) for n in range(N) for c in range(K)])
            host_s.append(time.perf_counter() - t0)
        ref = np.array(vals).reshape(N, K, 3)
        got = torch.stack([out["hd"], out["hd_percentile"], out["assd"]], -1).cpu().numpy()
        agree = bool(np.allclose(got, ref, rtol=1e-12, atol=0, equal_nan=True))

        kernels = "not measured"
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(block):
                    surface_distances(pd, td, K)
                torch.cuda.synchronize()
            kernels = {e.key.split("(")[0].replace("void unet::", ""): round(e.device_time_total / e.count, 2)
                       for e in prof.key_averages() if "surface_" in e.key}
        except Exception as exc:  # the tracer is optional: the end-to-end figures stand without it
            kernels = f"not measured ({type(exc).__name__})"

        per = ms / calls
        res["shapes"][f"K{K}"] = {
            "surface_pixels": int(out["n_pred"].sum() + out["n_true"].sum()),
            "device_ms_per_call": round(per, 4), "calls_timed": calls, "timed_ms": round(ms, 1),
            "host_ms_per_call": round(min(host_s) * 1e3, 2), "host_ms_all": [round(s * 1e3, 2) for s in host_s],
            "host_over_device": round(min(host_s) * 1e3 / per, 1), "agrees_with_host_1e-12": agree,
            "kernel_us_per_launch": kernels}
    pool.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
