"""Time unet.utils.connected_components + filter_components at 4 x 512^2 label maps, K in {2, 16}, against the host
route users have today.

Two inputs per K: blob-shaped masks (the argmax of smooth random fields, a 16 x 16 grid per class, bicubically
upsampled) and per-pixel noise at density 0.59, the site-percolation threshold, which gives the most components and
the longest union-find chains.
  (a) device: filter_components(min_size=20) on device label maps (label + filter, 4 launches), HIP events around
              blocks of 20 calls after 10 warm-up calls, blocks repeated until over --seconds of timed work; the
              median block is reported.  The same for keep_largest=True (6 launches).
  (b) host:   .cpu(), scipy.ndimage.label once per class and image, np.bincount for the areas, the area filter, and
              the copy back to the device; wall clock around a final synchronise, best of --host-reps.  Without
              scipy the kernel times stand alone and the JSON says so.
Per-kernel times come from the same process: torch.profiler around a block of calls after the timed section.  Writes
a JSON; needs the GPU: there is no CPU mode.

  python tools/cc_time.py [--out profiles/cc_label_mi355x.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))

MIN_SIZE = 20


def host_route(pd, K, ndimage):
    """The route the device path replaces: 8-connected components per class and image, blobs under MIN_SIZE dropped."""
    p = pd.cpu().numpy()
    out = np.zeros_like(p)
    for n in range(p.shape[0]):
        for c in range(1, K):
            lab, _ = ndimage.label(p[n] == c, structure=np.ones((3, 3), bool))
            keep = np.bincount(lab.ravel()) >= MIN_SIZE
            keep[0] = False
            out[n][keep[lab]] = c
    return out


def timed_blocks(fn, seconds, torch, block=20):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    times = []
    while sum(times) < seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(block):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times) / block, len(times) * block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cc_label_mi355x.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per case")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from unet.utils import connected_components, filter_components
    if not torch.cuda.is_available():
        sys.exit("cc_time.py measures on the GPU; none is visible")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    N, H = a.batch, a.size
    gen = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "label_maps": f"{N} x {H} x {H} int64", "min_size": MIN_SIZE,
           "connectivity": 8,
           "timing": "HIP events around blocks of 20 calls after 10 warm-up calls, median block; host: wall clock, "
                     f"best of {a.host_reps}, one process",
           "host_route": "scipy.ndimage.label per class and image" if ndimage else "scipy absent: not measured",
           "cases": {}}
    for K in (2, 16):
        blob = F.interpolate(torch.randn(N, K, 16, 16, generator=gen), size=(H, H), mode="bicubic").argmax(1)
        fg = torch.rand(N, H, H, generator=gen) < 0.59
        noise = torch.where(fg, torch.randint(1, K, (N, H, H), generator=gen), 0)
        for name, p in (("blobs", blob), ("noise", noise)):
            pd = p.cuda()
            ms, calls = timed_blocks(lambda: filter_components(pd, K, MIN_SIZE), a.seconds, torch)
            ms_kl, _ = timed_blocks(lambda: filter_components(pd, K, MIN_SIZE, keep_largest=True), a.seconds, torch)
            out = filter_components(pd, K, MIN_SIZE)
            case = {"components": int(connected_components(pd, K)["count"].sum()),
                    "device_ms_per_call": round(ms, 4), "calls_timed": calls,
                    "device_ms_per_call_keep_largest": round(ms_kl, 4)}
            if ndimage:
                host_s = []
                for _ in range(a.host_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ref = torch.from_numpy(host_route(pd, K, ndimage)).cuda()
                    torch.cuda.synchronize()
                    host_s.append(time.perf_counter() - t0)
                case.update({"host_ms_per_call": round(min(host_s) * 1e3, 2),
                             "host_ms_all": [round(s * 1e3, 2) for s in host_s],
                             "host_over_device": round(min(host_s) * 1e3 / ms, 1),
                             "agrees_with_host": bool(torch.equal(out, ref))})
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(20):
                        filter_components(pd, K, MIN_SIZE, keep_largest=True)
                    torch.cuda.synchronize()
                case["kernel_us_per_launch"] = {
                    e.key.split("(")[0].replace("void unet::", ""): round(e.device_time_total / e.count, 2)
                    for e in prof.key_averages() if "cc_" in e.key}
            except Exception as exc:  # the tracer is optional: the end-to-end figures stand without it
                case["kernel_us_per_launch"] = f"not measured ({type(exc).__name__})"
            res["cases"][f"K{K}_{name}"] = case
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
