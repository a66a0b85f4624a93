"""Time the device training augmentation (GpuTrainAugment) on one GPU.

Workload: batches of 4 decoded 512x512 uint8 slices with masks, already on the device (the PNG decode and the
upload of the slices are the same with and without augmentation).  Timed with HIP events after a warm-up:

  * `reference`: whole calls (table upload, resize, elastic fields, apply) cycling through 64 seeded tables drawn
    with the reference's probabilities: the expected cost per batch of the reference's recipe;
  * `forced`: whole calls with every transform switched on for every sample: the worst case;
  * `plain`: GpuSliceTransform on the same batch (what a run without augmentation already pays);
  * `kernels`: unet_aug_elastic_field and unet_aug_apply alone (forced table, back-to-back launches), next to the
    bytes each must move and the time that traffic takes at the 8 TB/s the project uses for its HBM-bound kernels
    (DESIGN.md §4).  The byte counts are algorithmic (every output written once, every input read once; the
    blur's halo and the bilinear fetch's neighbours are expected to come from cache).

Prints one JSON line.  --step-ms gives the train-step time to express the augmentation as a share of it.

    python tools/augment_bench.py [--n 4] [--size 512] [--iters 4000] [--step-ms 8.0]
"""

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))

HBM_BYTES_PER_S = 8e12


def event_time_us(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--step-ms", type=float, default=8.0, help="train-step time of bench.py on the same GPU")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a ROCm GPU: nothing is measured without one")

    from unet._hip import lib as L
    from unet._hip.runtime import stream, vp
    from unet.utils.gpu_pipeline import GpuSliceTransform, GpuTrainAugment

    N, S = a.n, a.size
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (N, S, S), dtype=np.uint8)).cuda()
    masks = torch.from_numpy((rng.random((N, S, S)) < 0.05).astype(np.uint8) * 255).cuda()
    aug = GpuTrainAugment(img_size=S)
    plain = GpuSliceTransform(img_size=S)
    tables = [aug.draw(N, np.random.default_rng(100 + i)) for i in range(64)]
    forced = aug.draw(N, np.random.default_rng(1))
    forced["flags"] = 255
    n_el_ref = float(np.mean([((t["flags"] & L.AUG_ELASTIC) != 0).sum() for t in tables]))

    t_ref = event_time_us(lambda i: aug(imgs, masks, tables[i % len(tables)]), a.iters, a.warmup)
    t_forced = event_time_us(lambda i: aug(imgs, masks, forced), a.iters, a.warmup)
    t_plain = event_time_us(lambda i: plain(imgs, masks, None), a.iters, a.warmup)

    # the two kernels alone, forced table
    tab = forced.copy()
    tab["elastic_slot"] = np.arange(N)
    tab_dev = torch.from_numpy(tab.view(np.uint8)).cuda()
    slots = torch.arange(N, dtype=torch.int32, device="cuda")
    field = aug.elastic_fields(tab_dev, slots, N)
    yt, xt = aug.tables.nearest(S, S), aug.tables.nearest(S, S)
    img = torch.empty(N, 1, S, S, device="cuda")
    mk = torch.empty(N, S, S, dtype=torch.int64, device="cuda")
    t_field = event_time_us(lambda i: aug.elastic_fields(tab_dev, slots, N), a.iters, a.warmup)
    t_apply = event_time_us(
        lambda i: L.call("unet_aug_apply", N, S, vp(imgs), S, S, vp(masks), vp(yt), vp(xt), vp(tab_dev), N, vp(field), N,
                         0.5, 0.5, vp(img), vp(mk), stream()), a.iters, a.warmup)
    px = N * S * S
    b_field = px * 2 * 4 * 3            # horizontal pass writes tmp; vertical pass reads it and writes the field
    b_apply = px * (1 + 1 + 8 + 4 + 8)  # u8 image + u8 mask + two fp32 displacements read; fp32 image + int64 mask written

    def kernel(t_us, nbytes):
        bound = nbytes / HBM_BYTES_PER_S * 1e6
        return {"us": round(t_us, 2), "bytes": nbytes, "us_at_8TBps": round(bound, 2), "x_bound": round(t_us / bound, 2),
                "GBps": round(nbytes / t_us * 1e-3, 1)}

    step_us = a.step_ms * 1e3
    print(json.dumps({
        "workload": f"{N}x{S}x{S} uint8 slices + masks on the device", "iters": a.iters, "warmup": a.warmup,
        "reference": {"us_per_batch": round(t_ref, 1), "us_per_image": round(t_ref / N, 1),
                      "mean_elastic_samples_per_batch": round(n_el_ref, 2), "share_of_step": round(t_ref / step_us, 4)},
        "forced": {"us_per_batch": round(t_forced, 1), "us_per_image": round(t_forced / N, 1),
                   "share_of_step": round(t_forced / step_us, 4)},
        "plain": {"us_per_batch": round(t_plain, 1), "us_per_image": round(t_plain / N, 1)},
        "step_ms": a.step_ms,
        "kernels": {"elastic_field": kernel(t_field, b_field), "augment_apply": kernel(t_apply, b_apply)},
    }))


if __name__ == "__main__":
    main()
