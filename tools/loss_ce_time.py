"""Time forward + backward of the multi-class loss at 4 x K x 512^2 fp32 logits, K in {2, 16}, one logit set and four
(the deep-supervision sets [main, ds1, ds2, ds3] with weights [1, 0.4, 0.2, 0.1]), alternating in one process
  (a) stock:   torch.nn.CrossEntropyLoss (log_softmax, nll_loss and their backward kernels; four sets: the per-set
               loop of DeepSupervisionLoss),
  (b) ce:      unet.utils.CrossEntropyLoss (csrc/loss_ce.hip: one reduce, one finalize, one grad launch),
  (c) dice_ce: unet.utils.DiceCELoss (the same three launches with the Dice sums),
each with class weights, label smoothing 0.1 and about 10 % ignored pixels.  HIP events around blocks of calls, the
sides alternating block by block until each has over --seconds of timed work.  Writes a JSON: ms per call, the bytes
the algorithm has to move (from shapes, not measured: the fused passes read the logits twice and write dz once, plus
the int64 targets twice; stock is counted by the same minimum, so its GB/s is an effective rate) and the GB/s and
share of 8 TB/s these give.  Needs the GPU: there is no CPU mode.

  python tools/loss_ce_time.py [--out profiles/loss_ce_mi355x.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))
from unet.utils import CrossEntropyLoss, DeepSupervisionLoss, DiceCELoss  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "loss_ce_mi355x.json"))
ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side and shape")
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--batch", type=int, default=4)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("loss_ce_time.py measures on the GPU; none is visible")
dev, N, H, DS_W = "cuda", a.batch, a.size, [1.0, 0.4, 0.2, 0.1]
gen = torch.Generator(device=dev).manual_seed(0)

runs = {}        # (K, S, side) -> callable of one forward + backward
algo_bytes = {}  # (K, S) -> bytes
for K in (2, 16):
    t = torch.randint(0, K, (N, H, H), generator=gen, device=dev)
    t[torch.rand(N, H, H, generator=gen, device=dev) < 0.1] = -100
    w = (torch.rand(K, generator=gen, device=dev) + 0.5)
    crits = {"stock": torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1),
             "ce": CrossEntropyLoss(weight=w, label_smoothing=0.1),
             "dice_ce": DiceCELoss(class_weights=w.tolist(), label_smoothing=0.1).to(dev)}
    for S in (1, 4):
        zs = [(torch.randn(N, K, H, H, generator=gen, device=dev) * 2).requires_grad_() for _ in range(S)]
        algo_bytes[(K, S)] = S * 3 * N * K * H * H * 4 + 2 * N * H * H * 8
        for side, crit in crits.items():
            full = crit if S == 1 else DeepSupervisionLoss(crit, DS_W)

            def fn(full=full, zs=zs, t=t, S=S):
                loss = full(zs[0] if S == 1 else zs, t)
                return torch.autograd.grad(loss, zs)
            runs[(K, S, side)] = fn

for fn in runs.values():
    for _ in range(10):
        fn()
torch.cuda.synchronize()
acc = {k: [0.0, 0] for k in runs}   # ms, calls
block = 50
while any(ms < a.seconds * 1e3 for ms, _ in acc.values()):
    for key, fn in runs.items():
        if acc[key][0] >= a.seconds * 1e3:
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(block):
            fn()
        e1.record()
        torch.cuda.synchronize()
        acc[key][0] += e0.elapsed_time(e1)
        acc[key][1] += block

res = {"device": torch.cuda.get_device_name(0), "logits": f"{N} x K x {H} x {H} fp32", "hbm_peak_TBps": 8.0,
       "timing": "HIP events around blocks of 50 forward + backward calls, sides alternating", "shapes": {}}
for K in (2, 16):
    for S in (1, 4):
        out = {"algorithmic_bytes": algo_bytes[(K, S)]}
        for side in ("stock", "ce", "dice_ce"):
            ms, calls = acc[(K, S, side)]
            per = ms / calls
            out[side] = {"ms_per_call": round(per, 5), "calls_timed": calls, "timed_ms": round(ms, 1),
                         "GBps": round(algo_bytes[(K, S)] / per / 1e6, 1),
                         "share_of_hbm_peak": round(algo_bytes[(K, S)] / per / 1e6 / 8000.0, 4)}
        out["stock_over_ce"] = round(out["stock"]["ms_per_call"] / out["ce"]["ms_per_call"], 3)
        res["shapes"][f"K{K}_sets{S}"] = out
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
