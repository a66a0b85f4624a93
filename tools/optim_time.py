"""Time the tail of the training step (clip + AdamW + EMA) at the bench model, AttentionUNet 1x512^2 base 64, with
seeded gradients, alternating in one process
  (a) torch:  clip_grad_norm_ + torch.optim.AdamW(fused=True) + the per-tensor EMA loop (mul_ / add_ per parameter,
              copy_ per buffer, as ModelEMA.update of the reference is written), and
  (b) fused:  FusedClipAdamW(max_grad_norm=1.0) + ModelEMA (csrc/optim.hip),
each as the whole tail, the step alone and the EMA alone.  HIP events around blocks of steps, the sides alternating
block by block until each has over --seconds of timed work.  Writes a JSON: ms per step, launches per step (kernel
events of one profiled step), the bytes the algorithm has to move (from shapes, not measured) and the GB/s and
share of 8 TB/s these give.  Needs the GPU: there is no CPU mode.

  python tools/optim_time.py [--out profiles/optim_tail_mi355x.json]"""
import argparse
import copy
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))
from unet.models import AttentionUNet  # noqa: E402
from unet.utils import FusedClipAdamW, ModelEMA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=str(ROOT / "profiles" / "optim_tail_mi355x.json"))
ap.add_argument("--seconds", type=float, default=1.5, help="timed work per side and mode")
ap.add_argument("--base", type=int, default=64)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("optim_time.py measures on the GPU; none is visible")
dev, lr, wd, clip, decay = "cuda", 5e-5, 1e-4, 1.0, 0.999

torch.manual_seed(0)
model_a = AttentionUNet(1, 2, base_features=a.base).to(dev)
model_b = copy.deepcopy(model_a)
gen = torch.Generator(device=dev).manual_seed(1)
for pa, pb in zip(model_a.parameters(), model_b.parameters()):
    pa.grad = 1e-3 * torch.randn(pa.shape, generator=gen, device=dev)
    pb.grad = pa.grad.clone()
params_a = list(model_a.parameters())
opt_a = torch.optim.AdamW(params_a, lr=lr, weight_decay=wd, fused=True)
ema_a = copy.deepcopy(model_a).eval()
pairs_p = list(zip(ema_a.parameters(), model_a.parameters()))
pairs_b = list(zip(ema_a.buffers(), model_a.buffers()))
opt_b = FusedClipAdamW(model_b.parameters(), lr=lr, weight_decay=wd, max_grad_norm=clip)
ema_b = ModelEMA(model_b, decay)


def a_step():
    torch.nn.utils.clip_grad_norm_(params_a, clip)
    opt_a.step()


@torch.no_grad()
def a_ema():
    for e, p in pairs_p:
        e.mul_(decay).add_(p, alpha=1 - decay)
    for e, b in pairs_b:
        e.copy_(b)


sides = {
    "torch": {"step": a_step, "ema": a_ema, "tail": lambda: (a_step(), a_ema())},
    "fused": {"step": opt_b.step, "ema": lambda: ema_b.update(model_b),
              "tail": lambda: (opt_b.step(), ema_b.update(model_b))},
}
n_param = sum(p.numel() for p in params_a)
buf_bytes = sum(b.numel() * b.element_size() for b in model_a.buffers())
algo_bytes = {"step": 32 * n_param,               # norm: read g; update: read p, g, m, v, write p, m, v (4 B each)
              "ema": 12 * n_param + 2 * buf_bytes}  # read e, p, write e; buffers read + written
algo_bytes["tail"] = algo_bytes["step"] + algo_bytes["ema"]

acc = {(s, m): [0.0, 0] for s in sides for m in ("tail", "step", "ema")}   # ms, steps
for fn in (f for s in sides.values() for f in s.values()):
    for _ in range(10):
        fn()
torch.cuda.synchronize()
block = 50
while any(ms < a.seconds * 1e3 for ms, _ in acc.values()):
    for mode in ("tail", "step", "ema"):
        for side in sides:
            if acc[(side, mode)][0] >= a.seconds * 1e3:
                continue
            fn = sides[side][mode]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                fn()
            e1.record()
            torch.cuda.synchronize()
            acc[(side, mode)][0] += e0.elapsed_time(e1)
            acc[(side, mode)][1] += block

res = {"device": torch.cuda.get_device_name(0), "model": f"AttentionUNet(1, 2, base_features={a.base})",
       "parameters": n_param, "parameter_tensors": len(params_a), "buffers": len(pairs_b), "hbm_peak_TBps": 8.0,
       "algorithmic_bytes": algo_bytes, "timing": "HIP events around blocks of 50 steps, sides alternating", "sides": {}}
for side in sides:
    out = {}
    for mode in ("tail", "step", "ema"):
        ms, steps = acc[(side, mode)]
        per = ms / steps
        out[mode] = {"ms_per_step": round(per, 5), "steps_timed": steps, "timed_ms": round(ms, 1),
                     "GBps": round(algo_bytes[mode] / per / 1e6, 1),
                     "share_of_hbm_peak": round(algo_bytes[mode] / per / 1e6 / 8000.0, 4), "launches_per_step": None}
    res["sides"][side] = out
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

# launches per step: the device kernel / copy events of one profiled step (written after the timings, which stand
# without it if the profiler is unavailable)
try:
    from torch.profiler import ProfilerActivity, profile
    for side in sides:
        for mode in ("tail", "step", "ema"):
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3):
                    sides[side][mode]()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            res["sides"][side][mode]["launches_per_step"] = round(n / 3, 1)
except Exception as ex:   # noqa: BLE001
    res["launch_count_error"] = f"{type(ex).__name__}: {ex}"
Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
print(json.dumps(res))
