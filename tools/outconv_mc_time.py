"""Launch the multi-class OutConv forward and backward (csrc/outconv_mc.hip) a few times at one shape, for a kernel
trace:  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/outconv_mc_time.py
        python tools/profsum.py DIR <reps>
Prints the bytes each launch has to move (derived, not measured) next to its HIP-event time."""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "unet-segment-pytorch_amd"))
from unet._hip import lib as L, runtime as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=5, default=[4, 512, 512, 64, 16], metavar=("N", "H", "W", "C", "K"))
ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32"])
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
N, H, W, C, K = a.shape
dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.precision]
code = R._PRECISIONS[a.precision].code
dev = "cuda"
y = torch.randn(N, H, W, C, device=dev).to(dt)
sc, sf = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.4
w, b = torch.randn(K, C, device=dev) * 0.1, torch.randn(K, device=dev)
out, dl = torch.empty(N, K, H, W, device=dev), torch.randn(N, K, H, W, device=dev)
da = torch.empty(N, H, W, C, device=dev)
rows = L.load().unet_outconv_rows(N * H * W)
part = torch.empty(rows, K + 1, C, device=dev)
P, es = N * H * W, y.element_size()
calls = {
    "fwd": (P * C * es + P * K * 4,
            lambda: L.call("unet_outconv_mc_fwd", code, N, H, W, C, K, R.vp(y), R.vp(sc), R.vp(sf), 1, R.vp(w), R.vp(b),
                           R.vp(out), R.stream())),
    "bwd": (P * C * es + P * K * 4 + P * C * 4,
            lambda: L.call("unet_outconv_mc_bwd", code, N, H, W, C, K, R.vp(y), R.vp(sc), R.vp(sf), 1, R.vp(w), R.vp(dl),
                           R.vp(da), 0, R.vp(part), R.stream())),
}
for name, (nbytes, fn) in calls.items():
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / a.reps
    print(f"{name} {a.precision} {N}x{H}x{W} C={C} K={K}: {us:.1f} us, {nbytes / 1e6:.0f} MB -> "
          f"{nbytes / us / 1e6:.2f} TB/s ({100 * nbytes / us / 8e6:.0f}% of 8 TB/s)")
