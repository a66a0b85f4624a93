"""Time the multi-channel first conv (csrc/stem.hip), forward and weight gradient (fold included), against the route
it replaces (UNET_STEM_MFMA=0: conv_generic_kernel, wgrad_kernel + wgrad_reduce_kernel) in one process, alternating
the two sides in blocks of HIP-event-timed launches until each side has at least --seconds of timed work.
Shape 4 x Cin x 512^2 -> 64, Cin in {5, 8, 16} bf16 plus one fp16 line; each time stands next to the bytes floor
(the fp32 input read once + the 16-bit output, or dy, once) at 8 TB/s.  Writes profiles/stem_conv_mi355x.json."""
import argparse
import ctypes
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))
from unet._hip import lib as L, runtime as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--out", default=str(ROOT / "profiles" / "stem_conv_mi355x.json"))
a = ap.parse_args()
N, H, W, COUT = 4, 512, 512, 64
so, dev = L.load(), "cuda"
SIDES = {"stem": None, "parent": "0"}


def side(name):
    if SIDES[name] is None:
        os.environ.pop("UNET_STEM_MFMA", None)
    else:
        os.environ["UNET_STEM_MFMA"] = SIDES[name]


def variant(d, wgrad):
    buf = ctypes.create_string_buffer(128)
    (so.unet_wgrad_variant if wgrad else so.unet_conv_variant)(ctypes.byref(d), buf, 128)
    return buf.value.decode()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def ab(fn):
    """{side: us per call}: blocks of launches, the sides alternating, until each has a.seconds of timed work"""
    reps, tot, cnt = {}, {}, {}
    for s in SIDES:
        side(s)
        reps[s] = max(5, int(a.seconds / 4 / (timed(fn, 5) / 5)))   # also the warm-up
        tot[s], cnt[s] = 0.0, 0
    while min(tot.values()) < a.seconds:
        for s in SIDES:
            side(s)
            tot[s] += timed(fn, reps[s])
            cnt[s] += reps[s]
    return {s: 1e6 * tot[s] / cnt[s] for s in SIDES}


res = []
for prec, cin in (("bf16", 5), ("bf16", 8), ("bf16", 16), ("fp16", 16)):
    P = R._PRECISIONS[prec]
    dt = torch.bfloat16 if prec == "bf16" else torch.float16
    x = torch.rand(N, cin, H, W, device=dev) * 2 - 1
    w = torch.randn(COUT, cin, 3, 3, device=dev) * 0.1
    wp = R.pack_weight(w, P, transpose=False)
    y = torch.empty(N, H, W, COUT, device=dev, dtype=dt)
    dy = torch.randn(N, H, W, COUT, device=dev).to(dt)
    dw = torch.empty(COUT, cin, 3, 3, device=dev)
    dc, dg = L.ConvDesc(), L.WgradDesc()
    for d in (dc, dg):
        d.dtype, d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = P.code, N, H, W, cin, COUT, 3, 1
        d.src[0].kind, d.src[0].C, d.src[0].H, d.src[0].W, d.src[0].data = 4, cin, H, W, x.data_ptr()
    dc.weight, dc.out, dc.out_mode = wp.data_ptr(), y.data_ptr(), 0
    dg.dy, dg.dw, dg.accum = dy.data_ptr(), dw.data_ptr(), 0
    rows, ws, names = 0, 16, {}
    for s in SIDES:   # the stats table and the workspace hold either route
        side(s)
        rows = max(rows, so.unet_conv_stats_rows(ctypes.byref(dc)))
        ws = max(ws, so.unet_wgrad_workspace(ctypes.byref(dg)))
        names[s] = (variant(dc, False), variant(dg, True))
    stats = torch.empty(2 * COUT * rows, device=dev)
    wsb = torch.empty(ws // 4 + 4, device=dev)
    dc.stats, dg.workspace = stats.data_ptr(), wsb.data_ptr()
    floor_us = (N * cin * H * W * 4 + N * H * W * COUT * 2) / 8e6
    for op, fn in (("fwd", lambda: L.call("unet_conv", dc, R.stream())),
                   ("wgrad", lambda: L.call("unet_conv_wgrad", dg, R.stream()))):
        us = ab(fn)
        i = 0 if op == "fwd" else 1
        rec = dict(op=op, precision=prec, shape=[N, cin, H, W], cout=COUT, floor_us=round(floor_us, 1),
                   stem_us=round(us["stem"], 1), parent_us=round(us["parent"], 1), stem=names["stem"][i],
                   parent=names["parent"][i])
        res.append(rec)
        print(json.dumps(rec), flush=True)
Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), seconds_per_side=a.seconds, runs=res),
                                  indent=1) + "\n")
