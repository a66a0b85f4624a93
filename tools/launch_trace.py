#!/usr/bin/env python
"""Launch trace of the stage executor: which library calls one seeded step makes, with which arguments, and
the bits it computes.  Two versions of the `unet` package's Python that trace equal over the same built library
plan the same launches in the same order and compute the same results.

    python tools/launch_trace.py run --pkg unet-segment-pytorch_amd --out tree.json
    UNET_HIP_LIB=.../libunet_hip.so python tools/launch_trace.py run --pkg <other package root> --out parent.json
    python tools/launch_trace.py compare parent.json tree.json --summary profiles/launch_trace_summary.json

`run` needs the GPU.  It wraps `lib.call`; the canonical form of a call is its name plus every argument, typed
by `lib._SIGS`: integers and floats by value, `void*` as null / non-null, descriptor structs and job arrays
field by field under the same rule.  After each configuration's step it appends a SHA-256 of the bytes of the
loss, every output, every parameter gradient, every BatchNorm buffer and (where the input requires grad) the
input gradient.  `compare` runs on the host: it prints the first differing call of a configuration that differs,
writes the per-configuration summary and exits non-zero on any difference.
"""

from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys

SWITCHES = ("UNET_NO_ACT_OUT", "UNET_NO_BNB_FUSE", "UNET_NO_GATE_FUSE", "UNET_NO_GATE_BN_FUSE", "UNET_NO_GUP_FUSE",
            "UNET_NO_POOL_FOLD", "UNET_NO_OC_FUSE")


# ---- canonical form -------------------------------------------------------------------------------------------
def _canon(tp, v) -> str:
    """One value of ctypes type `tp` (an argument, a struct field or an array element)."""
    if isinstance(tp, type) and issubclass(tp, ctypes._Pointer):
        if v is None:
            return "null"
        if isinstance(v, ctypes.Array):      # a job array / a table of pointers or weights
            return "[" + ", ".join(_canon(v._type_, e) for e in v) + "]"
        return _canon(tp._type_, v)          # a descriptor passed by reference
    if isinstance(tp, type) and issubclass(tp, ctypes.Structure):
        return "{" + ", ".join(f"{n}={_canon(t, getattr(v, n))}" for n, t in tp._fields_) + "}"
    if isinstance(tp, type) and issubclass(tp, ctypes.Array):
        return "[" + ", ".join(_canon(tp._type_, e) for e in v) + "]"
    if tp is ctypes.c_void_p:
        return "null" if not v else "ptr"
    if tp in (ctypes.c_float, ctypes.c_double):
        return repr(ctypes.c_float(v).value if tp is ctypes.c_float else float(v))
    return repr(int(v))


def canon_call(sigs, name: str, args) -> str:
    types = sigs[name][1]
    assert len(types) == len(args), (name, len(types), len(args))
    return name + "(" + ", ".join(_canon(t, a) for t, a in zip(types, args)) + ")"


def _sha(t) -> str:
    import torch
    b = t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(b).hexdigest()


# ---- configurations -------------------------------------------------------------------------------------------
def _net(kind, prec, shape, *, mode="train", env=None, need_dx=False, **kw):
    return dict(what="net", kind=kind, prec=prec, shape=shape, mode=mode, env=env, need_dx=need_dx, kw=kw)


def configurations():
    c = {"att_bf16_128": _net("AttentionUNet", "bf16", (4, 1, 128, 128))}
    for s in SWITCHES:
        c["att_bf16_128_" + s] = _net("AttentionUNet", "bf16", (4, 1, 128, 128), env=s)
    c["att_fp16_64"] = _net("AttentionUNet", "fp16", (2, 1, 64, 64))
    c["att_fp32_64"] = _net("AttentionUNet", "fp32", (2, 1, 64, 64))
    c["att_bf16_98"] = _net("AttentionUNet", "bf16", (2, 1, 98, 98))
    c["att_bf16_64_ds"] = _net("AttentionUNet", "bf16", (2, 1, 64, 64), deep_supervision=True)
    c["att_bf16_64_need_dx"] = _net("AttentionUNet", "bf16", (2, 1, 64, 64), need_dx=True)
    for prec in ("bf16", "fp32"):
        for bilinear in (True, False):
            c[f"unet_{prec}_64_{'bilinear' if bilinear else 'convt'}"] = _net("UNet", prec, (2, 1, 64, 64),
                                                                             bilinear=bilinear)
    c["att_bf16_64_eval_nograd"] = _net("AttentionUNet", "bf16", (2, 1, 64, 64), mode="eval_nograd")
    c["unet_bf16_64_eval_nograd"] = _net("UNet", "bf16", (2, 1, 64, 64), mode="eval_nograd")
    c["att_bf16_64_eval_backward"] = _net("AttentionUNet", "bf16", (2, 1, 64, 64), mode="eval_backward")
    # standalone modules (run_module), bf16, inputs requiring grad: the first input is 2 x 64 x 32 x 32, a skip
    # input the 2 x 64 x 64 x 64 map the module's geometry asks for
    a, b = (2, 64, 32, 32), (2, 64, 64, 64)
    for name, ctor, shapes in (("DoubleConv", (64, 64), [a]), ("Down", (64, 128), [a]), ("Up", (128, 64), [a, b]),
                               ("AttentionUp", (128, 64), [a, b]), ("AttentionGate", (64, 64), [a, b]),
                               ("OutConv", (64, 2), [a])):
        c["module_" + name] = dict(what="module", kind=name, ctor=ctor, shapes=shapes, prec="bf16")
    return c


def _run_config(cfg):
    """One seeded step; returns the named tensors whose bits are the configuration's result."""
    import torch
    from unet import models
    from unet.models import layers
    from unet.utils.loss import DeepSupervisionLoss, DiceBCELoss
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    res = {}
    if cfg["what"] == "module":
        m = getattr(layers, cfg["kind"])(*cfg["ctor"]).cuda().train()
        m.hip_precision = cfg["prec"]
        xs = [(torch.rand(*s, generator=g) * 2 - 1).cuda().requires_grad_(True) for s in cfg["shapes"]]
        out = m(*xs)
        out.backward((torch.rand(*out.shape, generator=g) * 2 - 1).cuda())
        res["out"] = out
        for i, x in enumerate(xs):
            res[f"input_grad.{i}"] = x.grad
    else:
        m = getattr(models, cfg["kind"])(1, 2, **cfg["kw"]).cuda()
        m.hip_precision = cfg["prec"]
        N, _, H, W = cfg["shape"]
        x = (torch.rand(*cfg["shape"], generator=g) * 2 - 1).cuda()
        t = (torch.rand(N, H, W, generator=g) < 0.1).long().cuda()
        crit = DeepSupervisionLoss(DiceBCELoss()) if cfg["kw"].get("deep_supervision") else DiceBCELoss()
        if cfg["mode"] == "eval_nograd":
            m.eval()
            with torch.no_grad():
                outs = m(x)
        else:
            m.train(cfg["mode"] == "train")
            x.requires_grad_(cfg["need_dx"])
            outs = m(x)
            loss = crit(outs, t)
            loss.backward()
            res["loss"] = loss
            if cfg["need_dx"]:
                res["input_grad"] = x.grad
        for i, o in enumerate(outs if isinstance(outs, (list, tuple)) else [outs]):
            res[f"out.{i}"] = o
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if p.grad is not None:
            res["grad." + n] = p.grad
    for n, b in m.named_buffers():
        res["buffer." + n] = b
    return res


def run(pkg: str, out: str, only):
    sys.path.insert(0, os.path.abspath(pkg))
    from unet._hip import lib as L
    calls = []
    orig = L.call

    def rec(name, *args):
        calls.append(canon_call(L._SIGS, name, args))
        return orig(name, *args)

    result = {}
    for name, cfg in configurations().items():
        if only and name not in only:
            continue
        for s in SWITCHES:
            os.environ.pop(s, None)
        if cfg.get("env"):
            os.environ[cfg["env"]] = "1"
        del calls[:]
        L.call = rec
        try:
            res = _run_config(cfg)
        finally:
            L.call = orig
        digests = {k: _sha(v) for k, v in res.items()}
        result[name] = {"calls": list(calls), "digests": digests}
        print(f"{name}: {len(calls)} calls, {len(digests)} digests", flush=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=0)


# ---- compare ----------------------------------------------------------------------------------------------------
def _hash(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:16]


def compare(parent: str, tree: str, summary) -> int:
    with open(parent) as f:
        a = json.load(f)
    with open(tree) as f:
        b = json.load(f)
    bad = 0
    rows = {}
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}: only in {'parent' if name in a else 'tree'}")
            bad += 1
            continue
        pa, tr = a[name], b[name]
        rows[name] = {"parent": {"calls": len(pa["calls"]), "trace": _hash(pa["calls"]), "outputs": _hash(pa["digests"])},
                      "tree": {"calls": len(tr["calls"]), "trace": _hash(tr["calls"]), "outputs": _hash(tr["digests"])}}
        if pa["calls"] != tr["calls"]:
            bad += 1
            i = next((i for i, (x, y) in enumerate(zip(pa["calls"], tr["calls"])) if x != y),
                     min(len(pa["calls"]), len(tr["calls"])))
            print(f"{name}: call lists differ at call {i} ({len(pa['calls'])} vs {len(tr['calls'])} calls)")
            print("  parent:", pa["calls"][i] if i < len(pa["calls"]) else "<end>")
            print("  tree:  ", tr["calls"][i] if i < len(tr["calls"]) else "<end>")
        diff = sorted(k for k in set(pa["digests"]) | set(tr["digests"]) if pa["digests"].get(k) != tr["digests"].get(k))
        if diff:
            bad += 1
            print(f"{name}: {len(diff)} digests differ, first {diff[0]}")
    print(f"{len(rows)} configurations compared, {bad} differences")
    if summary:
        with open(summary, "w") as f:
            json.dump({"configurations": rows, "equal": bad == 0}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--pkg", required=True, help="directory that holds the `unet` package to trace")
    r.add_argument("--out", required=True)
    r.add_argument("--only", nargs="*", help="configuration names (default: all)")
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("tree")
    c.add_argument("--summary")
    a = ap.parse_args()
    if a.cmd == "run":
        run(a.pkg, a.out, a.only)
        return 0
    return compare(a.parent, a.tree, a.summary)


if __name__ == "__main__":
    sys.exit(main())
