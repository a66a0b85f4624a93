"""Generator of tests/golden/routes.json: which kernel family the library chooses for a descriptor.

    python tests/golden/make_routes.py --lib <libunet_hip.so of the PARENT commit> --commit <its hash>

The query entry points (unet_conv_variant / _stats_rows / _workspace / _act_out_ok, unet_wgrad_variant /
_workspace) are pure functions of the descriptor and the environment: they launch nothing and dereference no
device pointer, so they run on a machine without a GPU with dummy non-null pointers.  The table is recorded from a
build of the commit BEFORE a change to the routing code, never from the code under test; tests/test_routes_cpu.py
imports the case -> descriptor builders below and asserts that the library as built answers the same.

A case is a JSON list (one per line in routes.json):
  conv : [env, dtype, ksize, shape, Cout, [[kind, C, gate], ...], out, act_out, workspace]
  wgrad: [env, dtype, ksize, shape, Cout, [[kind, C, gate], ...]]
followed by its recorded answers ([variant index, stats rows, workspace bytes, act_out_ok] / [variant index,
workspace bytes]).  env indexes "envs", shape indexes "shapes", the variant index "variants".
"""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "unet-segment-pytorch_amd"))
from unet._hip import lib as L  # noqa: E402  (the descriptor structs; the ABI is part of what must not change)

PTR = 0x1000   # dummy non-null pointer: no query dereferences it
SHAPES = [(4, 512, 512), (4, 256, 256), (4, 128, 128), (4, 64, 64), (4, 32, 32), (1, 1024, 1024), (2, 40, 56),
          (1, 16, 16)]
# per-call switches, varied one at a time (plus the two "everything" settings together); the cached ones
# (UNET_CONV3_TILE, UNET_PW_WIDE, UNET_PW_WGRAD_MINP) stay unset
ENVS = [{}, {"UNET_CONV5": "0"}, {"UNET_CONV5": "1"}, {"UNET_CONV5W": "0"}, {"UNET_CONV5W": "1"},
        {"UNET_CONV5_MI2": "0"}, {"UNET_CONV5_MI2": "2"}, {"UNET_CONV5_SPLIT": "0"},
        {"UNET_CONV5": "1", "UNET_CONV5W": "1"}, {"UNET_WGRAD5": "0"}, {"UNET_WGRAD5": "1"}]
CONV_ENVS, WGRAD_ENVS = list(range(9)), [0, 9, 10]
ROUTE_SWITCHES = ["UNET_CONV5", "UNET_CONV5W", "UNET_CONV5_MI2", "UNET_CONV5_SPLIT", "UNET_WGRAD5", "UNET_C5_PRIO",
                  "UNET_C5_BNB_PIPE", "UNET_W5_WCO2", "UNET_W5_SPLIT8", "UNET_PW_BLOCKS", "UNET_PW_XD",
                  "UNET_PWW_BLOCKS", "UNET_SMALLCIN_MFMA", "UNET_CONV3_TILE", "UNET_PW_WIDE", "UNET_PW_WGRAD_MINP"]

PLAIN, ACT, POOL_ACT, UP_ACT, NCHW, UP_PLAIN = (L.SRC_PLAIN, L.SRC_ACT, L.SRC_POOL_ACT, L.SRC_UP_ACT, L.SRC_NCHW_F32,
                                                L.SRC_UP_PLAIN)
KINDS = [PLAIN, ACT, POOL_ACT, UP_ACT, UP_PLAIN, NCHW]


def _src(s, spec, H, W):
    kind, C, gate = spec
    s.kind, s.C, s.H, s.W, s.data = kind, C, H, W, PTR
    if kind in (ACT, POOL_ACT, UP_ACT):
        s.scale, s.shift, s.relu = PTR, PTR, 1
    if kind == POOL_ACT:
        s.H, s.W = 2 * H, 2 * W
    if kind in (UP_ACT, UP_PLAIN):
        s.H, s.W = max(H // 2, 1), max(W // 2, 1)
        s.up_h, s.up_w = 2 * s.H, 2 * s.W
        s.pad_t, s.pad_l = (H - s.up_h) // 2, (W - s.up_w) // 2
        s.sh = (s.H - 1) / max(s.up_h - 1, 1)
        s.sw = (s.W - 1) / max(s.up_w - 1, 1)
    if gate:
        s.gate_p, s.gate_ab = PTR, PTR


def conv_desc(case):
    _, dtype, ks, shape, Cout, srcs, out, act_out, ws = case
    N, H, W = SHAPES[shape]
    d = L.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cout, d.ksize, d.nsrc = dtype, N, H, W, Cout, ks, len(srcs)
    d.Cin = sum(s[1] for s in srcs)
    for i, s in enumerate(srcs):
        _src(d.src[i], s, H, W)
    d.weight, d.out = PTR, PTR
    if out in ("y", "ys", "yb"):
        d.out_mode = L.OUT_Y
        if out == "ys":
            d.stats = PTR
        if out == "yb":
            d.bnb_y = d.bnb_scale = d.bnb_shift = d.bnb_mean = d.bnb_invstd = d.bnb_stats = PTR
            d.bnb_relu = 1
    elif out in ("f", "fs", "fsa"):
        d.out_mode, d.split = L.OUT_F32, Cout if out == "f" else Cout // 2
        if out != "f":
            d.out2 = PTR
        if out == "fsa":
            d.accum = d.accum2 = 1
    elif out == "p":
        d.out_mode = L.OUT_POOL_BWD
        _src(d.pool_src, (ACT, Cout, 0), 2 * H, 2 * W)
    elif out == "s2":
        d.out_mode = L.OUT_SHUFFLE2
    elif out == "fg":
        d.out_mode, d.split = L.OUT_F32_GATED, Cout
        d.pool_src.data = d.pool_src.gate_p = d.pool_src.gate_ab = PTR
    else:
        raise ValueError(out)
    if act_out:
        d.act_out = PTR
    if ws:
        d.workspace = PTR
    return d


def wgrad_desc(case):
    _, dtype, ks, shape, Cout, srcs = case
    N, H, W = SHAPES[shape]
    d = L.WgradDesc()
    d.dtype, d.N, d.H, d.W, d.Cout, d.ksize, d.nsrc = dtype, N, H, W, Cout, ks, len(srcs)
    d.Cin = sum(s[1] for s in srcs)
    for i, s in enumerate(srcs):
        _src(d.src[i], s, H, W)
    d.dy = d.dw = d.workspace = PTR
    return d


def bind(path):
    so = ctypes.CDLL(str(path))
    for name in ("unet_conv_variant", "unet_conv_stats_rows", "unet_conv_workspace", "unet_conv_act_out_ok",
                 "unet_wgrad_variant", "unet_wgrad_workspace"):
        f = getattr(so, name)
        f.restype, f.argtypes = L._SIGS[name]
    return so


def query_conv(so, case):
    d = conv_desc(case)
    buf = ctypes.create_string_buffer(128)
    assert so.unet_conv_variant(ctypes.byref(d), buf, 128) == 0
    return [buf.value.decode(), so.unet_conv_stats_rows(ctypes.byref(d)), so.unet_conv_workspace(ctypes.byref(d)),
            so.unet_conv_act_out_ok(ctypes.byref(d))]


def query_wgrad(so, case):
    d = wgrad_desc(case)
    buf = ctypes.create_string_buffer(128)
    assert so.unet_wgrad_variant(ctypes.byref(d), buf, 128) == 0
    return [buf.value.decode(), so.unet_wgrad_workspace(ctypes.byref(d))]


def set_env(env, setenv=os.environ.__setitem__, delenv=lambda k: os.environ.pop(k, None)):
    for k in ROUTE_SWITCHES:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)


def conv_path(variant):
    for prefix, path in (("smallcin_fwd", "smallcin"), ("pw_conv_kernel", "pw"), ("conv_generic_kernel", "generic"),
                         ("conv5w_kernel", "conv5w"), ("conv3_kernel", "conv3"), ("conv2_kernel", "conv2")):
        if variant.startswith(prefix):
            return path
    assert variant.startswith("conv5_kernel"), variant
    return "conv5_splitk" if "+splitk" in variant else "conv5"


def wgrad_path(variant):
    for prefix, path in (("smallcin_wgrad", "smallcin"), ("pw_wgrad_kernel", "pw"), ("wgrad5_kernel", "wgrad5"),
                         ("wgrad2_kernel", "wgrad2"), ("wgrad_kernel", "wgrad")):
        if variant.startswith(prefix):
            return path
    raise AssertionError(variant)


# ---- the grid (deterministic, and small enough to read: every listed value and state appears, crossed where the
# routing thresholds lie, not everywhere).  unet_conv rejects: sum of source channels != Cin (never built), SHUFFLE2
# with ksize != 1 or Cout % 4, bnb_* with forward stats or another mode (never built); act_out where
# unet_conv_act_out_ok says no and F32_GATED off the pw path are pruned in main() by asking the parent library.
PAIRS = [(1, 64), (3, 64), (3, 32), (16, 16), (16, 3), (20, 32), (32, 48), (32, 64), (48, 64), (64, 64), (64, 128),
         (128, 64), (128, 128), (256, 128), (256, 256), (512, 256), (512, 512), (1024, 512), (1024, 1024), (64, 1),
         (64, 20)]
C5_PAIRS = [(64, 64), (128, 128), (256, 128), (512, 512), (1024, 512)]
CONCATS = [(64, 64), (16, 48), (48, 16), (20, 44), (512, 512)]
ALL_SHAPES = list(range(len(SHAPES)))


def conv_cases():
    bf, hf, f32 = L.BF16, L.F16, L.F32
    out = []
    # 1. channel sweep: one stored source, forward with stats, every shape
    for ks in (1, 3):
        for sh in ALL_SHAPES if ks == 3 else (0, 2, 3, 4):
            for ci, co in PAIRS:
                out.append([0, bf, ks, sh, co, [[PLAIN, ci, 0]], "ys", 0, 1])
    # 2. dtype x source kind x gate
    for dt in (bf, hf, f32):
        for ks in (1, 3):
            if dt != bf and ks == 1:
                continue
            for sh in (0, 6) if dt != hf else (0,):
                for ci, co in ((48, 64), (512, 512)):
                    for kind in KINDS:
                        for gate in (0, 1):
                            out.append([0, dt, ks, sh, co, [[kind, ci, gate]], "ys", 0, 1])
    # 2b. the network's first conv: the fp32 NCHW input with 1-4 channels
    for dt in (bf, hf, f32):
        for sh in (0, 3, 4, 5, 7):
            for ci, co in ((1, 64), (3, 20)):
                out.append([0, dt, 3, sh, co, [[NCHW, ci, 0]], "ys", 0, 1])
    # 3. output modes (the gradient modes read the stored dy; the forward ones a BN activation too)
    for dt in (bf, hf, f32):
        for sh in {bf: (0, 3, 6), hf: (3,), f32: (0,)}[dt]:
            for ci, co in ((20, 32), (64, 128)):
                for kind, ks, mode in ((PLAIN, 3, "y"), (ACT, 3, "y"), (PLAIN, 3, "yb"), (PLAIN, 3, "f"), (PLAIN, 3, "fs"),
                                       (PLAIN, 3, "fsa"), (PLAIN, 3, "p"), (ACT, 1, "y"), (PLAIN, 1, "f"),
                                       (PLAIN, 1, "fs"), (PLAIN, 1, "yb"), (PLAIN, 1, "s2"), (PLAIN, 1, "fg"),
                                       (ACT, 1, "fg")):
                    out.append([0, dt, ks, sh, co, [[kind, ci, 0]], mode, 0, 1])
    # 4. two-source concats (first source C % 16 != 0 and C % 32 != 0 among them), with conv5 and without
    for env, dt in ((0, bf), (1, bf), (0, f32)):
        for sh in (0, 4) if dt == bf else (0,):
            for c0, c1 in CONCATS:
                co = 64 if c0 + c1 <= 128 else 256
                for s0, s1, ks, mode in (((PLAIN, 0), (PLAIN, 0), 3, "ys"), ((ACT, 0), (PLAIN, 0), 3, "ys"),
                                         ((ACT, 1), (PLAIN, 0), 3, "ys"), ((ACT, 0), (UP_ACT, 0), 3, "ys"),
                                         ((PLAIN, 0), (PLAIN, 0), 3, "fs"), ((PLAIN, 0), (PLAIN, 0), 3, "fsa"),
                                         ((PLAIN, 0), (UP_PLAIN, 0), 1, "ys"), ((ACT, 0), (PLAIN, 0), 1, "ys")):
                    out.append([env, dt, ks, sh, co, [[s0[0], c0, s0[1]], [s1[0], c1, s1[1]]], mode, 0, 1])
    # 5. the conv5 region under every switch, with and without a workspace and act_out
    for env in CONV_ENVS:
        for dt in (bf, hf):
            if dt == hf and env:
                continue
            shapes = (0, 3, 4, 6, 7) if (env, dt) == (0, bf) else (0, 3, 4)
            pairs = C5_PAIRS if (env, dt) == (0, bf) else [(256, 128), (512, 512)]
            for sh in shapes:
                for ci, co in pairs:
                    for kind, gate, mode in ((PLAIN, 0, "ys"), (PLAIN, 0, "yb"), (PLAIN, 0, "f"), (ACT, 0, "ys"),
                                             (ACT, 1, "ys")):
                        if (env or dt == hf) and (mode == "yb" or gate):
                            continue
                        for ws in (0, 1):
                            if not ws and SHAPES[sh][1] > 128:
                                continue   # (split-K only serves maps too small to fill the chip)
                            out.append([env, dt, 3, sh, co, [[kind, ci, gate]], mode, 0, ws])
                            if kind == ACT and not gate and ws:
                                out.append([env, dt, 3, sh, co, [[kind, ci, gate]], mode, 1, ws])
                # a gated [skip, up] concat, the decoder's first conv
                for ws in (0, 1):
                    out.append([env, dt, 3, sh, 256, [[ACT, 256, 1], [PLAIN, 256, 0]], "ys", 0, ws])
    return out


def wgrad_cases():
    bf, hf, f32 = L.BF16, L.F16, L.F32
    out = []
    for ks in (1, 3):   # every shape and channel pair, one stored source
        for sh in ALL_SHAPES if ks == 3 else (0, 1, 2, 3):
            for ci, co in PAIRS:
                out.append([0, bf, ks, sh, co, [[PLAIN, ci, 0]]])
    for dt in (bf, hf, f32):   # dtype x source kind
        for ks in (1, 3):
            for sh in (0, 3):
                for kind, gate in ((PLAIN, 0), (ACT, 0), (ACT, 1), (POOL_ACT, 0), (UP_ACT, 0), (UP_PLAIN, 0)):
                    for ci, co in ((64, 64), (256, 128)):
                        out.append([0, dt, ks, sh, co, [[kind, ci, gate]]])
                out.append([0, dt, ks, sh, 64, [[NCHW, 3, 0]]])
                out.append([0, dt, ks, sh, 32, [[NCHW, 1, 0]]])
                for c0, c1 in CONCATS:
                    if dt == bf:
                        out.append([0, dt, ks, sh, 64, [[ACT, c0, 1], [PLAIN, c1, 0]]])
    for env in WGRAD_ENVS[1:]:   # the wgrad5 / wgrad2 boundary under UNET_WGRAD5
        for sh in ALL_SHAPES:
            for ci, co in ((64, 64), (256, 128), (48, 64)):
                for kind in (PLAIN, ACT):
                    out.append([env, bf, 3, sh, co, [[kind, ci, 0]]])
    return out


def dedupe(cases):
    seen, out = set(), []
    for c in cases:
        k = json.dumps(c)
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libunet_hip.so built from the parent commit")
    ap.add_argument("--commit", required=True, help="hash of that commit")
    ap.add_argument("--out", default=str(Path(__file__).with_name("routes.json")))
    a = ap.parse_args()
    so = bind(a.lib)
    variants, vidx = [], {}

    def vi(v):
        if v not in vidx:
            vidx[v] = len(variants)
            variants.append(v)
        return vidx[v]

    conv, wgrad = [], []
    for env in range(len(ENVS)):
        set_env(ENVS[env])
        for c in dedupe(conv_cases()):
            if c[0] != env:
                continue
            v, rows, ws, act = query_conv(so, c)
            if c[7] and not act:
                continue   # unet_conv rejects act_out there
            if c[6] == "fg" and conv_path(v) != "pw":
                continue   # ... and F32_GATED off the pw path
            conv.append(c + [vi(v), rows, ws, act])
        for c in dedupe(wgrad_cases()):
            if c[0] != env:
                continue
            v, ws = query_wgrad(so, c)
            wgrad.append(c + [vi(v), ws])
    dump = lambda x: json.dumps(x, separators=(",", ":"))
    with open(a.out, "w") as f:
        f.write('{"commit":%s,\n"envs":%s,\n"shapes":%s,\n"variants":%s,\n' %
                (dump(a.commit), dump(ENVS), dump(SHAPES), dump(variants)))
        f.write('"conv":[\n' + ",\n".join(dump(c) for c in conv) + '\n],\n')
        f.write('"wgrad":[\n' + ",\n".join(dump(c) for c in wgrad) + '\n]}\n')
    from collections import Counter
    print("conv cases", len(conv), dict(Counter(conv_path(variants[c[9]]) for c in conv)))
    print("wgrad cases", len(wgrad), dict(Counter(wgrad_path(variants[c[6]]) for c in wgrad)))
    print("bytes", os.path.getsize(a.out))


if __name__ == "__main__":
    main()
