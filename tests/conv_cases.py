"""Case tables of the exact-grid convolution tests, and the code that turns a case into operands, an fp64 reference
and a descriptor.

The method (tests/ref_ops.py, "the exact-grid method"): every operand is drawn on a dyadic grid, so every product is a
multiple of one unit u, and where Σ|terms| / u < 2^24 the fp32 accumulator of ANY correct kernel (any tile split, chunk
order, split-K factor or MFMA shape) equals the fp64 value.  The gate is then bit equality, with no tolerance: one
dropped, doubled or misplaced term fails it.  tests/test_conv_cases_cpu.py proves on the CPU, for every case here,
that the condition holds and that the case reaches the kernel instantiation it names; tests/test_gpu_conv_exact.py and
tests/test_gpu_wgrad_exact.py launch them.

Grids: stored activations and shifts k/4 with |·| <= 1, BN scales in {−1, 1, 2} (so a transformed input is k/4 with
|·| <= 3), plain inputs k/4 with |·| <= 3, weights k/8 with |·| <= 1/2, gradients dy k/4 with |·| <= 2.  A gate's
pre-sigmoid value is exactly 0 or +40 (σ = 1/2 or 1), an exact up-sampling uses up = 2·s − 1 (bilinear weights
{0, 1/2, 1}).

A case is plain data (a dict).  Common keys: id, dt ('bf16' / 'fp16' / 'fp32'), k, shape (N, H, W), srcs, cout,
variant (the kernel instantiation it must run on), env (per-call switches), gate ('exact', or 'elem' for the two
inexact-by-construction kinds: an fp32 operand through a gate's sigmoid, and a conventional up = 2·s bilinear, which
the tables keep to fp32 — a 16-bit kernel rounds the blended value to its operand type, and where the reference rounds
it the other way the operand itself differs).
A source is dict(kind, C, gate, relu, up, pad, extra):
  kind  plain | act | pool_act | up_act | up_plain | nchw
  up    'half' (up = 2·s − 1: exact) or 'conv' (up = 2·s: the general-scale path, inexact)
  pad   (pad_t, pad_l) of a placed map; extra: (rows, cols) a pooled source is larger than 2H x 2W by
Conv cases add: out ('y', 'f32', 'pool_bwd', 'shuffle2', 'f32_gated'), dgrad (weights packed with transpose; the
sources are then the gradient dy), ws (pass a workspace), stats, bnb, split, accum, accum2, act_out, pool_code,
pool_extra, bias.  Wgrad cases add accum.

A new kernel form adds its cases here; test_conv_cases_cpu.py fails until every variant name of
tests/golden/routes.json is covered by a case or listed in UNREACHED with a reason.
"""

import ctypes
from types import SimpleNamespace as NS

import numpy as np
import torch

import ref_ops as ro

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
KIND = {"plain": 0, "act": 1, "pool_act": 2, "up_act": 3, "nchw": 4, "up_plain": 5}
OUT = {"y": 0, "f32": 1, "pool_bwd": 2, "shuffle2": 3, "f32_gated": 4}
SWITCHES = ("UNET_CONV5", "UNET_CONV5W", "UNET_CONV5_MI2", "UNET_CONV5_SPLIT", "UNET_WGRAD5", "UNET_SMALLCIN_MFMA")
MAX_PIXELS, MAX_CHANNELS = 65536, 512
PTR = 0x1000   # dummy non-null pointer of the CPU route queries, which dereference nothing

STEP_X, STEP_W, STEP_DY = 0.25, 0.125, 0.25
GATE_AB = (-40.0, 40.0)   # p in {0, 1}: the pre-sigmoid value is exactly +40 or 0


def S(kind, C, gate=0, relu=1, up="half", pad=(0, 0), extra=(0, 0)):
    return dict(kind=kind, C=C, gate=gate, relu=relu, up=up, pad=pad, extra=extra)


def conv(id, dt, k, shape, srcs, cout, variant, out="y", **kw):
    c = dict(id=id, dt=dt, k=k, shape=shape, srcs=srcs, cout=cout, variant=variant, out=out, dgrad=0, ws=1, env={},
             gate="exact", stats=0, bnb=0, split=None, accum=0, accum2=0, act_out=0, pool_code=0, pool_extra=(0, 0),
             bias=0, sums=())
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


def wgrad(id, dt, k, shape, srcs, cout, variant, **kw):
    c = dict(id=id, dt=dt, k=k, shape=shape, srcs=srcs, cout=cout, variant=variant, env={}, gate="exact", accum=0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


# ---- geometry, operands, reference ------------------------------------------------------------------

def src_geom(s, H, W):
    """stored size and placement of a source in an H x W conv input"""
    g = NS(H=H, W=W, up_h=0, up_w=0, pad_t=0, pad_l=0, sh=0.0, sw=0.0)
    if s["kind"] == "pool_act":
        g.H, g.W = 2 * H + s["extra"][0], 2 * W + s["extra"][1]
    elif s["kind"] == "up_act":
        g.pad_t, g.pad_l = s["pad"]
        if s["up"] == "half":   # the largest odd size that fits below / right of the pad
            g.up_h, g.up_w = (H - g.pad_t - 1) // 2 * 2 + 1, (W - g.pad_l - 1) // 2 * 2 + 1
            g.H, g.W = (g.up_h + 1) // 2, (g.up_w + 1) // 2
        else:
            g.H, g.W = (H - g.pad_t) // 2, (W - g.pad_l) // 2
            g.up_h, g.up_w = 2 * g.H, 2 * g.W
        # fp32 align_corners scales as ATen's area_pixel_compute_scale
        g.sh = float(np.float32(g.H - 1) / np.float32(g.up_h - 1)) if g.up_h > 1 else 0.0
        g.sw = float(np.float32(g.W - 1) / np.float32(g.up_w - 1)) if g.up_w > 1 else 0.0
        assert g.H >= 1 and g.W >= 1
    elif s["kind"] == "up_plain":
        g.pad_t, g.pad_l = s["pad"]
        g.up_h, g.up_w = max(H - g.pad_t - 1, 1), max(W - g.pad_l - 2, 1)
        g.H, g.W = g.up_h, g.up_w
    return g


def _affine(C, gen):
    scale = torch.tensor([(-1.0, 1.0, 2.0)[(c + 1) % 3] for c in range(C)])
    return scale, ro.grid((C,), STEP_X, 4, torch.float32, gen)


def src_operands(s, N, H, W, dtype, gen):
    """the tensors of one source (CPU) and its reference spec for ref_ops.conv_input"""
    g, C = src_geom(s, H, W), s["C"]
    t = NS(geom=g, x=None, scale=None, shift=None, gate_p=None, gate_ab=None)
    if s["kind"] == "nchw":
        t.x = ro.grid((N, C, H, W), STEP_X, 12, torch.float32, gen)
    elif s["kind"] in ("plain", "up_plain"):
        t.x = ro.grid((N, g.H, g.W, C), STEP_X, 12, dtype, gen)
    else:
        # pooled sources draw from a small range, so 2x2 ties and all-negative windows are common
        t.x = ro.grid((N, g.H, g.W, C), STEP_X, 2 if s["kind"] == "pool_act" else 4, dtype, gen)
        t.scale, t.shift = _affine(C, gen)
    if s["gate"]:
        t.gate_p = torch.randint(0, 2, (N, g.H, g.W), generator=gen).float()
        t.gate_ab = torch.tensor(GATE_AB)
    t.spec = dict(kind=s["kind"], x=t.x, scale=t.scale, shift=t.shift, relu=s["relu"], gate_p=t.gate_p,
                  gate_ab=t.gate_ab, up=(g.up_h, g.up_w, g.pad_t, g.pad_l))
    return t


def src_unit(s):
    """the grid step of a source's values as the conv reads them"""
    if s["kind"] == "up_act":
        return STEP_X / 4   # four-corner blend with weights in {0, 1/2, 1}
    return STEP_X / 2 if s["gate"] else STEP_X


def cin(case):
    return sum(s["C"] for s in case["srcs"])


def _seed(case):
    return sum((i + 1) * b for i, b in enumerate(case["id"].encode())) % (2 ** 31)


def conv_operands(case):
    """every input tensor of a conv case, on the CPU, deterministic in the case id"""
    gen = torch.Generator().manual_seed(_seed(case))
    dtype, (N, H, W), Cin, Cout, k = DT[case["dt"]], case["shape"], cin(case), case["cout"], case["k"]
    o = NS(srcs=[src_operands(s, N, H, W, dtype, gen) for s in case["srcs"]])
    # forward: OIHW [Cout, Cin]; dgrad: the forward conv's weight [Cin_fwd = Cout, ...] is [Cin, Cout] here
    o.w = ro.grid((Cin, Cout, k, k) if case["dgrad"] else (Cout, Cin, k, k), STEP_W, 4, torch.float32, gen)
    o.old = o.old2 = o.bias = o.pool = o.code = o.bnb = o.gdata = o.gp = None
    split = Cout if case["split"] is None else case["split"]
    if case["out"] in ("f32", "f32_gated"):
        if case["accum"]:
            o.old = ro.grid((N, H, W, split), STEP_X, 12, torch.float32, gen)
        if case["accum2"]:
            o.old2 = ro.grid((N, H, W, Cout - split), STEP_X, 12, torch.float32, gen)
    if case["out"] == "f32_gated":
        o.gdata = ro.grid((N, H, W, Cout), STEP_X, 12, torch.float32, gen)
        o.gp = torch.randint(0, 2, (N, H, W), generator=gen).float()
    if case["out"] == "pool_bwd":
        Hs, Ws = 2 * H + case["pool_extra"][0], 2 * W + case["pool_extra"][1]
        o.pool = NS(x=ro.grid((N, Hs, Ws, Cout), STEP_X, 2, dtype, gen))   # small range: ties, all-negative windows
        o.pool.scale, o.pool.shift = _affine(Cout, gen)
        o.old = ro.grid((N, Hs, Ws, Cout), STEP_X, 12, torch.float32, gen)
        if case["pool_code"]:   # independent of the values: the kernel must route by the code
            o.code = torch.randint(0, 4, (N, H, W, Cout), generator=gen, dtype=torch.uint8)
    if case["bias"]:
        o.bias = ro.grid((Cout // 4,), STEP_X, 12, torch.float32, gen)
    if case["bnb"]:
        o.bnb = NS(y=ro.grid((N, H, W, Cout), STEP_X, 4, dtype, gen), mean=ro.grid((Cout,), STEP_X, 4, torch.float32, gen),
                   invstd=torch.tensor([(1.0, 2.0, 0.5)[c % 3] for c in range(Cout)]))
        o.bnb.scale, o.bnb.shift = _affine(Cout, gen)
    return o


def to_device(o, device):
    """a copy of an operand namespace with every tensor on `device`"""
    def mv(v):
        if isinstance(v, torch.Tensor):
            return v.to(device)
        if isinstance(v, NS):
            return NS(**{k: mv(x) for k, x in vars(v).items()})
        if isinstance(v, dict):
            return {k: mv(x) for k, x in v.items()}
        if isinstance(v, list):
            return [mv(x) for x in v]
        return v
    return mv(o)


def conv_reference(case, o):
    """fp64 expectations of a conv case from its operands (any device).  r.outs: name -> (ref64, abs_terms, unit,
    torch dtype); r.sums: name -> (ref64, abs_terms, unit) of the per-channel sums reduced over the partial rows"""
    dtype, (N, H, W), Cout, k = DT[case["dt"]], case["shape"], case["cout"], case["k"]
    x = ro.conv_input([t.spec for t in o.srcs], N, H, W, dtype)
    ux = min(src_unit(s) for s in case["srcs"])
    u = ux * STEP_W
    w = o.w.double()
    if case["dgrad"]:
        c = ro.conv_dgrad(x, w, k)
        y, a = c.dx, c.abs_terms
    else:
        c = ro.conv_fwd(x, w, k)
        y, a = c.y, c.abs_terms
    r = NS(x=x, y=y, outs={}, sums={}, unit=u)
    mode = case["out"]
    if mode == "y":
        r.outs["out"] = (y, a, u, dtype)
        if case["stats"]:
            st = ro.conv_stats(y)
            r.sums["stats"] = (torch.stack([st.sum, st.sumsq]), torch.stack([st.abs_sum, st.abs_sumsq]), (u, u * u))
        if case["bnb"]:
            b = o.bnb
            g = y.float().to(dtype)   # the gradient as stored
            s = ro.conv_bnb(g, b.y, b.scale, b.shift, 1, b.mean, b.invstd)
            r.sums["bnb"] = (torch.stack([s.sum_g, s.sum_gx]), torch.stack([s.abs_g, s.abs_gx]),
                             (u, u * STEP_X * 0.5))
        if case["act_out"]:
            C0 = case["srcs"][0]["C"]
            r.outs["act_out"] = (x[..., :C0], x[..., :C0].abs(), src_unit(case["srcs"][0]), dtype)
    elif mode in ("f32", "f32_gated"):
        split = Cout if case["split"] is None else case["split"]
        if mode == "f32_gated":
            s = torch.sigmoid(o.gp.double() * GATE_AB[0] + GATE_AB[1]).unsqueeze(-1)
            s = torch.where(s > 0.75, torch.ones_like(s), torch.full_like(s, 0.5))   # exactly 1 or 1/2
            y, a = y + s * o.gdata.double(), a + (s * o.gdata.double()).abs()
        y1, a1, y2, a2 = y[..., :split], a[..., :split], y[..., split:], a[..., split:]
        if o.old is not None:
            y1, a1 = y1 + o.old.double(), a1 + o.old.double().abs()
        if o.old2 is not None:
            y2, a2 = y2 + o.old2.double(), a2 + o.old2.double().abs()
        r.outs["out"] = (y1, a1, u, torch.float32)
        if split < Cout:
            r.outs["out2"] = (y2, a2, u, torch.float32)
    elif mode == "pool_bwd":
        p = o.pool
        Hs, Ws = p.x.shape[1:3]
        code = o.code if o.code is not None else ro.maxpool_act(p.x, p.scale, p.shift, 1, H, W).code
        r.code = code
        r.outs["out"] = (ro.pool_bwd(y, code, Hs, Ws, o.old), ro.pool_bwd(a, code, Hs, Ws, o.old.abs()), u, torch.float32)
    elif mode == "shuffle2":
        t = ro.convt_k2s2(x, w, o.bias)
        r.outs["out"] = (t.out, t.abs_terms, u, dtype)
    return r


def wgrad_operands(case):
    gen = torch.Generator().manual_seed(_seed(case))
    dtype, (N, H, W), Cin, Cout, k = DT[case["dt"]], case["shape"], cin(case), case["cout"], case["k"]
    o = NS(srcs=[src_operands(s, N, H, W, dtype, gen) for s in case["srcs"]])
    o.dy = ro.grid((N, H, W, Cout), STEP_DY, 8, dtype, gen)
    o.old = ro.grid((Cout, Cin, k, k), STEP_X, 12, torch.float32, gen) if case["accum"] else None
    return o


def wgrad_reference(case, o):
    dtype, (N, H, W), k = DT[case["dt"]], case["shape"], case["k"]
    x = ro.conv_input([t.spec for t in o.srcs], N, H, W, dtype)
    u = min(src_unit(s) for s in case["srcs"]) * STEP_DY
    c = ro.conv_wgrad(x, o.dy.double(), k)
    dw, a = c.dw, c.abs_terms
    if o.old is not None:
        dw, a = dw + o.old.double(), a + o.old.double().abs()
    return NS(x=x, outs={"dw": (dw, a, u, torch.float32)}, unit=u)


def exact_and_elem(case):
    """is every source of the case on the exact grid?  (fp32 operands through a gate's sigmoid keep the device's
    exp / rcp error, and up = 2·s has general bilinear weights: those cases are gated with ref_ops.check_elem)"""
    inexact = any((s["gate"] and case["dt"] == "fp32") or (s["kind"] == "up_act" and s["up"] == "conv")
                  for s in case["srcs"])
    return "elem" if inexact else "exact"


# ---- descriptors ------------------------------------------------------------------------------------

def fill_src(L, d, s, g, ptr):
    """one unet_src from a source spec, its geometry and a dict of addresses (data, scale, shift, gate_p, gate_ab)"""
    d.kind, d.C, d.H, d.W, d.data = KIND[s["kind"]], s["C"], g.H, g.W, ptr["data"]
    if s["kind"] in ("act", "pool_act", "up_act"):
        d.scale, d.shift, d.relu = ptr["scale"], ptr["shift"], s["relu"]
    if s["kind"] in ("up_act", "up_plain"):
        d.up_h, d.up_w, d.pad_t, d.pad_l, d.sh, d.sw = g.up_h, g.up_w, g.pad_t, g.pad_l, g.sh, g.sw
    if s["gate"]:
        d.gate_p, d.gate_ab = ptr["gate_p"], ptr["gate_ab"]


_DUMMY = dict(data=PTR, scale=PTR, shift=PTR, gate_p=PTR, gate_ab=PTR)


def conv_desc(L, case, src_ptrs=None, ptr=None):
    """the unet_conv_desc of a case.  ptr: name -> address of weight, out, out2, stats, bnb_*, act_out, bias,
    pool_code, pool_* and workspace (None: dummy non-null pointers, for the route queries)"""
    p = (lambda k: PTR) if ptr is None else (lambda k: ptr[k])
    N, H, W = case["shape"]
    d = L.ConvDesc()
    d.dtype, d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = CODE[case["dt"]], N, H, W, cin(case), case["cout"], \
        case["k"], len(case["srcs"])
    for i, s in enumerate(case["srcs"]):
        fill_src(L, d.src[i], s, src_geom(s, H, W), _DUMMY if src_ptrs is None else src_ptrs[i])
    d.weight, d.out, d.out_mode = p("weight"), p("out"), OUT[case["out"]]
    mode = case["out"]
    if mode == "y":
        if case["stats"]:
            d.stats = p("stats")
        if case["bnb"]:
            d.bnb_y, d.bnb_scale, d.bnb_shift, d.bnb_mean, d.bnb_invstd, d.bnb_stats = (
                p("bnb_y"), p("bnb_scale"), p("bnb_shift"), p("bnb_mean"), p("bnb_invstd"), p("bnb_stats"))
            d.bnb_relu = 1
        if case["act_out"]:
            d.act_out = p("act_out")
    elif mode in ("f32", "f32_gated"):
        d.split = case["cout"] if case["split"] is None else case["split"]
        d.accum, d.accum2 = case["accum"], case["accum2"]
        if d.split < case["cout"]:
            d.out2 = p("out2")
        if mode == "f32_gated":
            d.pool_src.data, d.pool_src.gate_p, d.pool_src.gate_ab = p("gdata"), p("gp"), p("gab")
    elif mode == "pool_bwd":
        ps = d.pool_src
        ps.kind, ps.C, ps.relu = KIND["act"], case["cout"], 1
        ps.H, ps.W = 2 * H + case["pool_extra"][0], 2 * W + case["pool_extra"][1]
        ps.data, ps.scale, ps.shift = p("pool_x"), p("pool_scale"), p("pool_shift")
        if case["pool_code"]:
            d.pool_code = p("pool_code")
    elif mode == "shuffle2" and case["bias"]:
        d.bias = p("bias")
    if case["ws"]:
        d.workspace = p("workspace")
    return d


def wgrad_desc(L, case, src_ptrs=None, ptr=None):
    p = (lambda k: PTR) if ptr is None else (lambda k: ptr[k])
    N, H, W = case["shape"]
    d = L.WgradDesc()
    d.dtype, d.N, d.H, d.W, d.Cin, d.Cout, d.ksize, d.nsrc = CODE[case["dt"]], N, H, W, cin(case), case["cout"], \
        case["k"], len(case["srcs"])
    for i, s in enumerate(case["srcs"]):
        fill_src(L, d.src[i], s, src_geom(s, H, W), _DUMMY if src_ptrs is None else src_ptrs[i])
    d.dy, d.dw, d.workspace, d.accum = p("dy"), p("dw"), p("workspace"), case["accum"]
    return d


def variant_of(so, d, wgrad=False):
    buf = ctypes.create_string_buffer(128)
    rc = (so.unet_wgrad_variant if wgrad else so.unet_conv_variant)(ctypes.byref(d), buf, 128)
    assert rc == 0
    return buf.value.decode()


def set_env(case, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        assert k in SWITCHES, k
        monkeypatch.setenv(k, v)


# ---- launching a case (GPU) -------------------------------------------------------------------------

class Guarded:
    """an output inside a larger buffer: `pad` elements of NaN before and after it, which must come back unchanged;
    the body starts as NaN too, or as `fill` where the call accumulates"""

    def __init__(self, shape, dtype, pad, device, fill=None):
        n = int(np.prod(shape))
        self.pad = (pad + 63) // 64 * 64   # keeps the body 16-byte aligned
        self.flat = torch.full((2 * self.pad + n,), float("nan"), dtype=dtype, device=device)
        self.body = self.flat[self.pad:self.pad + n].view(*shape)
        if fill is not None:
            self.body.copy_(fill)

    def ptr(self):
        return self.body.data_ptr()

    def check(self, what):
        assert self.flat[:self.pad].isnan().all() and self.flat[self.pad + self.body.numel():].isnan().all(), \
            (what, "wrote outside its output")


def _src_ptrs(o):
    keep, ptrs = [], []
    for t in o.srcs:
        ts = {k: getattr(t, k).contiguous() for k in ("x", "scale", "shift", "gate_p", "gate_ab") if getattr(t, k) is not None}
        keep.append(ts)
        ptrs.append(dict(data=ts["x"].data_ptr(), scale=ts["scale"].data_ptr() if "scale" in ts else None,
                         shift=ts["shift"].data_ptr() if "shift" in ts else None,
                         gate_p=ts["gate_p"].data_ptr() if "gate_p" in ts else None,
                         gate_ab=ts["gate_ab"].data_ptr() if "gate_ab" in ts else None))
    return keep, ptrs


def _nan_workspace(nbytes, device):
    return torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=device)


def launch_conv(L, R, case, o):
    """run unet_conv on a case's operands (on the GPU).  Returns NS(outs: name -> Guarded, stats / bnb: the partial
    tables reduced over their rows in fp64, or None).  Asserts the route before launching."""
    dev = o.w.device
    so, P = L.load(), R._PRECISIONS[case["dt"]]
    dtype, (N, H, W), Cout = DT[case["dt"]], case["shape"], case["cout"]
    keep, sp = _src_ptrs(o)
    wp = R.pack_weight(o.w, P, transpose=bool(case["dgrad"]))
    row = 16 * W   # pixels of one tile row
    mode, bufs, ptr = case["out"], {}, dict(weight=wp.data_ptr())
    split = Cout if case["split"] is None else case["split"]
    if mode == "y":
        bufs["out"] = Guarded((N, H, W, Cout), dtype, row * Cout, dev)
        if case["act_out"]:
            C0 = case["srcs"][0]["C"]
            bufs["act_out"] = Guarded((N, H, W, C0), dtype, row * C0, dev)
            ptr["act_out"] = bufs["act_out"].ptr()
        if case["bnb"]:
            b = o.bnb
            keep.append([b.y.contiguous()])
            ptr.update(bnb_y=keep[-1][0].data_ptr(), bnb_scale=b.scale.data_ptr(), bnb_shift=b.shift.data_ptr(),
                       bnb_mean=b.mean.data_ptr(), bnb_invstd=b.invstd.data_ptr())
    elif mode in ("f32", "f32_gated"):
        bufs["out"] = Guarded((N, H, W, split), torch.float32, row * split, dev, o.old)
        if split < Cout:
            bufs["out2"] = Guarded((N, H, W, Cout - split), torch.float32, row * (Cout - split), dev, o.old2)
            ptr["out2"] = bufs["out2"].ptr()
        if mode == "f32_gated":
            gab = torch.tensor(GATE_AB, device=dev)
            keep.append([gab])
            ptr.update(gdata=o.gdata.data_ptr(), gp=o.gp.data_ptr(), gab=gab.data_ptr())
    elif mode == "pool_bwd":
        Hs, Ws = o.pool.x.shape[1:3]
        bufs["out"] = Guarded((N, Hs, Ws, Cout), torch.float32, 32 * Ws * Cout, dev, o.old)
        ptr.update(pool_x=o.pool.x.data_ptr(), pool_scale=o.pool.scale.data_ptr(), pool_shift=o.pool.shift.data_ptr())
        if o.code is not None:
            ptr["pool_code"] = o.code.data_ptr()
    elif mode == "shuffle2":
        bufs["out"] = Guarded((N, 2 * H, 2 * W, Cout // 4), dtype, 2 * row * Cout, dev)
        if o.bias is not None:
            ptr["bias"] = o.bias.data_ptr()
    ptr["out"] = bufs["out"].ptr()
    # the tables are sized by the row query, asked of the descriptor as it will be launched (workspace, stats and
    # bnb pointers set: the route reads them)
    ptr.update(stats=PTR, bnb_stats=PTR, workspace=None)
    d = conv_desc(L, case, sp, ptr)
    nws = so.unet_conv_workspace(ctypes.byref(d))
    ws = _nan_workspace(nws, dev) if case["ws"] and nws else None
    d.workspace = ws.data_ptr() if ws is not None else None
    rows = so.unet_conv_stats_rows(ctypes.byref(d))
    st = bn = None
    if mode == "y" and case["stats"]:
        st = torch.full((2 * Cout * rows,), float("nan"), device=dev)
        d.stats = st.data_ptr()
    if mode == "y" and case["bnb"]:
        bn = torch.full((2 * rows * Cout,), float("nan"), device=dev)
        d.bnb_stats = bn.data_ptr()
    got = variant_of(so, d)
    assert got == case["variant"], (case["id"], "routes to", got)
    L.call("unet_conv", d, R.stream())
    torch.cuda.synchronize()
    r = NS(outs=bufs, stats=None, bnb=None, keep=(keep, wp, ws))
    if st is not None:
        assert torch.isfinite(st).all(), (case["id"], "stats rows left unwritten or not finite")
        r.stats = st.view(2, Cout, rows).double().sum(-1)
    if bn is not None:
        assert torch.isfinite(bn).all(), (case["id"], "bnb rows left unwritten or not finite")
        r.bnb = bn.view(2, rows, Cout).double().sum(1)
    return r


def launch_wgrad(L, R, case, o):
    dev = o.dy.device
    so = L.load()
    Cin, Cout, k = cin(case), case["cout"], case["k"]
    keep, sp = _src_ptrs(o)
    dy = o.dy.contiguous()
    dw = Guarded((Cout, Cin, k, k), torch.float32, 16 * Cin * k * k, dev, o.old)
    d = wgrad_desc(L, case, sp, dict(dy=dy.data_ptr(), dw=dw.ptr(), workspace=None))
    ws = _nan_workspace(max(so.unet_wgrad_workspace(ctypes.byref(d)), 16), dev)
    d.workspace = ws.data_ptr()
    got = variant_of(so, d, True)
    assert got == case["variant"], (case["id"], "routes to", got)
    L.call("unet_conv_wgrad", d, R.stream())
    torch.cuda.synchronize()
    return NS(outs={"dw": dw}, keep=(keep, dy, ws))


def check_outputs(case, run, ref):
    """every output against its fp64 expectation: bit equality (ref_ops.check_exact), or ref_ops.check_elem for the
    inexact-by-construction cases; the sentinels around every output untouched"""
    names = ("co", "ci", "kh", "kw") if "dw" in run.outs else ("n", "h", "w", "c")
    mods = (16, 16, 0, 0) if "dw" in run.outs else (0, 16, 32, 16)
    assert set(run.outs) == set(ref.outs), (set(run.outs), set(ref.outs))
    for name, buf in run.outs.items():
        want, a, u, dtype = ref.outs[name]
        what = f"{case['id']} [{case['variant']}] {name}"
        buf.check(what)
        if case["gate"] == "exact":
            assert ro.exact_units(a, u) < ro.EXACT_CAP, what
            ro.check_exact(buf.body, want, dtype, what, names, mods)
        else:
            ro.check_elem(buf.body, want, a, "fp32" if dtype == torch.float32 else case["dt"], what)


def check_sums(case, got, ref, gates, what):
    """a reduced partial table [2, C] against its expectation: equal where the table says the sum is exact, else
    ref_ops.check_sums with its defaults"""
    want, a, _ = ref
    for i, gate in enumerate(gates):
        w = f"{case['id']} [{case['variant']}] {what}[{i}]"
        if gate == "eq":
            bad = (got[i] != want[i]).nonzero().flatten().tolist()
            assert not bad, (w, "channels", bad[:8], "expected", want[i][bad[:4]].tolist(), "got", got[i][bad[:4]].tolist())
        else:
            ro.check_sums(got[i], want[i], a[i], w)


# ---- the tables -------------------------------------------------------------------------------------
# Variant names of tests/golden/routes.json that no case can reach, each with its reason.
UNREACHED = {
    "pw_wgrad_kernel<bf16>": "serves 1x1 weight gradients over >= 131072 pixels, above the 65536-pixel budget; below it "
                             "only through UNET_PW_WGRAD_MINP, which is cached at first use",
    "pw_wgrad_kernel<fp16>": "as pw_wgrad_kernel<bf16>",
}

# Shapes: 1x5x7 (smaller than any tile), 2x17x33 and 3x15x31 (one more / one less than the 16-row, 32-column tiles,
# N = 2 and 3), 1x24x40; 4x128x128 and 4x113x129 (>= 256 16-row tiles: the 16-row and 4-wave conv3 tiles, conv5's
# 16-row form), 4x64x64, 4x65x63 and 4x71x65 (>= 256 8-row tiles), 4x130x97 (more conv5 tiles than workgroups, with
# a ragged last round), 1x127x131 and 3x129x131 (pw: >= 16384 pixels, not a multiple of the 256-pixel block).
# `sums`: the gate of each per-channel sum of a stats / bnb table, in order (Σy, Σy²) then (Σg, Σg·x̂): 'eq' where
# its exact_units are below 2^24, else 'tol' (ref_ops.check_sums); test_conv_cases_cpu.py recomputes them.
# The f32_gated cases ("-dfg") are gated exactly although the device evaluates the sigmoid and nothing rounds
# gdata·σ to 16 bits: with the pre-sigmoid value exactly 0 or +40, sigmoidf_ (common.h: 1 / (1 + __expf(−x))) is
# 1 / (1 + 1) and 1 / (1 + 4e-18) — __expf(0) = exp2(0) is exactly 1, 1 + 4e-18 rounds to 1, and the reciprocal of a
# power of two is exact — so σ is exactly 1/2 or 1 by the formula, not by a measured run.  A change of sigmoidf_
# that loses this fails these cases, and the operands' gate must then move to check_elem with them.
CONV_CASES = [
    conv("bf16-k1-1x5x7-p3-20-ys", "bf16", 1, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<bf16,1,32>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-2x17x33-nchw6-40-ys", "bf16", 1, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<bf16,1,64>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-3x15x31-a20g-36-fx12A", "bf16", 1, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv_generic_kernel<bf16,1,64>", out='f32', split=12, accum2=1),
    conv("bf16-k1-2x17x33-pool12e10-20-y", "bf16", 1, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv_generic_kernel<bf16,1,32>"),
    conv("bf16-k1-3x15x31-up10p12-40-ys", "bf16", 1, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<bf16,1,64>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x5x7-upp6p11-33-y", "bf16", 1, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<bf16,1,64>"),
    conv("bf16-k1-1x24x40-a20+p12-40-ys", "bf16", 1, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv_generic_kernel<bf16,1,64>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-2x17x33-p20-20-dpbe11", "bf16", 1, (2, 17, 33), [S("plain", 20)], 20, "conv_generic_kernel<bf16,1,32>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("bf16-k1-3x15x31-p36-20-dpbc", "bf16", 1, (3, 15, 31), [S("plain", 36)], 20, "conv_generic_kernel<bf16,1,32>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("bf16-k1-1x24x40-p36-20-dyb", "bf16", 1, (1, 24, 40), [S("plain", 36)], 20, "conv_generic_kernel<bf16,1,32>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k1-3x15x31-p36-6-dfa", "bf16", 1, (3, 15, 31), [S("plain", 36)], 6, "conv_generic_kernel<bf16,1,32>", out='f32', dgrad=1, accum=1),
    conv("bf16-k1-2x17x33-p10-36-dfx12aA", "bf16", 1, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<bf16,1,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("bf16-k1-1x5x7-a6-20-fx8", "bf16", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<bf16,1,32>", out='f32', split=8),
    conv("bf16-k3-1x5x7-p3-20-ys", "bf16", 3, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<bf16,3,32>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-nchw6-40-ys", "bf16", 3, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<bf16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a20g-36-fx12A", "bf16", 3, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv_generic_kernel<bf16,3,64>", out='f32', split=12, accum2=1),
    conv("bf16-k3-2x17x33-pool12e10-20-y", "bf16", 3, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv_generic_kernel<bf16,3,32>"),
    conv("bf16-k3-3x15x31-up10p12-40-ys", "bf16", 3, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<bf16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x5x7-upp6p11-33-y", "bf16", 3, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<bf16,3,64>"),
    conv("bf16-k3-1x24x40-a20+p12-40-ys", "bf16", 3, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv_generic_kernel<bf16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-p20-20-dpbe11", "bf16", 3, (2, 17, 33), [S("plain", 20)], 20, "conv_generic_kernel<bf16,3,32>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("bf16-k3-3x15x31-p36-20-dpbc", "bf16", 3, (3, 15, 31), [S("plain", 36)], 20, "conv_generic_kernel<bf16,3,32>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("bf16-k3-1x24x40-p36-20-dyb", "bf16", 3, (1, 24, 40), [S("plain", 36)], 20, "conv_generic_kernel<bf16,3,32>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x15x31-p36-6-dfa", "bf16", 3, (3, 15, 31), [S("plain", 36)], 6, "conv_generic_kernel<bf16,3,32>", out='f32', dgrad=1, accum=1),
    conv("bf16-k3-2x17x33-p10-36-dfx12aA", "bf16", 3, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<bf16,3,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("bf16-k3-1x5x7-a6-20-fx8", "bf16", 3, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<bf16,3,32>", out='f32', split=8),
    conv("bf16-k1-2x17x33-p10-40-s2B", "bf16", 1, (2, 17, 33), [S("plain", 10)], 40, "conv_generic_kernel<bf16,1,64>", out='shuffle2', bias=1),
    conv("bf16-k1-1x5x7-a6-20-s2", "bf16", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<bf16,1,32>", out='shuffle2'),
    conv("fp16-k1-1x5x7-p3-20-ys", "fp16", 1, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<fp16,1,32>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-2x17x33-nchw6-40-ys", "fp16", 1, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<fp16,1,64>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-3x15x31-a20g-36-fx12A", "fp16", 1, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv_generic_kernel<fp16,1,64>", out='f32', split=12, accum2=1),
    conv("fp16-k1-2x17x33-pool12e10-20-y", "fp16", 1, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv_generic_kernel<fp16,1,32>"),
    conv("fp16-k1-3x15x31-up10p12-40-ys", "fp16", 1, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<fp16,1,64>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x5x7-upp6p11-33-y", "fp16", 1, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<fp16,1,64>"),
    conv("fp16-k1-1x24x40-a20+p12-40-ys", "fp16", 1, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv_generic_kernel<fp16,1,64>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-2x17x33-p20-20-dpbe11", "fp16", 1, (2, 17, 33), [S("plain", 20)], 20, "conv_generic_kernel<fp16,1,32>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("fp16-k1-3x15x31-p36-20-dpbc", "fp16", 1, (3, 15, 31), [S("plain", 36)], 20, "conv_generic_kernel<fp16,1,32>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp16-k1-1x24x40-p36-20-dyb", "fp16", 1, (1, 24, 40), [S("plain", 36)], 20, "conv_generic_kernel<fp16,1,32>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k1-3x15x31-p36-6-dfa", "fp16", 1, (3, 15, 31), [S("plain", 36)], 6, "conv_generic_kernel<fp16,1,32>", out='f32', dgrad=1, accum=1),
    conv("fp16-k1-2x17x33-p10-36-dfx12aA", "fp16", 1, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<fp16,1,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("fp16-k1-1x5x7-a6-20-fx8", "fp16", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp16,1,32>", out='f32', split=8),
    conv("fp16-k3-1x5x7-p3-20-ys", "fp16", 3, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<fp16,3,32>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-nchw6-40-ys", "fp16", 3, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<fp16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a20g-36-fx12A", "fp16", 3, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv_generic_kernel<fp16,3,64>", out='f32', split=12, accum2=1),
    conv("fp16-k3-2x17x33-pool12e10-20-y", "fp16", 3, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv_generic_kernel<fp16,3,32>"),
    conv("fp16-k3-3x15x31-up10p12-40-ys", "fp16", 3, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<fp16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x5x7-upp6p11-33-y", "fp16", 3, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<fp16,3,64>"),
    conv("fp16-k3-1x24x40-a20+p12-40-ys", "fp16", 3, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv_generic_kernel<fp16,3,64>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-p20-20-dpbe11", "fp16", 3, (2, 17, 33), [S("plain", 20)], 20, "conv_generic_kernel<fp16,3,32>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("fp16-k3-3x15x31-p36-20-dpbc", "fp16", 3, (3, 15, 31), [S("plain", 36)], 20, "conv_generic_kernel<fp16,3,32>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp16-k3-1x24x40-p36-20-dyb", "fp16", 3, (1, 24, 40), [S("plain", 36)], 20, "conv_generic_kernel<fp16,3,32>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x15x31-p36-6-dfa", "fp16", 3, (3, 15, 31), [S("plain", 36)], 6, "conv_generic_kernel<fp16,3,32>", out='f32', dgrad=1, accum=1),
    conv("fp16-k3-2x17x33-p10-36-dfx12aA", "fp16", 3, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<fp16,3,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("fp16-k3-1x5x7-a6-20-fx8", "fp16", 3, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp16,3,32>", out='f32', split=8),
    conv("fp16-k1-2x17x33-p10-40-s2B", "fp16", 1, (2, 17, 33), [S("plain", 10)], 40, "conv_generic_kernel<fp16,1,64>", out='shuffle2', bias=1),
    conv("fp16-k1-1x5x7-a6-20-s2", "fp16", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp16,1,32>", out='shuffle2'),
    conv("fp32-k1-1x5x7-p3-20-ys", "fp32", 1, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<fp32,1,32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-2x17x33-nchw6-40-ys", "fp32", 1, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<fp32,1,64>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-3x15x31-a20g-36-fx12A", "fp32", 1, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv2_kernel<fp32,1,2,2,2,1>", out='f32', gate='elem', split=12, accum2=1),
    conv("fp32-k1-2x17x33-pool12e10-20-y", "fp32", 1, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv2_kernel<fp32,1,2,2,1,4>"),
    conv("fp32-k1-3x15x31-up10p12-40-ys", "fp32", 1, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<fp32,1,64>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k1-1x5x7-upp6p11-33-y", "fp32", 1, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<fp32,1,64>"),
    conv("fp32-k1-1x24x40-a20+p12-40-ys", "fp32", 1, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv2_kernel<fp32,1,2,2,2,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-2x17x33-p20-20-dpbe11", "fp32", 1, (2, 17, 33), [S("plain", 20)], 20, "conv2_kernel<fp32,1,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("fp32-k1-3x15x31-p36-20-dpbc", "fp32", 1, (3, 15, 31), [S("plain", 36)], 20, "conv2_kernel<fp32,1,2,2,1,1>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp32-k1-1x24x40-p36-20-dyb", "fp32", 1, (1, 24, 40), [S("plain", 36)], 20, "conv2_kernel<fp32,1,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp32-k1-3x15x31-p36-6-dfa", "fp32", 1, (3, 15, 31), [S("plain", 36)], 6, "conv2_kernel<fp32,1,2,2,1,1>", out='f32', dgrad=1, accum=1),
    conv("fp32-k1-2x17x33-p10-36-dfx12aA", "fp32", 1, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<fp32,1,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("fp32-k1-1x5x7-a6-20-fx8", "fp32", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp32,1,32>", out='f32', split=8),
    conv("fp32-k3-1x5x7-p3-20-ys", "fp32", 3, (1, 5, 7), [S("plain", 3)], 20, "conv_generic_kernel<fp32,3,32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-2x17x33-nchw6-40-ys", "fp32", 3, (2, 17, 33), [S("nchw", 6)], 40, "conv_generic_kernel<fp32,3,64>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-3x15x31-a20g-36-fx12A", "fp32", 3, (3, 15, 31), [S("act", 20, gate=1)], 36, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', gate='elem', split=12, accum2=1),
    conv("fp32-k3-2x17x33-pool12e10-20-y", "fp32", 3, (2, 17, 33), [S("pool_act", 12, extra=(1, 0))], 20, "conv2_kernel<fp32,3,2,2,1,4>"),
    conv("fp32-k3-3x15x31-up10p12-40-ys", "fp32", 3, (3, 15, 31), [S("up_act", 10, pad=(1, 2))], 40, "conv_generic_kernel<fp32,3,64>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-1x5x7-upp6p11-33-y", "fp32", 3, (1, 5, 7), [S("up_plain", 6, pad=(1, 1))], 33, "conv_generic_kernel<fp32,3,64>"),
    conv("fp32-k3-1x24x40-a20+p12-40-ys", "fp32", 3, (1, 24, 40), [S("act", 20), S("plain", 12)], 40, "conv2_kernel<fp32,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-2x17x33-p20-20-dpbe11", "fp32", 3, (2, 17, 33), [S("plain", 20)], 20, "conv2_kernel<fp32,3,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 1)),
    conv("fp32-k3-3x15x31-p36-20-dpbc", "fp32", 3, (3, 15, 31), [S("plain", 36)], 20, "conv2_kernel<fp32,3,2,2,1,1>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp32-k3-1x24x40-p36-20-dyb", "fp32", 3, (1, 24, 40), [S("plain", 36)], 20, "conv2_kernel<fp32,3,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp32-k3-3x15x31-p36-6-dfa", "fp32", 3, (3, 15, 31), [S("plain", 36)], 6, "conv2_kernel<fp32,3,2,2,1,1>", out='f32', dgrad=1, accum=1),
    conv("fp32-k3-2x17x33-p10-36-dfx12aA", "fp32", 3, (2, 17, 33), [S("plain", 10)], 36, "conv_generic_kernel<fp32,3,64>", out='f32', dgrad=1, split=12, accum=1, accum2=1),
    conv("fp32-k3-1x5x7-a6-20-fx8", "fp32", 3, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp32,3,32>", out='f32', split=8),
    conv("fp32-k1-2x17x33-p10-40-s2B", "fp32", 1, (2, 17, 33), [S("plain", 10)], 40, "conv_generic_kernel<fp32,1,64>", out='shuffle2', bias=1),
    conv("fp32-k1-1x5x7-a6-20-s2", "fp32", 1, (1, 5, 7), [S("act", 6)], 20, "conv_generic_kernel<fp32,1,32>", out='shuffle2'),
    conv("fp32-k3-3x15x31-up10c-20-y", "fp32", 3, (3, 15, 31), [S("up_act", 10, up='conv')], 20, "conv_generic_kernel<fp32,3,32>", gate='elem'),
    conv("bf16-k1-1x5x7-p8-8-ys", "bf16", 1, (1, 5, 7), [S("plain", 8)], 8, "conv2_kernel<bf16,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-2x17x33-a40-32-ys", "bf16", 1, (2, 17, 33), [S("act", 40)], 32, "conv2_kernel<bf16,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-3x15x31-a72g-48-ys", "bf16", 1, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv2_kernel<bf16,1,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-2x17x33-p96-64-s2B", "bf16", 1, (2, 17, 33), [S("plain", 96)], 64, "conv2_kernel<bf16,1,2,2,2,1>", out='shuffle2', bias=1),
    conv("bf16-k1-3x15x31-a48-96-s2", "bf16", 1, (3, 15, 31), [S("act", 48)], 96, "conv2_kernel<bf16,1,2,2,2,1>", out='shuffle2'),
    conv("bf16-k1-1x24x40-a16+upp24p11-40-ys", "bf16", 1, (1, 24, 40), [S("act", 16), S("up_plain", 24, pad=(1, 1))], 40, "conv2_kernel<bf16,1,2,2,2,1>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-2x17x33-a32g+up16-48-ys", "bf16", 1, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16)], 48, "conv2_kernel<bf16,1,2,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-3x15x31-pool48e11-40-ys", "bf16", 1, (3, 15, 31), [S("pool_act", 48, extra=(1, 1))], 40, "conv2_kernel<bf16,1,2,2,2,4>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k1-3x15x31-pool16-16-y", "bf16", 1, (3, 15, 31), [S("pool_act", 16)], 16, "conv2_kernel<bf16,1,2,2,1,4>"),
    conv("bf16-k1-1x24x40-up40p21-192-y", "bf16", 1, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv2_kernel<bf16,1,2,2,2,4>"),
    conv("bf16-k1-2x17x33-p64-40-dfx16a", "bf16", 1, (2, 17, 33), [S("plain", 64)], 40, "conv2_kernel<bf16,1,2,2,2,1>", out='f32', dgrad=1, split=16, accum=1),
    conv("bf16-k1-3x15x31-p192-96-dfa", "bf16", 1, (3, 15, 31), [S("plain", 192)], 96, "conv2_kernel<bf16,1,2,2,2,1>", out='f32', dgrad=1, accum=1),
    conv("bf16-k1-1x24x40-p48-32-dyb", "bf16", 1, (1, 24, 40), [S("plain", 48)], 32, "conv2_kernel<bf16,1,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k1-3x15x31-p32-16-dpbe10", "bf16", 1, (3, 15, 31), [S("plain", 32)], 16, "conv2_kernel<bf16,1,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("bf16-k1-4x113x129-p40-48-ys", "bf16", 1, (4, 113, 129), [S("plain", 40)], 48, "conv2_kernel<bf16,1,4,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-4x128x128-a16+p24-128-ys", "bf16", 1, (4, 128, 128), [S("act", 16), S("plain", 24)], 128, "conv2_kernel<bf16,1,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-4x113x129-pool8-40-y", "bf16", 1, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<bf16,1,4,2,2,4>"),
    conv("bf16-k1-4x65x63-p40-192-ys", "bf16", 1, (4, 65, 63), [S("plain", 40)], 192, "conv2_kernel<bf16,1,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-4x64x64-up8-192-y", "bf16", 1, (4, 64, 64), [S("up_act", 8)], 192, "conv2_kernel<bf16,1,2,4,2,4>"),
    conv("bf16-k1-4x65x63-p72-192-dfx96A", "bf16", 1, (4, 65, 63), [S("plain", 72)], 192, "conv2_kernel<bf16,1,2,4,2,1>", out='f32', dgrad=1, split=96, accum2=1),
    conv("fp16-k1-1x5x7-p8-8-ys", "fp16", 1, (1, 5, 7), [S("plain", 8)], 8, "conv2_kernel<fp16,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-2x17x33-a40-32-ys", "fp16", 1, (2, 17, 33), [S("act", 40)], 32, "conv2_kernel<fp16,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-3x15x31-a72g-48-ys", "fp16", 1, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv2_kernel<fp16,1,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-2x17x33-p96-64-s2B", "fp16", 1, (2, 17, 33), [S("plain", 96)], 64, "conv2_kernel<fp16,1,2,2,2,1>", out='shuffle2', bias=1),
    conv("fp16-k1-3x15x31-a48-96-s2", "fp16", 1, (3, 15, 31), [S("act", 48)], 96, "conv2_kernel<fp16,1,2,2,2,1>", out='shuffle2'),
    conv("fp16-k1-1x24x40-a16+upp24p11-40-ys", "fp16", 1, (1, 24, 40), [S("act", 16), S("up_plain", 24, pad=(1, 1))], 40, "conv2_kernel<fp16,1,2,2,2,1>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-2x17x33-a32g+up16-48-ys", "fp16", 1, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16)], 48, "conv2_kernel<fp16,1,2,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-3x15x31-pool48e11-40-ys", "fp16", 1, (3, 15, 31), [S("pool_act", 48, extra=(1, 1))], 40, "conv2_kernel<fp16,1,2,2,2,4>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k1-3x15x31-pool16-16-y", "fp16", 1, (3, 15, 31), [S("pool_act", 16)], 16, "conv2_kernel<fp16,1,2,2,1,4>"),
    conv("fp16-k1-1x24x40-up40p21-192-y", "fp16", 1, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv2_kernel<fp16,1,2,2,2,4>"),
    conv("fp16-k1-2x17x33-p64-40-dfx16a", "fp16", 1, (2, 17, 33), [S("plain", 64)], 40, "conv2_kernel<fp16,1,2,2,2,1>", out='f32', dgrad=1, split=16, accum=1),
    conv("fp16-k1-3x15x31-p192-96-dfa", "fp16", 1, (3, 15, 31), [S("plain", 192)], 96, "conv2_kernel<fp16,1,2,2,2,1>", out='f32', dgrad=1, accum=1),
    conv("fp16-k1-1x24x40-p48-32-dyb", "fp16", 1, (1, 24, 40), [S("plain", 48)], 32, "conv2_kernel<fp16,1,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k1-3x15x31-p32-16-dpbe10", "fp16", 1, (3, 15, 31), [S("plain", 32)], 16, "conv2_kernel<fp16,1,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("fp16-k1-4x113x129-p40-48-ys", "fp16", 1, (4, 113, 129), [S("plain", 40)], 48, "conv2_kernel<fp16,1,4,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-4x128x128-a16+p24-128-ys", "fp16", 1, (4, 128, 128), [S("act", 16), S("plain", 24)], 128, "conv2_kernel<fp16,1,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-4x113x129-pool8-40-y", "fp16", 1, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<fp16,1,4,2,2,4>"),
    conv("fp16-k1-4x65x63-p40-192-ys", "fp16", 1, (4, 65, 63), [S("plain", 40)], 192, "conv2_kernel<fp16,1,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-4x64x64-up8-192-y", "fp16", 1, (4, 64, 64), [S("up_act", 8)], 192, "conv2_kernel<fp16,1,2,4,2,4>"),
    conv("fp16-k1-4x65x63-p72-192-dfx96A", "fp16", 1, (4, 65, 63), [S("plain", 72)], 192, "conv2_kernel<fp16,1,2,4,2,1>", out='f32', dgrad=1, split=96, accum2=1),
    conv("fp32-k1-1x5x7-p8-8-ys", "fp32", 1, (1, 5, 7), [S("plain", 8)], 8, "conv2_kernel<fp32,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-2x17x33-a40-32-ys", "fp32", 1, (2, 17, 33), [S("act", 40)], 32, "conv2_kernel<fp32,1,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-3x15x31-a72g-48-ys", "fp32", 1, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv2_kernel<fp32,1,2,2,2,1>", gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k1-2x17x33-p96-64-s2B", "fp32", 1, (2, 17, 33), [S("plain", 96)], 64, "conv2_kernel<fp32,1,2,2,2,1>", out='shuffle2', bias=1),
    conv("fp32-k1-3x15x31-a48-96-s2", "fp32", 1, (3, 15, 31), [S("act", 48)], 96, "conv2_kernel<fp32,1,2,2,2,1>", out='shuffle2'),
    conv("fp32-k1-1x24x40-a16+upp24p11-40-ys", "fp32", 1, (1, 24, 40), [S("act", 16), S("up_plain", 24, pad=(1, 1))], 40, "conv2_kernel<fp32,1,2,2,2,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k1-2x17x33-a32g+up16-48-ys", "fp32", 1, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16)], 48, "conv2_kernel<fp32,1,2,2,2,4>", gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k1-3x15x31-pool48e11-40-ys", "fp32", 1, (3, 15, 31), [S("pool_act", 48, extra=(1, 1))], 40, "conv2_kernel<fp32,1,2,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k1-3x15x31-pool16-16-y", "fp32", 1, (3, 15, 31), [S("pool_act", 16)], 16, "conv2_kernel<fp32,1,2,2,1,4>"),
    conv("fp32-k1-1x24x40-up40p21-192-y", "fp32", 1, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv2_kernel<fp32,1,2,2,2,4>"),
    conv("fp32-k1-2x17x33-p64-40-dfx16a", "fp32", 1, (2, 17, 33), [S("plain", 64)], 40, "conv2_kernel<fp32,1,2,2,2,1>", out='f32', dgrad=1, split=16, accum=1),
    conv("fp32-k1-3x15x31-p192-96-dfa", "fp32", 1, (3, 15, 31), [S("plain", 192)], 96, "conv2_kernel<fp32,1,2,2,2,1>", out='f32', dgrad=1, accum=1),
    conv("fp32-k1-1x24x40-p48-32-dyb", "fp32", 1, (1, 24, 40), [S("plain", 48)], 32, "conv2_kernel<fp32,1,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp32-k1-3x15x31-p32-16-dpbe10", "fp32", 1, (3, 15, 31), [S("plain", 32)], 16, "conv2_kernel<fp32,1,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("fp32-k1-4x113x129-p40-48-ys", "fp32", 1, (4, 113, 129), [S("plain", 40)], 48, "conv2_kernel<fp32,1,4,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k1-4x128x128-a16+p24-128-ys", "fp32", 1, (4, 128, 128), [S("act", 16), S("plain", 24)], 128, "conv2_kernel<fp32,1,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k1-4x113x129-pool8-40-y", "fp32", 1, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<fp32,1,4,2,2,4>"),
    conv("fp32-k1-4x65x63-p40-192-ys", "fp32", 1, (4, 65, 63), [S("plain", 40)], 192, "conv2_kernel<fp32,1,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k1-4x64x64-up8-192-y", "fp32", 1, (4, 64, 64), [S("up_act", 8)], 192, "conv2_kernel<fp32,1,2,4,2,4>"),
    conv("fp32-k1-4x65x63-p72-192-dfx96A", "fp32", 1, (4, 65, 63), [S("plain", 72)], 192, "conv2_kernel<fp32,1,2,4,2,1>", out='f32', dgrad=1, split=96, accum2=1),
    conv("bf16-k3-1x5x7-p8-8-ys", "bf16", 3, (1, 5, 7), [S("plain", 8)], 8, "conv3_kernel<bf16,3,2,2,1,4,1>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-1x5x7-a16-16-ys", "bf16", 3, (1, 5, 7), [S("act", 16)], 16, "conv3_kernel<bf16,3,2,2,1,4,1>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-a40-32-ys-nows", "bf16", 3, (2, 17, 33), [S("act", 40)], 32, "conv3_kernel<bf16,3,2,2,1,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a72g-48-ys-nows", "bf16", 3, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv3_kernel<bf16,3,2,2,2,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x24x40-p96-40-ys-nows", "bf16", 3, (1, 24, 40), [S("plain", 96)], 40, "conv3_kernel<bf16,3,2,2,2,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-a32g+up16p10-64-ys", "bf16", 3, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16, pad=(1, 0))], 64, "conv3_kernel<bf16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a32+up40-96-ys", "bf16", 3, (3, 15, 31), [S("act", 32), S("up_act", 40)], 96, "conv3_kernel<bf16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x24x40-a16g+p32-40-ys", "bf16", 3, (1, 24, 40), [S("act", 16, gate=1), S("plain", 32)], 40, "conv2_kernel<bf16,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-a48+upp16p01-48-ys", "bf16", 3, (2, 17, 33), [S("act", 48), S("up_plain", 16, pad=(0, 1))], 48, "conv2_kernel<bf16,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a32+upp8p11-40-ys", "bf16", 3, (3, 15, 31), [S("act", 32), S("up_plain", 8, pad=(1, 1))], 40, "conv3_kernel<bf16,3,2,2,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-pool48e11-40-ys", "bf16", 3, (2, 17, 33), [S("pool_act", 48, extra=(1, 1))], 40, "conv3_kernel<bf16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-pool16-16-ys", "bf16", 3, (3, 15, 31), [S("pool_act", 16)], 16, "conv3_kernel<bf16,3,2,2,1,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x24x40-up40p21-192-y", "bf16", 3, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv3_kernel<bf16,3,2,2,2,4,4>"),
    conv("bf16-k3-1x5x7-up8-8-y", "bf16", 3, (1, 5, 7), [S("up_act", 8)], 8, "conv3_kernel<bf16,3,2,2,1,4,4>"),
    conv("bf16-k3-2x17x33-p64-40-dfx16a-nows", "bf16", 3, (2, 17, 33), [S("plain", 64)], 40, "conv3_kernel<bf16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=16, accum=1),
    conv("bf16-k3-3x15x31-p192-96-dfa-nows", "bf16", 3, (3, 15, 31), [S("plain", 192)], 96, "conv3_kernel<bf16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, accum=1),
    conv("bf16-k3-3x15x31-p48-96-dfx48aA-nows", "bf16", 3, (3, 15, 31), [S("plain", 48)], 96, "conv3_kernel<bf16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=48, accum=1, accum2=1),
    conv("bf16-k3-1x5x7-p16-32-dfx8", "bf16", 3, (1, 5, 7), [S("plain", 16)], 32, "conv3_kernel<bf16,3,2,2,1,4,1>", out='f32', dgrad=1, split=8),
    conv("bf16-k3-2x17x33-p64-40-dfx24A-nows", "bf16", 3, (2, 17, 33), [S("plain", 64)], 40, "conv3_kernel<bf16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=24, accum2=1),
    conv("bf16-k3-1x24x40-p48-32-dyb-nows", "bf16", 3, (1, 24, 40), [S("plain", 48)], 32, "conv3_kernel<bf16,3,2,2,1,4,1>", dgrad=1, ws=0, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-p16-16-dyb", "bf16", 3, (2, 17, 33), [S("plain", 16)], 16, "conv3_kernel<bf16,3,2,2,1,4,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x15x31-p32-16-dpbe10", "bf16", 3, (3, 15, 31), [S("plain", 32)], 16, "conv3_kernel<bf16,3,2,2,1,4,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("bf16-k3-2x17x33-p96-48-dpbce11", "bf16", 3, (2, 17, 33), [S("plain", 96)], 48, "conv3_kernel<bf16,3,2,2,2,4,1>", out='pool_bwd', dgrad=1, pool_code=1, pool_extra=(1, 1)),
    conv("bf16-k3-1x24x40-p64-192-dpbc", "bf16", 3, (1, 24, 40), [S("plain", 64)], 192, "conv3_kernel<bf16,3,2,2,2,4,1>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("bf16-k3-1x5x7-p16-6-dpb", "bf16", 3, (1, 5, 7), [S("plain", 16)], 6, "conv2_kernel<bf16,3,2,2,1,1>", out='pool_bwd', dgrad=1),
    conv("bf16-k3-3x15x31-a16+p32-40-fx20A", "bf16", 3, (3, 15, 31), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<bf16,3,2,2,2,1>", out='f32', split=20, accum2=1),
    conv("bf16-k3-2x17x33-pool16-40-fx40", "bf16", 3, (2, 17, 33), [S("pool_act", 16)], 40, "conv2_kernel<bf16,3,2,2,2,4>", out='f32', split=40),
    conv("bf16-k3-4x113x129-p8-40-ys", "bf16", 3, (4, 113, 129), [S("plain", 8)], 40, "conv3_kernel<bf16,3,1,4,1,8,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x128x128-a16-72-ys", "bf16", 3, (4, 128, 128), [S("act", 16)], 72, "conv3_kernel<bf16,3,1,4,2,8,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x113x129-upp16p11-64-ys", "bf16", 3, (4, 113, 129), [S("up_plain", 16, pad=(1, 1))], 64, "conv3_kernel<bf16,3,1,4,1,8,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x128x128-pool8-40-ys", "bf16", 3, (4, 128, 128), [S("pool_act", 8)], 40, "conv3_kernel<bf16,3,4,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x113x129-a8g-40-fx40", "bf16", 3, (4, 113, 129), [S("act", 8, gate=1)], 40, "conv3_kernel<bf16,3,2,4,1,8,1>", out='f32', split=40),
    conv("bf16-k3-4x113x129-pool8-40-fx20", "bf16", 3, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<bf16,3,4,2,2,4>", out='f32', split=20),
    conv("bf16-k3-4x128x128-p16-72-dfx72a", "bf16", 3, (4, 128, 128), [S("plain", 16)], 72, "conv3_kernel<bf16,3,2,4,2,8,1>", out='f32', dgrad=1, split=72, accum=1),
    conv("bf16-k3-4x113x129-p16-40-dpb", "bf16", 3, (4, 113, 129), [S("plain", 16)], 40, "conv3_kernel<bf16,3,2,4,1,8,1>", out='pool_bwd', dgrad=1),
    conv("bf16-k3-4x113x129-a16+p32-40-pbc", "bf16", 3, (4, 113, 129), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<bf16,3,4,2,2,1>", out='pool_bwd', pool_code=1),
    conv("bf16-k3-4x128x128-p16+p32-72-fx36", "bf16", 3, (4, 128, 128), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<bf16,3,4,2,4,1>", out='f32', split=36),
    conv("bf16-k3-4x113x129-p16+p32-72-ys-CONV50", "bf16", 3, (4, 113, 129), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<bf16,3,2,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-p32+p16-72-ys-CONV50", "bf16", 3, (4, 113, 129), [S("plain", 32), S("plain", 16)], 72, "conv3_kernel<bf16,3,1,4,2,8,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x128x128-p32+p32-48-fx24-CONV50", "bf16", 3, (4, 128, 128), [S("plain", 32), S("plain", 32)], 48, "conv3_kernel<bf16,3,2,4,1,8,1>", out='f32', env={'UNET_CONV5': '0'}, split=24),
    conv("bf16-k3-4x65x63-p8-192-ys", "bf16", 3, (4, 65, 63), [S("plain", 8)], 192, "conv3_kernel<bf16,3,2,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x64x64-pool8-192-ys", "bf16", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv3_kernel<bf16,3,2,4,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x65x63-up16p11-192-y", "bf16", 3, (4, 65, 63), [S("up_act", 16, pad=(1, 1))], 192, "conv3_kernel<bf16,3,2,4,2,4,4>"),
    conv("bf16-k3-4x65x63-a16+p32-192-ys", "bf16", 3, (4, 65, 63), [S("act", 16), S("plain", 32)], 192, "conv2_kernel<bf16,3,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x64x64-pool8-192-fx96", "bf16", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv2_kernel<bf16,3,2,4,2,4>", out='f32', split=96),
    conv("bf16-k3-4x65x63-a32g+p32-192-ys-CONV50", "bf16", 3, (4, 65, 63), [S("act", 32, gate=1), S("plain", 32)], 192, "conv3_kernel<bf16,3,2,4,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x64x64-a48+up16-256-ys", "bf16", 3, (4, 64, 64), [S("act", 48), S("up_act", 16)], 256, "conv2_kernel<bf16,3,2,4,2,4>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x65x63-p16-192-dyb", "bf16", 3, (4, 65, 63), [S("plain", 16)], 192, "conv3_kernel<bf16,3,2,4,2,4,1>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x5x7-p8-8-ys", "fp16", 3, (1, 5, 7), [S("plain", 8)], 8, "conv3_kernel<fp16,3,2,2,1,4,1>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-1x5x7-a16-16-ys", "fp16", 3, (1, 5, 7), [S("act", 16)], 16, "conv3_kernel<fp16,3,2,2,1,4,1>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-a40-32-ys-nows", "fp16", 3, (2, 17, 33), [S("act", 40)], 32, "conv3_kernel<fp16,3,2,2,1,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a72g-48-ys-nows", "fp16", 3, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv3_kernel<fp16,3,2,2,2,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x24x40-p96-40-ys-nows", "fp16", 3, (1, 24, 40), [S("plain", 96)], 40, "conv3_kernel<fp16,3,2,2,2,4,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-a32g+up16p10-64-ys", "fp16", 3, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16, pad=(1, 0))], 64, "conv3_kernel<fp16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a32+up40-96-ys", "fp16", 3, (3, 15, 31), [S("act", 32), S("up_act", 40)], 96, "conv3_kernel<fp16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x24x40-a16g+p32-40-ys", "fp16", 3, (1, 24, 40), [S("act", 16, gate=1), S("plain", 32)], 40, "conv2_kernel<fp16,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-a48+upp16p01-48-ys", "fp16", 3, (2, 17, 33), [S("act", 48), S("up_plain", 16, pad=(0, 1))], 48, "conv2_kernel<fp16,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a32+upp8p11-40-ys", "fp16", 3, (3, 15, 31), [S("act", 32), S("up_plain", 8, pad=(1, 1))], 40, "conv3_kernel<fp16,3,2,2,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-pool48e11-40-ys", "fp16", 3, (2, 17, 33), [S("pool_act", 48, extra=(1, 1))], 40, "conv3_kernel<fp16,3,2,2,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-pool16-16-ys", "fp16", 3, (3, 15, 31), [S("pool_act", 16)], 16, "conv3_kernel<fp16,3,2,2,1,4,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x24x40-up40p21-192-y", "fp16", 3, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv3_kernel<fp16,3,2,2,2,4,4>"),
    conv("fp16-k3-1x5x7-up8-8-y", "fp16", 3, (1, 5, 7), [S("up_act", 8)], 8, "conv3_kernel<fp16,3,2,2,1,4,4>"),
    conv("fp16-k3-2x17x33-p64-40-dfx16a-nows", "fp16", 3, (2, 17, 33), [S("plain", 64)], 40, "conv3_kernel<fp16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=16, accum=1),
    conv("fp16-k3-3x15x31-p192-96-dfa-nows", "fp16", 3, (3, 15, 31), [S("plain", 192)], 96, "conv3_kernel<fp16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, accum=1),
    conv("fp16-k3-3x15x31-p48-96-dfx48aA-nows", "fp16", 3, (3, 15, 31), [S("plain", 48)], 96, "conv3_kernel<fp16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=48, accum=1, accum2=1),
    conv("fp16-k3-1x5x7-p16-32-dfx8", "fp16", 3, (1, 5, 7), [S("plain", 16)], 32, "conv3_kernel<fp16,3,2,2,1,4,1>", out='f32', dgrad=1, split=8),
    conv("fp16-k3-2x17x33-p64-40-dfx24A-nows", "fp16", 3, (2, 17, 33), [S("plain", 64)], 40, "conv3_kernel<fp16,3,2,2,2,4,1>", out='f32', dgrad=1, ws=0, split=24, accum2=1),
    conv("fp16-k3-1x24x40-p48-32-dyb-nows", "fp16", 3, (1, 24, 40), [S("plain", 48)], 32, "conv3_kernel<fp16,3,2,2,1,4,1>", dgrad=1, ws=0, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-p16-16-dyb", "fp16", 3, (2, 17, 33), [S("plain", 16)], 16, "conv3_kernel<fp16,3,2,2,1,4,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x15x31-p32-16-dpbe10", "fp16", 3, (3, 15, 31), [S("plain", 32)], 16, "conv3_kernel<fp16,3,2,2,1,4,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("fp16-k3-2x17x33-p96-48-dpbce11", "fp16", 3, (2, 17, 33), [S("plain", 96)], 48, "conv3_kernel<fp16,3,2,2,2,4,1>", out='pool_bwd', dgrad=1, pool_code=1, pool_extra=(1, 1)),
    conv("fp16-k3-1x24x40-p64-192-dpbc", "fp16", 3, (1, 24, 40), [S("plain", 64)], 192, "conv3_kernel<fp16,3,2,2,2,4,1>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp16-k3-1x5x7-p16-6-dpb", "fp16", 3, (1, 5, 7), [S("plain", 16)], 6, "conv2_kernel<fp16,3,2,2,1,1>", out='pool_bwd', dgrad=1),
    conv("fp16-k3-3x15x31-a16+p32-40-fx20A", "fp16", 3, (3, 15, 31), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<fp16,3,2,2,2,1>", out='f32', split=20, accum2=1),
    conv("fp16-k3-2x17x33-pool16-40-fx40", "fp16", 3, (2, 17, 33), [S("pool_act", 16)], 40, "conv2_kernel<fp16,3,2,2,2,4>", out='f32', split=40),
    conv("fp16-k3-4x113x129-p8-40-ys", "fp16", 3, (4, 113, 129), [S("plain", 8)], 40, "conv3_kernel<fp16,3,1,4,1,8,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x128x128-a16-72-ys", "fp16", 3, (4, 128, 128), [S("act", 16)], 72, "conv3_kernel<fp16,3,1,4,2,8,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x113x129-upp16p11-64-ys", "fp16", 3, (4, 113, 129), [S("up_plain", 16, pad=(1, 1))], 64, "conv3_kernel<fp16,3,1,4,1,8,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x128x128-pool8-40-ys", "fp16", 3, (4, 128, 128), [S("pool_act", 8)], 40, "conv3_kernel<fp16,3,4,2,2,4,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-a8g-40-fx40", "fp16", 3, (4, 113, 129), [S("act", 8, gate=1)], 40, "conv3_kernel<fp16,3,2,4,1,8,1>", out='f32', split=40),
    conv("fp16-k3-4x113x129-pool8-40-fx20", "fp16", 3, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<fp16,3,4,2,2,4>", out='f32', split=20),
    conv("fp16-k3-4x128x128-p16-72-dfx72a", "fp16", 3, (4, 128, 128), [S("plain", 16)], 72, "conv3_kernel<fp16,3,2,4,2,8,1>", out='f32', dgrad=1, split=72, accum=1),
    conv("fp16-k3-4x113x129-p16-40-dpb", "fp16", 3, (4, 113, 129), [S("plain", 16)], 40, "conv3_kernel<fp16,3,2,4,1,8,1>", out='pool_bwd', dgrad=1),
    conv("fp16-k3-4x113x129-a16+p32-40-pbc", "fp16", 3, (4, 113, 129), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<fp16,3,4,2,2,1>", out='pool_bwd', pool_code=1),
    conv("fp16-k3-4x128x128-p16+p32-72-fx36", "fp16", 3, (4, 128, 128), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<fp16,3,4,2,4,1>", out='f32', split=36),
    conv("fp16-k3-4x113x129-p16+p32-72-ys-CONV50", "fp16", 3, (4, 113, 129), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<fp16,3,2,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-p32+p16-72-ys-CONV50", "fp16", 3, (4, 113, 129), [S("plain", 32), S("plain", 16)], 72, "conv3_kernel<fp16,3,1,4,2,8,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x128x128-p32+p32-48-fx24-CONV50", "fp16", 3, (4, 128, 128), [S("plain", 32), S("plain", 32)], 48, "conv3_kernel<fp16,3,2,4,1,8,1>", out='f32', env={'UNET_CONV5': '0'}, split=24),
    conv("fp16-k3-4x65x63-p8-192-ys", "fp16", 3, (4, 65, 63), [S("plain", 8)], 192, "conv3_kernel<fp16,3,2,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x64x64-pool8-192-ys", "fp16", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv3_kernel<fp16,3,2,4,2,4,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x65x63-up16p11-192-y", "fp16", 3, (4, 65, 63), [S("up_act", 16, pad=(1, 1))], 192, "conv3_kernel<fp16,3,2,4,2,4,4>"),
    conv("fp16-k3-4x65x63-a16+p32-192-ys", "fp16", 3, (4, 65, 63), [S("act", 16), S("plain", 32)], 192, "conv2_kernel<fp16,3,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x64x64-pool8-192-fx96", "fp16", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv2_kernel<fp16,3,2,4,2,4>", out='f32', split=96),
    conv("fp16-k3-4x65x63-a32g+p32-192-ys-CONV50", "fp16", 3, (4, 65, 63), [S("act", 32, gate=1), S("plain", 32)], 192, "conv3_kernel<fp16,3,2,4,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x64x64-a48+up16-256-ys", "fp16", 3, (4, 64, 64), [S("act", 48), S("up_act", 16)], 256, "conv2_kernel<fp16,3,2,4,2,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x65x63-p16-192-dyb", "fp16", 3, (4, 65, 63), [S("plain", 16)], 192, "conv3_kernel<fp16,3,2,4,2,4,1>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("fp32-k3-1x5x7-p8-8-ys", "fp32", 3, (1, 5, 7), [S("plain", 8)], 8, "conv2_kernel<fp32,3,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-1x5x7-a16-16-ys", "fp32", 3, (1, 5, 7), [S("act", 16)], 16, "conv2_kernel<fp32,3,2,2,1,1>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-2x17x33-a40-32-ys-nows", "fp32", 3, (2, 17, 33), [S("act", 40)], 32, "conv2_kernel<fp32,3,2,2,1,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-3x15x31-a72g-48-ys-nows", "fp32", 3, (3, 15, 31), [S("act", 72, gate=1)], 48, "conv2_kernel<fp32,3,2,2,2,1>", ws=0, gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-1x24x40-p96-40-ys-nows", "fp32", 3, (1, 24, 40), [S("plain", 96)], 40, "conv2_kernel<fp32,3,2,2,2,1>", ws=0, stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-2x17x33-a32g+up16p10-64-ys", "fp32", 3, (2, 17, 33), [S("act", 32, gate=1), S("up_act", 16, pad=(1, 0))], 64, "conv2_kernel<fp32,3,2,2,2,4>", gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-3x15x31-a32+up40-96-ys", "fp32", 3, (3, 15, 31), [S("act", 32), S("up_act", 40)], 96, "conv2_kernel<fp32,3,2,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-1x24x40-a16g+p32-40-ys", "fp32", 3, (1, 24, 40), [S("act", 16, gate=1), S("plain", 32)], 40, "conv2_kernel<fp32,3,2,2,2,1>", gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-2x17x33-a48+upp16p01-48-ys", "fp32", 3, (2, 17, 33), [S("act", 48), S("up_plain", 16, pad=(0, 1))], 48, "conv2_kernel<fp32,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-3x15x31-a32+upp8p11-40-ys", "fp32", 3, (3, 15, 31), [S("act", 32), S("up_plain", 8, pad=(1, 1))], 40, "conv2_kernel<fp32,3,2,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-2x17x33-pool48e11-40-ys", "fp32", 3, (2, 17, 33), [S("pool_act", 48, extra=(1, 1))], 40, "conv2_kernel<fp32,3,2,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-3x15x31-pool16-16-ys", "fp32", 3, (3, 15, 31), [S("pool_act", 16)], 16, "conv2_kernel<fp32,3,2,2,1,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-1x24x40-up40p21-192-y", "fp32", 3, (1, 24, 40), [S("up_act", 40, pad=(2, 1))], 192, "conv2_kernel<fp32,3,2,2,2,4>"),
    conv("fp32-k3-1x5x7-up8-8-y", "fp32", 3, (1, 5, 7), [S("up_act", 8)], 8, "conv2_kernel<fp32,3,2,2,1,4>"),
    conv("fp32-k3-2x17x33-p64-40-dfx16a-nows", "fp32", 3, (2, 17, 33), [S("plain", 64)], 40, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', dgrad=1, ws=0, split=16, accum=1),
    conv("fp32-k3-3x15x31-p192-96-dfa-nows", "fp32", 3, (3, 15, 31), [S("plain", 192)], 96, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', dgrad=1, ws=0, accum=1),
    conv("fp32-k3-3x15x31-p48-96-dfx48aA-nows", "fp32", 3, (3, 15, 31), [S("plain", 48)], 96, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', dgrad=1, ws=0, split=48, accum=1, accum2=1),
    conv("fp32-k3-1x5x7-p16-32-dfx8", "fp32", 3, (1, 5, 7), [S("plain", 16)], 32, "conv2_kernel<fp32,3,2,2,1,1>", out='f32', dgrad=1, split=8),
    conv("fp32-k3-2x17x33-p64-40-dfx24A-nows", "fp32", 3, (2, 17, 33), [S("plain", 64)], 40, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', dgrad=1, ws=0, split=24, accum2=1),
    conv("fp32-k3-1x24x40-p48-32-dyb-nows", "fp32", 3, (1, 24, 40), [S("plain", 48)], 32, "conv2_kernel<fp32,3,2,2,1,1>", dgrad=1, ws=0, bnb=1, sums=('eq', 'eq')),
    conv("fp32-k3-2x17x33-p16-16-dyb", "fp32", 3, (2, 17, 33), [S("plain", 16)], 16, "conv2_kernel<fp32,3,2,2,1,1>", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp32-k3-3x15x31-p32-16-dpbe10", "fp32", 3, (3, 15, 31), [S("plain", 32)], 16, "conv2_kernel<fp32,3,2,2,1,1>", out='pool_bwd', dgrad=1, pool_extra=(1, 0)),
    conv("fp32-k3-2x17x33-p96-48-dpbce11", "fp32", 3, (2, 17, 33), [S("plain", 96)], 48, "conv2_kernel<fp32,3,2,2,2,1>", out='pool_bwd', dgrad=1, pool_code=1, pool_extra=(1, 1)),
    conv("fp32-k3-1x24x40-p64-192-dpbc", "fp32", 3, (1, 24, 40), [S("plain", 64)], 192, "conv2_kernel<fp32,3,2,2,2,1>", out='pool_bwd', dgrad=1, pool_code=1),
    conv("fp32-k3-1x5x7-p16-6-dpb", "fp32", 3, (1, 5, 7), [S("plain", 16)], 6, "conv2_kernel<fp32,3,2,2,1,1>", out='pool_bwd', dgrad=1),
    conv("fp32-k3-3x15x31-a16+p32-40-fx20A", "fp32", 3, (3, 15, 31), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<fp32,3,2,2,2,1>", out='f32', split=20, accum2=1),
    conv("fp32-k3-2x17x33-pool16-40-fx40", "fp32", 3, (2, 17, 33), [S("pool_act", 16)], 40, "conv2_kernel<fp32,3,2,2,2,4>", out='f32', split=40),
    conv("fp32-k3-4x113x129-p8-40-ys", "fp32", 3, (4, 113, 129), [S("plain", 8)], 40, "conv2_kernel<fp32,3,4,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x128x128-a16-72-ys", "fp32", 3, (4, 128, 128), [S("act", 16)], 72, "conv2_kernel<fp32,3,4,2,4,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x113x129-upp16p11-64-ys", "fp32", 3, (4, 113, 129), [S("up_plain", 16, pad=(1, 1))], 64, "conv2_kernel<fp32,3,4,2,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x128x128-pool8-40-ys", "fp32", 3, (4, 128, 128), [S("pool_act", 8)], 40, "conv2_kernel<fp32,3,4,2,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x113x129-a8g-40-fx40", "fp32", 3, (4, 113, 129), [S("act", 8, gate=1)], 40, "conv2_kernel<fp32,3,4,2,2,1>", out='f32', gate='elem', split=40),
    conv("fp32-k3-4x113x129-pool8-40-fx20", "fp32", 3, (4, 113, 129), [S("pool_act", 8)], 40, "conv2_kernel<fp32,3,4,2,2,4>", out='f32', split=20),
    conv("fp32-k3-4x128x128-p16-72-dfx72a", "fp32", 3, (4, 128, 128), [S("plain", 16)], 72, "conv2_kernel<fp32,3,4,2,4,1>", out='f32', dgrad=1, split=72, accum=1),
    conv("fp32-k3-4x113x129-p16-40-dpb", "fp32", 3, (4, 113, 129), [S("plain", 16)], 40, "conv2_kernel<fp32,3,4,2,2,1>", out='pool_bwd', dgrad=1),
    conv("fp32-k3-4x113x129-a16+p32-40-pbc", "fp32", 3, (4, 113, 129), [S("act", 16), S("plain", 32)], 40, "conv2_kernel<fp32,3,4,2,2,1>", out='pool_bwd', pool_code=1),
    conv("fp32-k3-4x128x128-p16+p32-72-fx36", "fp32", 3, (4, 128, 128), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<fp32,3,4,2,4,1>", out='f32', split=36),
    conv("fp32-k3-4x113x129-p16+p32-72-ys-CONV50", "fp32", 3, (4, 113, 129), [S("plain", 16), S("plain", 32)], 72, "conv2_kernel<fp32,3,4,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-4x113x129-p32+p16-72-ys-CONV50", "fp32", 3, (4, 113, 129), [S("plain", 32), S("plain", 16)], 72, "conv2_kernel<fp32,3,4,2,4,1>", env={'UNET_CONV5': '0'}, stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-4x128x128-p32+p32-48-fx24-CONV50", "fp32", 3, (4, 128, 128), [S("plain", 32), S("plain", 32)], 48, "conv2_kernel<fp32,3,4,2,2,1>", out='f32', env={'UNET_CONV5': '0'}, split=24),
    conv("fp32-k3-4x65x63-p8-192-ys", "fp32", 3, (4, 65, 63), [S("plain", 8)], 192, "conv2_kernel<fp32,3,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x64x64-pool8-192-ys", "fp32", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv2_kernel<fp32,3,2,4,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x65x63-up16p11-192-y", "fp32", 3, (4, 65, 63), [S("up_act", 16, pad=(1, 1))], 192, "conv2_kernel<fp32,3,2,4,2,4>"),
    conv("fp32-k3-4x65x63-a16+p32-192-ys", "fp32", 3, (4, 65, 63), [S("act", 16), S("plain", 32)], 192, "conv2_kernel<fp32,3,2,4,2,1>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-4x64x64-pool8-192-fx96", "fp32", 3, (4, 64, 64), [S("pool_act", 8)], 192, "conv2_kernel<fp32,3,2,4,2,4>", out='f32', split=96),
    conv("fp32-k3-4x65x63-a32g+p32-192-ys-CONV50", "fp32", 3, (4, 65, 63), [S("act", 32, gate=1), S("plain", 32)], 192, "conv2_kernel<fp32,3,2,4,2,1>", env={'UNET_CONV5': '0'}, gate='elem', stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-4x64x64-a48+up16-256-ys", "fp32", 3, (4, 64, 64), [S("act", 48), S("up_act", 16)], 256, "conv2_kernel<fp32,3,2,4,2,4>", stats=1, sums=('tol', 'tol')),
    conv("fp32-k3-4x65x63-p16-192-dyb", "fp32", 3, (4, 65, 63), [S("plain", 16)], 192, "conv2_kernel<fp32,3,2,4,2,1>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x128x128-p32-72-ys", "bf16", 3, (4, 128, 128), [S("plain", 32)], 72, "conv5_kernel<bf16,4>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-a48-96-yso", "bf16", 3, (4, 113, 129), [S("act", 48)], 96, "conv5_kernel<bf16,4>", stats=1, act_out=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x113x129-a40g-64-ys", "bf16", 3, (4, 113, 129), [S("act", 40, gate=1)], 64, "conv5_kernel<bf16,2>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x130x97-a32+p40-128-ys", "bf16", 3, (4, 130, 97), [S("act", 32), S("plain", 40)], 128, "conv5_kernel<bf16,4>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x130x97-a16g+p32-128-ys", "bf16", 3, (4, 130, 97), [S("act", 16, gate=1), S("plain", 32)], 128, "conv5_kernel<bf16,4>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x130x97-p48+p24-192-ys", "bf16", 3, (4, 130, 97), [S("plain", 48), S("plain", 24)], 192, "conv5_kernel<bf16,4>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-p96-64-dyb", "bf16", 3, (4, 113, 129), [S("plain", 96)], 64, "conv5_kernel<bf16,2>", dgrad=1, bnb=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x128x128-a32-64-yb", "bf16", 3, (4, 128, 128), [S("act", 32)], 64, "conv5_kernel<bf16,2>", bnb=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x113x129-p72-64-dfx32a", "bf16", 3, (4, 113, 129), [S("plain", 72)], 64, "conv5_kernel<bf16,2>", out='f32', dgrad=1, split=32, accum=1),
    conv("bf16-k3-4x128x128-p32-40-dfa", "bf16", 3, (4, 128, 128), [S("plain", 32)], 40, "conv5_kernel<bf16,2>", out='f32', dgrad=1, accum=1),
    conv("bf16-k3-4x113x129-p40-48-dfx24aA", "bf16", 3, (4, 113, 129), [S("plain", 40)], 48, "conv5_kernel<bf16,2>", out='f32', dgrad=1, split=24, accum=1, accum2=1),
    conv("bf16-k3-4x113x129-p32-64-dfx16A", "bf16", 3, (4, 113, 129), [S("plain", 32)], 64, "conv5_kernel<bf16,2>", out='f32', dgrad=1, split=16, accum2=1),
    conv("bf16-k3-4x130x97-p32-128-dfx64-CONV5_MI22", "bf16", 3, (4, 130, 97), [S("plain", 32)], 128, "conv5_kernel<bf16,2>", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '2'}, split=64),
    conv("bf16-k3-1x249x251-p24-128-ys", "bf16", 3, (1, 249, 251), [S("plain", 24)], 128, "conv5_kernel<bf16,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x249x251-a32g-64-ys", "bf16", 3, (1, 249, 251), [S("act", 32, gate=1)], 64, "conv5_kernel<bf16,2>", stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x64x64-p32-256-ys", "bf16", 3, (4, 64, 64), [S("plain", 32)], 256, "conv5_kernel<bf16,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x71x65-a48-192-yso", "bf16", 3, (4, 71, 65), [S("act", 48)], 192, "conv5_kernel<bf16,2>", stats=1, act_out=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x71x65-a32g+p16-192-ys", "bf16", 3, (4, 71, 65), [S("act", 32, gate=1), S("plain", 16)], 192, "conv5_kernel<bf16,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x71x65-p40-256-dyb", "bf16", 3, (4, 71, 65), [S("plain", 40)], 256, "conv5_kernel<bf16,2>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x71x65-p48-192-dfx96a", "bf16", 3, (4, 71, 65), [S("plain", 48)], 192, "conv5_kernel<bf16,2>", out='f32', dgrad=1, split=96, accum=1),
    conv("bf16-k3-4x130x97-a40-128-ys-CONV5_MI22", "bf16", 3, (4, 130, 97), [S("act", 40)], 128, "conv5_kernel<bf16,2>", env={'UNET_CONV5_MI2': '2'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x7x33-p24-8-ys-CONV51-CONV5_SPLIT0", "bf16", 3, (1, 7, 33), [S("plain", 24)], 8, "conv3_kernel<bf16,3,2,2,1,4,1>", env={'UNET_CONV5': '1', 'UNET_CONV5_SPLIT': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x5x7-p64-8-ys", "bf16", 3, (1, 5, 7), [S("plain", 64)], 8, "conv5_kernel<bf16,2>+splitk2", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-a64-64-ys", "bf16", 3, (2, 17, 33), [S("act", 64)], 64, "conv5_kernel<bf16,2>+splitk2", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a32g+p32-32-ys", "bf16", 3, (3, 15, 31), [S("act", 32, gate=1), S("plain", 32)], 32, "conv5_kernel<bf16,2>+splitk2", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-p128-16-dyb", "bf16", 3, (2, 17, 33), [S("plain", 128)], 16, "conv5_kernel<bf16,2>+splitk4", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x15x31-a128g-64-ys", "bf16", 3, (3, 15, 31), [S("act", 128, gate=1)], 64, "conv5_kernel<bf16,2>+splitk4", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x24x40-p128-128-dfx64a", "bf16", 3, (1, 24, 40), [S("plain", 128)], 128, "conv5_kernel<bf16,2>+splitk4", out='f32', dgrad=1, split=64, accum=1),
    conv("bf16-k3-1x5x7-p256-32-dfa", "bf16", 3, (1, 5, 7), [S("plain", 256)], 32, "conv5_kernel<bf16,2>+splitk8", out='f32', dgrad=1, accum=1),
    conv("bf16-k3-3x15x31-a256-128-ys", "bf16", 3, (3, 15, 31), [S("act", 256)], 128, "conv5_kernel<bf16,2>+splitk8", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-p256-64-dyb", "bf16", 3, (2, 17, 33), [S("plain", 256)], 64, "conv5_kernel<bf16,2>+splitk8", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-1x16x32-p256-8-dfx4A", "bf16", 3, (1, 16, 32), [S("plain", 256)], 8, "conv5_kernel<bf16,2>+splitk8", out='f32', dgrad=1, split=4, accum2=1),
    conv("bf16-k3-1x5x7-p64-8-ys-CONV5_MI20", "bf16", 3, (1, 5, 7), [S("plain", 64)], 8, "conv5_kernel<bf16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-a64-64-ys-CONV5_MI20", "bf16", 3, (2, 17, 33), [S("act", 64)], 64, "conv5_kernel<bf16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-a32g+p32-32-ys-CONV5_MI20", "bf16", 3, (3, 15, 31), [S("act", 32, gate=1), S("plain", 32)], 32, "conv5_kernel<bf16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-p128-16-dyb-CONV5_MI20", "bf16", 3, (2, 17, 33), [S("plain", 128)], 16, "conv5_kernel<bf16,4>+splitk4", dgrad=1, env={'UNET_CONV5_MI2': '0'}, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x15x31-a128g-64-ys-CONV5_MI20", "bf16", 3, (3, 15, 31), [S("act", 128, gate=1)], 64, "conv5_kernel<bf16,4>+splitk4", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-1x24x40-p128-128-dfx64a-CONV5_MI20", "bf16", 3, (1, 24, 40), [S("plain", 128)], 128, "conv5_kernel<bf16,4>+splitk4", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, split=64, accum=1),
    conv("bf16-k3-1x5x7-p256-32-dfa-CONV5_MI20", "bf16", 3, (1, 5, 7), [S("plain", 256)], 32, "conv5_kernel<bf16,4>+splitk8", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, accum=1),
    conv("bf16-k3-3x15x31-a256-128-ys-CONV5_MI20", "bf16", 3, (3, 15, 31), [S("act", 256)], 128, "conv5_kernel<bf16,4>+splitk8", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x17x33-p256-64-dyb-CONV5_MI20", "bf16", 3, (2, 17, 33), [S("plain", 256)], 64, "conv5_kernel<bf16,4>+splitk8", dgrad=1, env={'UNET_CONV5_MI2': '0'}, bnb=1, sums=('eq', 'eq')),
    conv("bf16-k3-1x16x32-p256-8-dfx4A-CONV5_MI20", "bf16", 3, (1, 16, 32), [S("plain", 256)], 8, "conv5_kernel<bf16,4>+splitk8", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, split=4, accum2=1),
    conv("bf16-k3-4x128x128-a32-256-ys-CONV5W1", "bf16", 3, (4, 128, 128), [S("act", 32)], 256, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-a48g-256-yso-CONV5W1", "bf16", 3, (4, 113, 129), [S("act", 48, gate=1)], 256, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, act_out=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-a32+p48-256-ys-CONV5W1", "bf16", 3, (4, 113, 129), [S("act", 32), S("plain", 48)], 256, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-p48-256-ys-CONV5W1", "bf16", 3, (4, 113, 129), [S("plain", 48)], 256, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-p32-256-dyb-CONV5W1", "bf16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<bf16>", dgrad=1, env={'UNET_CONV5W': '1'}, bnb=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x113x129-p32-256-dfx128-CONV5W1", "bf16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<bf16>", out='f32', dgrad=1, env={'UNET_CONV5W': '1'}, split=128),
    conv("bf16-k3-4x130x97-a32g+p32-512-ys-CONV5W1", "bf16", 3, (4, 130, 97), [S("act", 32, gate=1), S("plain", 32)], 512, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x113x129-p32-256-df-CONV5W1", "bf16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<bf16>", out='f32', dgrad=1, env={'UNET_CONV5W': '1'}),
    conv("bf16-k3-1x249x251-a32-256-ys-CONV5W1", "bf16", 3, (1, 249, 251), [S("act", 32)], 256, "conv5w_kernel<bf16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("bf16-k3-4x64x64-a32-512-ys-CONV5W1", "bf16", 3, (4, 64, 64), [S("act", 32)], 512, "conv5w_kernel<bf16,4>", env={'UNET_CONV5W': '1'}, stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-4x71x65-a48g+p16-512-yso-CONV5W1", "bf16", 3, (4, 71, 65), [S("act", 48, gate=1), S("plain", 16)], 512, "conv5w_kernel<bf16,4>", env={'UNET_CONV5W': '1'}, stats=1, act_out=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x128x128-p32-72-ys", "fp16", 3, (4, 128, 128), [S("plain", 32)], 72, "conv5_kernel<fp16,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-a48-96-yso", "fp16", 3, (4, 113, 129), [S("act", 48)], 96, "conv5_kernel<fp16,4>", stats=1, act_out=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x113x129-a40g-64-ys", "fp16", 3, (4, 113, 129), [S("act", 40, gate=1)], 64, "conv5_kernel<fp16,2>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x130x97-a32+p40-128-ys", "fp16", 3, (4, 130, 97), [S("act", 32), S("plain", 40)], 128, "conv5_kernel<fp16,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x130x97-a16g+p32-128-ys", "fp16", 3, (4, 130, 97), [S("act", 16, gate=1), S("plain", 32)], 128, "conv5_kernel<fp16,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x130x97-p48+p24-192-ys", "fp16", 3, (4, 130, 97), [S("plain", 48), S("plain", 24)], 192, "conv5_kernel<fp16,4>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-p96-64-dyb", "fp16", 3, (4, 113, 129), [S("plain", 96)], 64, "conv5_kernel<fp16,2>", dgrad=1, bnb=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x128x128-a32-64-yb", "fp16", 3, (4, 128, 128), [S("act", 32)], 64, "conv5_kernel<fp16,2>", bnb=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x113x129-p72-64-dfx32a", "fp16", 3, (4, 113, 129), [S("plain", 72)], 64, "conv5_kernel<fp16,2>", out='f32', dgrad=1, split=32, accum=1),
    conv("fp16-k3-4x128x128-p32-40-dfa", "fp16", 3, (4, 128, 128), [S("plain", 32)], 40, "conv5_kernel<fp16,2>", out='f32', dgrad=1, accum=1),
    conv("fp16-k3-4x113x129-p40-48-dfx24aA", "fp16", 3, (4, 113, 129), [S("plain", 40)], 48, "conv5_kernel<fp16,2>", out='f32', dgrad=1, split=24, accum=1, accum2=1),
    conv("fp16-k3-4x113x129-p32-64-dfx16A", "fp16", 3, (4, 113, 129), [S("plain", 32)], 64, "conv5_kernel<fp16,2>", out='f32', dgrad=1, split=16, accum2=1),
    conv("fp16-k3-4x130x97-p32-128-dfx64-CONV5_MI22", "fp16", 3, (4, 130, 97), [S("plain", 32)], 128, "conv5_kernel<fp16,2>", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '2'}, split=64),
    conv("fp16-k3-1x249x251-p24-128-ys", "fp16", 3, (1, 249, 251), [S("plain", 24)], 128, "conv5_kernel<fp16,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x249x251-a32g-64-ys", "fp16", 3, (1, 249, 251), [S("act", 32, gate=1)], 64, "conv5_kernel<fp16,2>", stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x64x64-p32-256-ys", "fp16", 3, (4, 64, 64), [S("plain", 32)], 256, "conv5_kernel<fp16,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x71x65-a48-192-yso", "fp16", 3, (4, 71, 65), [S("act", 48)], 192, "conv5_kernel<fp16,2>", stats=1, act_out=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x71x65-a32g+p16-192-ys", "fp16", 3, (4, 71, 65), [S("act", 32, gate=1), S("plain", 16)], 192, "conv5_kernel<fp16,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x71x65-p40-256-dyb", "fp16", 3, (4, 71, 65), [S("plain", 40)], 256, "conv5_kernel<fp16,2>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x71x65-p48-192-dfx96a", "fp16", 3, (4, 71, 65), [S("plain", 48)], 192, "conv5_kernel<fp16,2>", out='f32', dgrad=1, split=96, accum=1),
    conv("fp16-k3-4x130x97-a40-128-ys-CONV5_MI22", "fp16", 3, (4, 130, 97), [S("act", 40)], 128, "conv5_kernel<fp16,2>", env={'UNET_CONV5_MI2': '2'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x7x33-p24-8-ys-CONV51-CONV5_SPLIT0", "fp16", 3, (1, 7, 33), [S("plain", 24)], 8, "conv3_kernel<fp16,3,2,2,1,4,1>", env={'UNET_CONV5': '1', 'UNET_CONV5_SPLIT': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x5x7-p64-8-ys", "fp16", 3, (1, 5, 7), [S("plain", 64)], 8, "conv5_kernel<fp16,2>+splitk2", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-a64-64-ys", "fp16", 3, (2, 17, 33), [S("act", 64)], 64, "conv5_kernel<fp16,2>+splitk2", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a32g+p32-32-ys", "fp16", 3, (3, 15, 31), [S("act", 32, gate=1), S("plain", 32)], 32, "conv5_kernel<fp16,2>+splitk2", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-p128-16-dyb", "fp16", 3, (2, 17, 33), [S("plain", 128)], 16, "conv5_kernel<fp16,2>+splitk4", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x15x31-a128g-64-ys", "fp16", 3, (3, 15, 31), [S("act", 128, gate=1)], 64, "conv5_kernel<fp16,2>+splitk4", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x24x40-p128-128-dfx64a", "fp16", 3, (1, 24, 40), [S("plain", 128)], 128, "conv5_kernel<fp16,2>+splitk4", out='f32', dgrad=1, split=64, accum=1),
    conv("fp16-k3-1x5x7-p256-32-dfa", "fp16", 3, (1, 5, 7), [S("plain", 256)], 32, "conv5_kernel<fp16,2>+splitk8", out='f32', dgrad=1, accum=1),
    conv("fp16-k3-3x15x31-a256-128-ys", "fp16", 3, (3, 15, 31), [S("act", 256)], 128, "conv5_kernel<fp16,2>+splitk8", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-p256-64-dyb", "fp16", 3, (2, 17, 33), [S("plain", 256)], 64, "conv5_kernel<fp16,2>+splitk8", dgrad=1, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-1x16x32-p256-8-dfx4A", "fp16", 3, (1, 16, 32), [S("plain", 256)], 8, "conv5_kernel<fp16,2>+splitk8", out='f32', dgrad=1, split=4, accum2=1),
    conv("fp16-k3-1x5x7-p64-8-ys-CONV5_MI20", "fp16", 3, (1, 5, 7), [S("plain", 64)], 8, "conv5_kernel<fp16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-a64-64-ys-CONV5_MI20", "fp16", 3, (2, 17, 33), [S("act", 64)], 64, "conv5_kernel<fp16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-a32g+p32-32-ys-CONV5_MI20", "fp16", 3, (3, 15, 31), [S("act", 32, gate=1), S("plain", 32)], 32, "conv5_kernel<fp16,4>+splitk2", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-p128-16-dyb-CONV5_MI20", "fp16", 3, (2, 17, 33), [S("plain", 128)], 16, "conv5_kernel<fp16,4>+splitk4", dgrad=1, env={'UNET_CONV5_MI2': '0'}, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x15x31-a128g-64-ys-CONV5_MI20", "fp16", 3, (3, 15, 31), [S("act", 128, gate=1)], 64, "conv5_kernel<fp16,4>+splitk4", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x24x40-p128-128-dfx64a-CONV5_MI20", "fp16", 3, (1, 24, 40), [S("plain", 128)], 128, "conv5_kernel<fp16,4>+splitk4", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, split=64, accum=1),
    conv("fp16-k3-1x5x7-p256-32-dfa-CONV5_MI20", "fp16", 3, (1, 5, 7), [S("plain", 256)], 32, "conv5_kernel<fp16,4>+splitk8", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, accum=1),
    conv("fp16-k3-3x15x31-a256-128-ys-CONV5_MI20", "fp16", 3, (3, 15, 31), [S("act", 256)], 128, "conv5_kernel<fp16,4>+splitk8", env={'UNET_CONV5_MI2': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x17x33-p256-64-dyb-CONV5_MI20", "fp16", 3, (2, 17, 33), [S("plain", 256)], 64, "conv5_kernel<fp16,4>+splitk8", dgrad=1, env={'UNET_CONV5_MI2': '0'}, bnb=1, sums=('eq', 'eq')),
    conv("fp16-k3-1x16x32-p256-8-dfx4A-CONV5_MI20", "fp16", 3, (1, 16, 32), [S("plain", 256)], 8, "conv5_kernel<fp16,4>+splitk8", out='f32', dgrad=1, env={'UNET_CONV5_MI2': '0'}, split=4, accum2=1),
    conv("fp16-k3-4x128x128-a32-256-ys-CONV5W1", "fp16", 3, (4, 128, 128), [S("act", 32)], 256, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-a48g-256-yso-CONV5W1", "fp16", 3, (4, 113, 129), [S("act", 48, gate=1)], 256, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, act_out=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-a32+p48-256-ys-CONV5W1", "fp16", 3, (4, 113, 129), [S("act", 32), S("plain", 48)], 256, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-p48-256-ys-CONV5W1", "fp16", 3, (4, 113, 129), [S("plain", 48)], 256, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-p32-256-dyb-CONV5W1", "fp16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<fp16>", dgrad=1, env={'UNET_CONV5W': '1'}, bnb=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x113x129-p32-256-dfx128-CONV5W1", "fp16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<fp16>", out='f32', dgrad=1, env={'UNET_CONV5W': '1'}, split=128),
    conv("fp16-k3-4x130x97-a32g+p32-512-ys-CONV5W1", "fp16", 3, (4, 130, 97), [S("act", 32, gate=1), S("plain", 32)], 512, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x113x129-p32-256-df-CONV5W1", "fp16", 3, (4, 113, 129), [S("plain", 32)], 256, "conv5w_kernel<fp16>", out='f32', dgrad=1, env={'UNET_CONV5W': '1'}),
    conv("fp16-k3-1x249x251-a32-256-ys-CONV5W1", "fp16", 3, (1, 249, 251), [S("act", 32)], 256, "conv5w_kernel<fp16>", env={'UNET_CONV5W': '1'}, stats=1, sums=('tol', 'tol')),
    conv("fp16-k3-4x64x64-a32-512-ys-CONV5W1", "fp16", 3, (4, 64, 64), [S("act", 32)], 512, "conv5w_kernel<fp16,4>", env={'UNET_CONV5W': '1'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-4x71x65-a48g+p16-512-yso-CONV5W1", "fp16", 3, (4, 71, 65), [S("act", 48, gate=1), S("plain", 16)], 512, "conv5w_kernel<fp16,4>", env={'UNET_CONV5W': '1'}, stats=1, act_out=1, sums=('eq', 'tol')),
    conv("bf16-k1-4x64x64-p32-16-ys", "bf16", 1, (4, 64, 64), [S("plain", 32)], 16, "pw_conv_kernel<1,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-a96-48-ys", "bf16", 1, (1, 127, 131), [S("act", 96)], 48, "pw_conv_kernel<1,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-a64g-32-ys", "bf16", 1, (1, 127, 131), [S("act", 64, gate=1)], 32, "pw_conv_kernel<2,4>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-a32g-96-y", "bf16", 1, (1, 127, 131), [S("act", 32, gate=1)], 96, "pw_conv_kernel<2,4>"),
    conv("bf16-k1-4x64x64-p128-64-ys", "bf16", 1, (4, 64, 64), [S("plain", 128)], 64, "pw_conv_kernel<4,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-a64-192-ys", "bf16", 1, (1, 127, 131), [S("act", 64)], 192, "pw_conv_kernel<4,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-4x128x128-a32g-64-ys", "bf16", 1, (4, 128, 128), [S("act", 32, gate=1)], 64, "pw_conv_kernel<4,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-3x129x131-p64-64-ys", "bf16", 1, (3, 129, 131), [S("plain", 64)], 64, "pw_conv_kernel<4,2>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-p96-64-dyb", "bf16", 1, (1, 127, 131), [S("plain", 96)], 64, "pw_conv_kernel<4,2>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("bf16-k1-1x127x131-p64-32-df", "bf16", 1, (1, 127, 131), [S("plain", 64)], 32, "pw_conv_kernel<2,4>", out='f32', dgrad=1),
    conv("bf16-k1-1x127x131-p32-48-dfx16a", "bf16", 1, (1, 127, 131), [S("plain", 32)], 48, "pw_conv_kernel<1,4>", out='f32', dgrad=1, split=16, accum=1),
    conv("bf16-k1-4x64x64-p64-128-dfx64A", "bf16", 1, (4, 64, 64), [S("plain", 64)], 128, "pw_conv_kernel<4,2>", out='f32', dgrad=1, split=64, accum2=1),
    conv("bf16-k1-1x127x131-p32-16-dfx8aA", "bf16", 1, (1, 127, 131), [S("plain", 32)], 16, "pw_conv_kernel<1,4>", out='f32', dgrad=1, split=8, accum=1, accum2=1),
    conv("bf16-k1-1x127x131-p32-64-dfg", "bf16", 1, (1, 127, 131), [S("plain", 32)], 64, "pw_conv_kernel<4,2>", out='f32_gated', dgrad=1),
    conv("bf16-k1-1x127x131-p64-48-dfga", "bf16", 1, (1, 127, 131), [S("plain", 64)], 48, "pw_conv_kernel<1,4>", out='f32_gated', dgrad=1, accum=1),
    conv("bf16-k1-4x64x64-p128-32-dfga", "bf16", 1, (4, 64, 64), [S("plain", 128)], 32, "pw_conv_kernel<2,4>", out='f32_gated', dgrad=1, accum=1),
    conv("fp16-k1-4x64x64-p32-16-ys", "fp16", 1, (4, 64, 64), [S("plain", 32)], 16, "pw_conv_kernel<fp16,1,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-a96-48-ys", "fp16", 1, (1, 127, 131), [S("act", 96)], 48, "pw_conv_kernel<fp16,1,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-a64g-32-ys", "fp16", 1, (1, 127, 131), [S("act", 64, gate=1)], 32, "pw_conv_kernel<fp16,2,4>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-a32g-96-y", "fp16", 1, (1, 127, 131), [S("act", 32, gate=1)], 96, "pw_conv_kernel<fp16,2,4>"),
    conv("fp16-k1-4x64x64-p128-64-ys", "fp16", 1, (4, 64, 64), [S("plain", 128)], 64, "pw_conv_kernel<fp16,4,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-a64-192-ys", "fp16", 1, (1, 127, 131), [S("act", 64)], 192, "pw_conv_kernel<fp16,4,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-4x128x128-a32g-64-ys", "fp16", 1, (4, 128, 128), [S("act", 32, gate=1)], 64, "pw_conv_kernel<fp16,4,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-3x129x131-p64-64-ys", "fp16", 1, (3, 129, 131), [S("plain", 64)], 64, "pw_conv_kernel<fp16,4,2>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-p96-64-dyb", "fp16", 1, (1, 127, 131), [S("plain", 96)], 64, "pw_conv_kernel<fp16,4,2>", dgrad=1, bnb=1, sums=('eq', 'tol')),
    conv("fp16-k1-1x127x131-p64-32-df", "fp16", 1, (1, 127, 131), [S("plain", 64)], 32, "pw_conv_kernel<fp16,2,4>", out='f32', dgrad=1),
    conv("fp16-k1-1x127x131-p32-48-dfx16a", "fp16", 1, (1, 127, 131), [S("plain", 32)], 48, "pw_conv_kernel<fp16,1,4>", out='f32', dgrad=1, split=16, accum=1),
    conv("fp16-k1-4x64x64-p64-128-dfx64A", "fp16", 1, (4, 64, 64), [S("plain", 64)], 128, "pw_conv_kernel<fp16,4,2>", out='f32', dgrad=1, split=64, accum2=1),
    conv("fp16-k1-1x127x131-p32-16-dfx8aA", "fp16", 1, (1, 127, 131), [S("plain", 32)], 16, "pw_conv_kernel<fp16,1,4>", out='f32', dgrad=1, split=8, accum=1, accum2=1),
    conv("fp16-k1-1x127x131-p32-64-dfg", "fp16", 1, (1, 127, 131), [S("plain", 32)], 64, "pw_conv_kernel<fp16,4,2>", out='f32_gated', dgrad=1),
    conv("fp16-k1-1x127x131-p64-48-dfga", "fp16", 1, (1, 127, 131), [S("plain", 64)], 48, "pw_conv_kernel<fp16,1,4>", out='f32_gated', dgrad=1, accum=1),
    conv("fp16-k1-4x64x64-p128-32-dfga", "fp16", 1, (4, 64, 64), [S("plain", 128)], 32, "pw_conv_kernel<fp16,2,4>", out='f32_gated', dgrad=1, accum=1),
    conv("bf16-k3-1x5x7-nchw1-8-ys", "bf16", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_fwd_kernel<bf16>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-nchw3-64-ys", "bf16", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_fwd_mfma_kernel<bf16>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x15x31-nchw1-64-ys", "bf16", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_fwd_mfma_kernel<bf16>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-1x24x40-nchw4-64-ys", "bf16", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_fwd_kernel<bf16>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-2x17x33-nchw2-40-ys", "bf16", 3, (2, 17, 33), [S("nchw", 2)], 40, "smallcin_fwd_kernel<bf16>", stats=1, sums=('eq', 'eq')),
    conv("bf16-k3-3x70x100-nchw3-64-ys", "bf16", 3, (3, 70, 100), [S("nchw", 3)], 64, "smallcin_fwd_mfma_kernel<bf16>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-2x130x129-nchw1-64-ys", "bf16", 3, (2, 130, 129), [S("nchw", 1)], 64, "smallcin_fwd_mfma_kernel<bf16>", stats=1, sums=('eq', 'tol')),
    conv("bf16-k3-3x15x31-nchw3-64-ys-SMALLCIN_MFMA0", "bf16", 3, (3, 15, 31), [S("nchw", 3)], 64, "smallcin_fwd_kernel<bf16>", env={'UNET_SMALLCIN_MFMA': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-1x5x7-nchw1-8-ys", "fp16", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_fwd_kernel<fp16>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-nchw3-64-ys", "fp16", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_fwd_mfma_kernel<fp16>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x15x31-nchw1-64-ys", "fp16", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_fwd_mfma_kernel<fp16>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-1x24x40-nchw4-64-ys", "fp16", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_fwd_kernel<fp16>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-2x17x33-nchw2-40-ys", "fp16", 3, (2, 17, 33), [S("nchw", 2)], 40, "smallcin_fwd_kernel<fp16>", stats=1, sums=('eq', 'eq')),
    conv("fp16-k3-3x70x100-nchw3-64-ys", "fp16", 3, (3, 70, 100), [S("nchw", 3)], 64, "smallcin_fwd_mfma_kernel<fp16>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-2x130x129-nchw1-64-ys", "fp16", 3, (2, 130, 129), [S("nchw", 1)], 64, "smallcin_fwd_mfma_kernel<fp16>", stats=1, sums=('eq', 'tol')),
    conv("fp16-k3-3x15x31-nchw3-64-ys-SMALLCIN_MFMA0", "fp16", 3, (3, 15, 31), [S("nchw", 3)], 64, "smallcin_fwd_kernel<fp16>", env={'UNET_SMALLCIN_MFMA': '0'}, stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-1x5x7-nchw1-8-ys", "fp32", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-2x17x33-nchw3-64-ys", "fp32", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-3x15x31-nchw1-64-ys", "fp32", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-1x24x40-nchw4-64-ys", "fp32", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-2x17x33-nchw2-40-ys", "fp32", 3, (2, 17, 33), [S("nchw", 2)], 40, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'eq')),
    conv("fp32-k3-3x70x100-nchw3-64-ys", "fp32", 3, (3, 70, 100), [S("nchw", 3)], 64, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-2x130x129-nchw1-64-ys", "fp32", 3, (2, 130, 129), [S("nchw", 1)], 64, "smallcin_fwd_kernel<fp32>", stats=1, sums=('eq', 'tol')),
    conv("fp32-k3-3x15x31-nchw3-64-ys-SMALLCIN_MFMA0", "fp32", 3, (3, 15, 31), [S("nchw", 3)], 64, "smallcin_fwd_kernel<fp32>", env={'UNET_SMALLCIN_MFMA': '0'}, stats=1, sums=('eq', 'eq')),
]

WGRAD_CASES = [
    wgrad("bf16-w1-1x5x7-p8-8", "bf16", 1, (1, 5, 7), [S("plain", 8)], 8, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-2x17x33-p40-20-a", "bf16", 1, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<bf16,1>", accum=1),
    wgrad("bf16-w1-3x15x31-a20-33", "bf16", 1, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<bf16,1>"),
    wgrad("bf16-w1-2x17x33-a64-64-a", "bf16", 1, (2, 17, 33), [S("act", 64)], 64, "wgrad2_kernel<bf16,1>", accum=1),
    wgrad("bf16-w1-3x15x31-a32g-128", "bf16", 1, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-1x24x40-pool96e11-48", "bf16", 1, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-3x15x31-up48p11-96-a", "bf16", 1, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad2_kernel<bf16,1>", accum=1),
    wgrad("bf16-w1-2x17x33-upp40p10-192", "bf16", 1, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-3x15x31-a16g+p32-64", "bf16", 1, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-2x17x33-a32+up16-40-a", "bf16", 1, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad2_kernel<bf16,1>", accum=1),
    wgrad("bf16-w1-1x24x40-a48+upp24p02-128", "bf16", 1, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-3x15x31-nchw6-16", "bf16", 1, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<bf16,1>"),
    wgrad("bf16-w1-1x5x7-p256-256", "bf16", 1, (1, 5, 7), [S("plain", 256)], 256, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-4x128x128-p16-16", "bf16", 1, (4, 128, 128), [S("plain", 16)], 16, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w1-4x113x129-a64-64-a", "bf16", 1, (4, 113, 129), [S("act", 64)], 64, "wgrad2_kernel<bf16,1>", accum=1),
    wgrad("bf16-w1-3x65x63-pool32-128", "bf16", 1, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w3-1x5x7-p8-8", "bf16", 3, (1, 5, 7), [S("plain", 8)], 8, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-2x17x33-p40-20-a", "bf16", 3, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-3x15x31-a20-33", "bf16", 3, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<bf16,3>"),
    wgrad("bf16-w3-2x17x33-a64-64-a", "bf16", 3, (2, 17, 33), [S("act", 64)], 64, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-3x15x31-a32g-128", "bf16", 3, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-1x24x40-pool96e11-48", "bf16", 3, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-3x15x31-up48p11-96-a", "bf16", 3, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-2x17x33-upp40p10-192", "bf16", 3, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-3x15x31-a16g+p32-64", "bf16", 3, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-2x17x33-a32+up16-40-a", "bf16", 3, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-1x24x40-a48+upp24p02-128", "bf16", 3, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-3x15x31-nchw6-16", "bf16", 3, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<bf16,3>"),
    wgrad("bf16-w3-1x5x7-p256-256", "bf16", 3, (1, 5, 7), [S("plain", 256)], 256, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-4x128x128-p16-16", "bf16", 3, (4, 128, 128), [S("plain", 16)], 16, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-4x113x129-a64-64-a", "bf16", 3, (4, 113, 129), [S("act", 64)], 64, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-3x65x63-pool32-128", "bf16", 3, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-1x5x7-nchw1-8", "bf16", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_wgrad_kernel<bf16>"),
    wgrad("bf16-w3-2x17x33-nchw3-64-a", "bf16", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_wgrad_mfma_kernel<bf16>", accum=1),
    wgrad("bf16-w3-3x15x31-nchw1-64", "bf16", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_wgrad_mfma_kernel<bf16>"),
    wgrad("bf16-w3-1x24x40-nchw4-64", "bf16", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_wgrad_kernel<bf16>"),
    wgrad("bf16-w3-3x70x100-nchw2-40-a", "bf16", 3, (3, 70, 100), [S("nchw", 2)], 40, "smallcin_wgrad_kernel<bf16>", accum=1),
    wgrad("bf16-w3-2x130x129-nchw3-64", "bf16", 3, (2, 130, 129), [S("nchw", 3)], 64, "smallcin_wgrad_mfma_kernel<bf16>"),
    wgrad("fp16-w1-1x5x7-p8-8", "fp16", 1, (1, 5, 7), [S("plain", 8)], 8, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-2x17x33-p40-20-a", "fp16", 1, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<fp16,1>", accum=1),
    wgrad("fp16-w1-3x15x31-a20-33", "fp16", 1, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<fp16,1>"),
    wgrad("fp16-w1-2x17x33-a64-64-a", "fp16", 1, (2, 17, 33), [S("act", 64)], 64, "wgrad2_kernel<fp16,1>", accum=1),
    wgrad("fp16-w1-3x15x31-a32g-128", "fp16", 1, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-1x24x40-pool96e11-48", "fp16", 1, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-3x15x31-up48p11-96-a", "fp16", 1, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad2_kernel<fp16,1>", accum=1),
    wgrad("fp16-w1-2x17x33-upp40p10-192", "fp16", 1, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-3x15x31-a16g+p32-64", "fp16", 1, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-2x17x33-a32+up16-40-a", "fp16", 1, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad2_kernel<fp16,1>", accum=1),
    wgrad("fp16-w1-1x24x40-a48+upp24p02-128", "fp16", 1, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-3x15x31-nchw6-16", "fp16", 1, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<fp16,1>"),
    wgrad("fp16-w1-1x5x7-p256-256", "fp16", 1, (1, 5, 7), [S("plain", 256)], 256, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-4x128x128-p16-16", "fp16", 1, (4, 128, 128), [S("plain", 16)], 16, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w1-4x113x129-a64-64-a", "fp16", 1, (4, 113, 129), [S("act", 64)], 64, "wgrad2_kernel<fp16,1>", accum=1),
    wgrad("fp16-w1-3x65x63-pool32-128", "fp16", 1, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w3-1x5x7-p8-8", "fp16", 3, (1, 5, 7), [S("plain", 8)], 8, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-2x17x33-p40-20-a", "fp16", 3, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-3x15x31-a20-33", "fp16", 3, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<fp16,3>"),
    wgrad("fp16-w3-2x17x33-a64-64-a", "fp16", 3, (2, 17, 33), [S("act", 64)], 64, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-3x15x31-a32g-128", "fp16", 3, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-1x24x40-pool96e11-48", "fp16", 3, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-3x15x31-up48p11-96-a", "fp16", 3, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-2x17x33-upp40p10-192", "fp16", 3, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-3x15x31-a16g+p32-64", "fp16", 3, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-2x17x33-a32+up16-40-a", "fp16", 3, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-1x24x40-a48+upp24p02-128", "fp16", 3, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-3x15x31-nchw6-16", "fp16", 3, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<fp16,3>"),
    wgrad("fp16-w3-1x5x7-p256-256", "fp16", 3, (1, 5, 7), [S("plain", 256)], 256, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-4x128x128-p16-16", "fp16", 3, (4, 128, 128), [S("plain", 16)], 16, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-4x113x129-a64-64-a", "fp16", 3, (4, 113, 129), [S("act", 64)], 64, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-3x65x63-pool32-128", "fp16", 3, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-1x5x7-nchw1-8", "fp16", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_wgrad_kernel<fp16>"),
    wgrad("fp16-w3-2x17x33-nchw3-64-a", "fp16", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_wgrad_mfma_kernel<fp16>", accum=1),
    wgrad("fp16-w3-3x15x31-nchw1-64", "fp16", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_wgrad_mfma_kernel<fp16>"),
    wgrad("fp16-w3-1x24x40-nchw4-64", "fp16", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_wgrad_kernel<fp16>"),
    wgrad("fp16-w3-3x70x100-nchw2-40-a", "fp16", 3, (3, 70, 100), [S("nchw", 2)], 40, "smallcin_wgrad_kernel<fp16>", accum=1),
    wgrad("fp16-w3-2x130x129-nchw3-64", "fp16", 3, (2, 130, 129), [S("nchw", 3)], 64, "smallcin_wgrad_mfma_kernel<fp16>"),
    wgrad("fp32-w1-1x5x7-p8-8", "fp32", 1, (1, 5, 7), [S("plain", 8)], 8, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-2x17x33-p40-20-a", "fp32", 1, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<fp32,1>", accum=1),
    wgrad("fp32-w1-3x15x31-a20-33", "fp32", 1, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-2x17x33-a64-64-a", "fp32", 1, (2, 17, 33), [S("act", 64)], 64, "wgrad_kernel<fp32,1>", accum=1),
    wgrad("fp32-w1-3x15x31-a32g-128", "fp32", 1, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad_kernel<fp32,1>", gate='elem'),
    wgrad("fp32-w1-1x24x40-pool96e11-48", "fp32", 1, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-3x15x31-up48p11-96-a", "fp32", 1, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad_kernel<fp32,1>", accum=1),
    wgrad("fp32-w1-2x17x33-upp40p10-192", "fp32", 1, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-3x15x31-a16g+p32-64", "fp32", 1, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad_kernel<fp32,1>", gate='elem'),
    wgrad("fp32-w1-2x17x33-a32+up16-40-a", "fp32", 1, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad_kernel<fp32,1>", accum=1),
    wgrad("fp32-w1-1x24x40-a48+upp24p02-128", "fp32", 1, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-3x15x31-nchw6-16", "fp32", 1, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-1x5x7-p256-256", "fp32", 1, (1, 5, 7), [S("plain", 256)], 256, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-4x128x128-p16-16", "fp32", 1, (4, 128, 128), [S("plain", 16)], 16, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-4x113x129-a64-64-a", "fp32", 1, (4, 113, 129), [S("act", 64)], 64, "wgrad_kernel<fp32,1>", accum=1),
    wgrad("fp32-w1-3x65x63-pool32-128", "fp32", 1, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad_kernel<fp32,1>"),
    wgrad("fp32-w1-3x15x31-up16c-16", "fp32", 1, (3, 15, 31), [S("up_act", 16, up='conv')], 16, "wgrad_kernel<fp32,1>", gate='elem'),
    wgrad("fp32-w3-1x5x7-p8-8", "fp32", 3, (1, 5, 7), [S("plain", 8)], 8, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-2x17x33-p40-20-a", "fp32", 3, (2, 17, 33), [S("plain", 40)], 20, "wgrad_kernel<fp32,3>", accum=1),
    wgrad("fp32-w3-3x15x31-a20-33", "fp32", 3, (3, 15, 31), [S("act", 20)], 33, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-2x17x33-a64-64-a", "fp32", 3, (2, 17, 33), [S("act", 64)], 64, "wgrad_kernel<fp32,3>", accum=1),
    wgrad("fp32-w3-3x15x31-a32g-128", "fp32", 3, (3, 15, 31), [S("act", 32, gate=1)], 128, "wgrad_kernel<fp32,3>", gate='elem'),
    wgrad("fp32-w3-1x24x40-pool96e11-48", "fp32", 3, (1, 24, 40), [S("pool_act", 96, extra=(1, 1))], 48, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-3x15x31-up48p11-96-a", "fp32", 3, (3, 15, 31), [S("up_act", 48, pad=(1, 1))], 96, "wgrad_kernel<fp32,3>", accum=1),
    wgrad("fp32-w3-2x17x33-upp40p10-192", "fp32", 3, (2, 17, 33), [S("up_plain", 40, pad=(1, 0))], 192, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-3x15x31-a16g+p32-64", "fp32", 3, (3, 15, 31), [S("act", 16, gate=1), S("plain", 32)], 64, "wgrad_kernel<fp32,3>", gate='elem'),
    wgrad("fp32-w3-2x17x33-a32+up16-40-a", "fp32", 3, (2, 17, 33), [S("act", 32), S("up_act", 16)], 40, "wgrad_kernel<fp32,3>", accum=1),
    wgrad("fp32-w3-1x24x40-a48+upp24p02-128", "fp32", 3, (1, 24, 40), [S("act", 48), S("up_plain", 24, pad=(0, 2))], 128, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-3x15x31-nchw6-16", "fp32", 3, (3, 15, 31), [S("nchw", 6)], 16, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-1x5x7-p256-256", "fp32", 3, (1, 5, 7), [S("plain", 256)], 256, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-4x128x128-p16-16", "fp32", 3, (4, 128, 128), [S("plain", 16)], 16, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-4x113x129-a64-64-a", "fp32", 3, (4, 113, 129), [S("act", 64)], 64, "wgrad_kernel<fp32,3>", accum=1),
    wgrad("fp32-w3-3x65x63-pool32-128", "fp32", 3, (3, 65, 63), [S("pool_act", 32)], 128, "wgrad_kernel<fp32,3>"),
    wgrad("fp32-w3-3x15x31-up16c-16", "fp32", 3, (3, 15, 31), [S("up_act", 16, up='conv')], 16, "wgrad_kernel<fp32,3>", gate='elem'),
    wgrad("fp32-w3-1x5x7-nchw1-8", "fp32", 3, (1, 5, 7), [S("nchw", 1)], 8, "smallcin_wgrad_kernel<fp32>"),
    wgrad("fp32-w3-2x17x33-nchw3-64-a", "fp32", 3, (2, 17, 33), [S("nchw", 3)], 64, "smallcin_wgrad_kernel<fp32>", accum=1),
    wgrad("fp32-w3-3x15x31-nchw1-64", "fp32", 3, (3, 15, 31), [S("nchw", 1)], 64, "smallcin_wgrad_kernel<fp32>"),
    wgrad("fp32-w3-1x24x40-nchw4-64", "fp32", 3, (1, 24, 40), [S("nchw", 4)], 64, "smallcin_wgrad_kernel<fp32>"),
    wgrad("fp32-w3-3x70x100-nchw2-40-a", "fp32", 3, (3, 70, 100), [S("nchw", 2)], 40, "smallcin_wgrad_kernel<fp32>", accum=1),
    wgrad("fp32-w3-2x130x129-nchw3-64", "fp32", 3, (2, 130, 129), [S("nchw", 3)], 64, "smallcin_wgrad_kernel<fp32>"),
    wgrad("bf16-w3-4x128x128-p64-64", "bf16", 3, (4, 128, 128), [S("plain", 64)], 64, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-4x113x129-a64-128-a", "bf16", 3, (4, 113, 129), [S("act", 64)], 128, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w3-4x113x129-a64g+p64-64", "bf16", 3, (4, 113, 129), [S("act", 64, gate=1), S("plain", 64)], 64, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-4x130x97-p128-192", "bf16", 3, (4, 130, 97), [S("plain", 128)], 192, "wgrad5_kernel<bf16>"),
    wgrad("bf16-w3-2x17x33-p64-64-WGRAD51", "bf16", 3, (2, 17, 33), [S("plain", 64)], 64, "wgrad5_kernel<bf16>", env={'UNET_WGRAD5': '1'}),
    wgrad("bf16-w3-1x5x7-a64g-128-a-WGRAD51", "bf16", 3, (1, 5, 7), [S("act", 64, gate=1)], 128, "wgrad5_kernel<bf16>", env={'UNET_WGRAD5': '1'}, accum=1),
    wgrad("bf16-w3-3x15x31-a64+p64-64-WGRAD51", "bf16", 3, (3, 15, 31), [S("act", 64), S("plain", 64)], 64, "wgrad5_kernel<bf16>", env={'UNET_WGRAD5': '1'}),
    wgrad("bf16-w3-4x65x63-a128-64-WGRAD51", "bf16", 3, (4, 65, 63), [S("act", 128)], 64, "wgrad5_kernel<bf16>", env={'UNET_WGRAD5': '1'}),
    wgrad("bf16-w3-4x128x128-p64-64-WGRAD50", "bf16", 3, (4, 128, 128), [S("plain", 64)], 64, "wgrad2_kernel<bf16,3>", env={'UNET_WGRAD5': '0'}),
    wgrad("bf16-w3-1x233x129-p128-192", "bf16", 3, (1, 233, 129), [S("plain", 128)], 192, "wgrad5_kernel<bf16>"),
    wgrad("bf16-w3-2x595x31-a128g-192-a", "bf16", 3, (2, 595, 31), [S("act", 128, gate=1)], 192, "wgrad5_kernel<bf16>", accum=1),
    wgrad("bf16-w3-1x233x129-a64+p64-192", "bf16", 3, (1, 233, 129), [S("act", 64), S("plain", 64)], 192, "wgrad5_kernel<bf16>"),
    wgrad("bf16-w3-1x50x33-a64-64-WGRAD51", "bf16", 3, (1, 50, 33), [S("act", 64)], 64, "wgrad5_kernel<bf16>", env={'UNET_WGRAD5': '1'}),
    wgrad("bf16-w3-1x337x97-p64-64", "bf16", 3, (1, 337, 97), [S("plain", 64)], 64, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w3-1x609x97-a64g-128-a", "bf16", 3, (1, 609, 97), [S("act", 64, gate=1)], 128, "wgrad2_kernel<bf16,3>", accum=1),
    wgrad("bf16-w1-1x609x97-a48-40", "bf16", 1, (1, 609, 97), [S("act", 48)], 40, "wgrad2_kernel<bf16,1>"),
    wgrad("bf16-w3-1x337x97-pool16-48", "bf16", 3, (1, 337, 97), [S("pool_act", 16)], 48, "wgrad2_kernel<bf16,3>"),
    wgrad("bf16-w1-1x337x97-p16+upp16p11-16-a", "bf16", 1, (1, 337, 97), [S("plain", 16), S("up_plain", 16, pad=(1, 1))], 16, "wgrad2_kernel<bf16,1>", accum=1),
    wgrad("fp16-w3-4x128x128-p64-64", "fp16", 3, (4, 128, 128), [S("plain", 64)], 64, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-4x113x129-a64-128-a", "fp16", 3, (4, 113, 129), [S("act", 64)], 128, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w3-4x113x129-a64g+p64-64", "fp16", 3, (4, 113, 129), [S("act", 64, gate=1), S("plain", 64)], 64, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-4x130x97-p128-192", "fp16", 3, (4, 130, 97), [S("plain", 128)], 192, "wgrad5_kernel<fp16>"),
    wgrad("fp16-w3-2x17x33-p64-64-WGRAD51", "fp16", 3, (2, 17, 33), [S("plain", 64)], 64, "wgrad5_kernel<fp16>", env={'UNET_WGRAD5': '1'}),
    wgrad("fp16-w3-1x5x7-a64g-128-a-WGRAD51", "fp16", 3, (1, 5, 7), [S("act", 64, gate=1)], 128, "wgrad5_kernel<fp16>", env={'UNET_WGRAD5': '1'}, accum=1),
    wgrad("fp16-w3-3x15x31-a64+p64-64-WGRAD51", "fp16", 3, (3, 15, 31), [S("act", 64), S("plain", 64)], 64, "wgrad5_kernel<fp16>", env={'UNET_WGRAD5': '1'}),
    wgrad("fp16-w3-4x65x63-a128-64-WGRAD51", "fp16", 3, (4, 65, 63), [S("act", 128)], 64, "wgrad5_kernel<fp16>", env={'UNET_WGRAD5': '1'}),
    wgrad("fp16-w3-4x128x128-p64-64-WGRAD50", "fp16", 3, (4, 128, 128), [S("plain", 64)], 64, "wgrad2_kernel<fp16,3>", env={'UNET_WGRAD5': '0'}),
    wgrad("fp16-w3-1x233x129-p128-192", "fp16", 3, (1, 233, 129), [S("plain", 128)], 192, "wgrad5_kernel<fp16>"),
    wgrad("fp16-w3-2x595x31-a128g-192-a", "fp16", 3, (2, 595, 31), [S("act", 128, gate=1)], 192, "wgrad5_kernel<fp16>", accum=1),
    wgrad("fp16-w3-1x233x129-a64+p64-192", "fp16", 3, (1, 233, 129), [S("act", 64), S("plain", 64)], 192, "wgrad5_kernel<fp16>"),
    wgrad("fp16-w3-1x50x33-a64-64-WGRAD51", "fp16", 3, (1, 50, 33), [S("act", 64)], 64, "wgrad5_kernel<fp16>", env={'UNET_WGRAD5': '1'}),
    wgrad("fp16-w3-1x337x97-p64-64", "fp16", 3, (1, 337, 97), [S("plain", 64)], 64, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w3-1x609x97-a64g-128-a", "fp16", 3, (1, 609, 97), [S("act", 64, gate=1)], 128, "wgrad2_kernel<fp16,3>", accum=1),
    wgrad("fp16-w1-1x609x97-a48-40", "fp16", 1, (1, 609, 97), [S("act", 48)], 40, "wgrad2_kernel<fp16,1>"),
    wgrad("fp16-w3-1x337x97-pool16-48", "fp16", 3, (1, 337, 97), [S("pool_act", 16)], 48, "wgrad2_kernel<fp16,3>"),
    wgrad("fp16-w1-1x337x97-p16+upp16p11-16-a", "fp16", 1, (1, 337, 97), [S("plain", 16), S("up_plain", 16, pad=(1, 1))], 16, "wgrad2_kernel<fp16,1>", accum=1),
]
