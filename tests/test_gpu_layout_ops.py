"""GPU op-level numerics of the pooling, materialise, layout and fill kernels of csrc/misc.hip —
unet_materialize_pool, unet_materialize (all source kinds, the vector fast path, the generic kernel and its channel
tail), unet_nchw_to_nhwc, unet_nhwc_to_nchw, unet_gated_to_nchw and unet_fill_f32 — against the fp64 references of
tests/ref_ops.py (proved against nn.functional in tests/test_ref_ops_cpu.py).  Outputs are NaN-filled before the
launch; one spare vector behind them must keep its NaN.

Gates
  copies, casts, codes   exact (bit for bit where a cast rounds)
  an affine              e = 2^-23·(|x·s| + |b|): the affine as one fma or as a multiply and an add, in fp32
  a 16-bit output        0.5·ulp_T(|ref| + e) + e, the form tests/test_gpu_materialize.py derives
  UP_ACT                 e = 2^-24·(8·Σ_taps w·m + 4·in_size·max_taps m), m = |x·s| + |b| (the same derivation)
  the gate's sigmoid     measured, not derived: GATE_SIG·|ref| on top, see test_gated_to_nchw"""

import pytest
import torch

import ref_ops as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
ERR_ARG = 1001
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BITS = {"fp32": torch.int32, "bf16": torch.int16, "fp16": torch.int16}
PRECS = ["bf16", "fp16", "fp32"]
U23, U24 = 2.0 ** -23, 2.0 ** -24
GATE_SIG = 4 * 7.1e-7        # test_gated_to_nchw


def _lr():
    from unet._hip import lib as L, runtime as R
    return L, R


def _code(prec):
    return _lr()[1]._PRECISIONS[prec].code


def _vec(prec):
    return 4 if prec == "fp32" else 8


def _src(kind, x, C, scale=None, shift=None, relu=0):
    L, R = _lr()
    s = L.Src()
    s.kind, s.C, s.H, s.W, s.data = kind, C, x.shape[1], x.shape[2], x.data_ptr()
    s.scale, s.shift, s.relu = R.vp(scale), R.vp(shift), int(relu)
    return s


def _out_tol(ref, e, prec):
    return 0.5 * RO.ulp(ref.abs() + e, DT[prec]) + e


def _close(got, ref, tol, what):
    assert torch.isfinite(got).all(), (what, "not finite")
    err = (got.double() - ref).abs()
    assert (err <= tol).all(), (what,) + RO._worst(err, tol + torch.zeros_like(err))


# ---- unet_materialize_pool -----------------------------------------------------------------------------

POOL_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 33, 20)]
POOL_PC = [(p, c) for p in ("bf16", "fp16") for c in (8, 16, 64)] + [("fp32", c) for c in (4, 8, 32)]


def _pool(prec, y, scale, shift, relu, N, H, W):
    L, R = _lr()
    C = y.shape[-1]
    out = torch.full((N * H * W * C + _vec(prec),), NAN, dtype=DT[prec], device=DEV)
    code = torch.full((N * H * W * C + 8,), 77, dtype=torch.uint8, device=DEV)
    s = _src(L.SRC_POOL_ACT, y, C, scale, shift, relu)
    L.call("unet_materialize_pool", _code(prec), s, N, H, W, R.vp(out), R.vp(code), R.stream())
    torch.cuda.synchronize()
    assert bool(out[N * H * W * C:].isnan().all()) and bool((code[N * H * W * C:] == 77).all())
    return out[:N * H * W * C].view(N, H, W, C), code[:N * H * W * C].view(N, H, W, C)


@pytest.mark.parametrize("pc", POOL_PC, ids=lambda pc: f"{pc[0]}-{pc[1]}")
def test_materialize_pool_exact_ties(pc):
    """y on multiples of 1/8 in [−4, 4], scale in {±0.5, ±1, ±2}, shift on multiples of 1/64: the affine is exact in
    fp32, ties are true ties and there are many (whole windows at 0 under the ReLU).  Values (the fp64 maximum
    cast to the output type) and codes equal the reference exactly: code 0 for an all-tied window, the first of
    two equal maxima otherwise.  Sources 2H x 2W and (2H+1) x (2W+1)."""
    prec, C = pc
    gen = torch.Generator(device=DEV).manual_seed(51 + C)
    choices = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV)
    all_tied = first_of_two = 0
    for N, H, W in POOL_SHAPES:
        for odd in (0, 1):
            for relu in (0, 1):
                y = (torch.randint(-32, 33, (N, 2 * H + odd, 2 * W + odd, C), generator=gen, device=DEV) / 8).to(DT[prec])
                scale = choices[torch.randint(0, 6, (C,), generator=gen, device=DEV)].contiguous()
                shift = (torch.randint(-64, 65, (C,), generator=gen, device=DEV) / 64).contiguous()
                out, code = _pool(prec, y, scale, shift, relu, N, H, W)
                ref = RO.maxpool_act(y, scale, shift, relu, H, W)
                what = (N, H, W, odd, relu)
                assert not out.isnan().any(), what
                assert torch.equal(out, ref.out.to(DT[prec])), what
                assert torch.equal(code, ref.code), what
                tied = (ref.win == ref.out.unsqueeze(3)).sum(3)
                all_tied += int(((tied == 4) & (code == 0)).sum())
                first_of_two += int(((tied >= 2) & (tied < 4)).sum())
    assert all_tied > 0 and first_of_two > 0


@pytest.mark.parametrize("pc", POOL_PC, ids=lambda pc: f"{pc[0]}-{pc[1]}")
def test_materialize_pool_random(pc):
    """random operands: the activation evaluated in fp32 (one fma) and gathered through the returned code reproduces
    `out` exactly and is >= every other activation of its window; `out` is within half an output ulp (plus the fma's
    2^-24) of the fp64 maximum"""
    prec, C = pc
    gen = torch.Generator(device=DEV).manual_seed(61 + C)
    for N, H, W in POOL_SHAPES:
        for odd, relu in ((0, 1), (1, 0), (1, 1)):
            y = torch.randn(N, 2 * H + odd, 2 * W + odd, C, generator=gen, device=DEV).to(DT[prec])
            scale = torch.randn(C, generator=gen, device=DEV)
            shift = torch.randn(C, generator=gen, device=DEV) * 0.3
            out, code = _pool(prec, y, scale, shift, relu, N, H, W)
            assert int(code.max()) <= 3
            # the fp32 fma: the product is exact in fp64 and the sum rounds once more, to fp32
            a32 = (y.double() * scale.double() + shift.double()).float()
            a32 = a32.clamp_min(0) if relu else a32
            win = RO.pool_windows(a32, H, W)
            picked = win.gather(3, code.long().unsqueeze(3)).squeeze(3)
            assert torch.equal(picked.to(DT[prec]), out), (N, H, W, odd, relu)
            assert bool((picked.unsqueeze(3) >= win).all())
            ref = RO.materialize("pool_act", y, H, W, scale, shift, relu)
            _close(out, ref.out, _out_tol(ref.out, U24 * ref.abs_terms, prec), (N, H, W, odd, relu))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("prec", PRECS)
def test_materialize_pool_nan(prec, relu):
    """one NaN per window position, in four separate windows: the NaN comes out, with that position's code (ATen:
    `val > max || isnan(val)`), with and without the ReLU (relu(NaN) is NaN)"""
    C = _vec(prec)
    y = torch.randn(1, 2, 8, C, device=DEV).to(DT[prec])
    for q in range(4):
        y[0, q >> 1, 2 * q + (q & 1), q % C] = NAN
    scale, shift = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    out, code = _pool(prec, y, scale, shift, relu, 1, 1, 4)
    ref = RO.maxpool_act(y, scale, shift, relu, 1, 4)
    for q in range(4):
        assert bool(out[0, 0, q, q % C].isnan()) and int(code[0, 0, q, q % C]) == q, (q, out[0, 0, q], code[0, 0, q])
    assert torch.equal(out.isnan(), ref.out.isnan()) and torch.equal(code, ref.code)
    assert torch.equal(out.nan_to_num(9.0), ref.out.to(DT[prec]).nan_to_num(9.0))


def test_materialize_pool_refuses_24_channels():
    L, R = _lr()
    y = torch.zeros(1, 2, 2, 24, dtype=torch.bfloat16, device=DEV)
    scale, shift = torch.ones(24, device=DEV), torch.zeros(24, device=DEV)
    out = torch.full((24,), NAN, dtype=torch.bfloat16, device=DEV)
    code = torch.full((24,), 77, dtype=torch.uint8, device=DEV)
    s = _src(L.SRC_POOL_ACT, y, 24, scale, shift, 1)
    assert L.load().unet_materialize_pool(L.BF16, s, 1, 1, 1, R.vp(out), R.vp(code), R.stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool((code == 77).all())


# ---- unet_materialize ----------------------------------------------------------------------------------

KINDS = ["plain", "act", "gated", "pool_act", "up_act", "up_plain"]
MAT_N, MAT_H, MAT_W = 2, 6, 10
UP = (4, 8, 1, 1)        # up_h, up_w, pad_t, pad_l: a (2, 4) source at x2, one pixel of padding all round


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", KINDS)
def test_materialize_kinds(kind, prec, monkeypatch):
    """every source kind at (N, H, W) = (2, 6, 10) and C = 16 (the vector fast path; for UP_ACT in 16 bits the
    LDS-tiled kernel, and the vector fast path in a second run under UNET_MAT_TILE=0), 24 (C / vec is no power of
    two: the generic kernel) and 13 (the generic kernel's C % VEC tail).  Plain copies are exact, the padding of the
    UP kinds is exact zeros, the element behind the last channel of the last pixel keeps its NaN."""
    L, R = _lr()
    N, H, W = MAT_N, MAT_H, MAT_W
    dt = DT[prec]
    gen = torch.Generator(device=DEV).manual_seed(71)
    sig = 0.0
    for C in (16, 24, 13):
        scale = torch.randn(C, generator=gen, device=DEV)
        shift = torch.randn(C, generator=gen, device=DEV) * 0.3
        hs, ws = {"pool_act": (2 * H, 2 * W), "up_act": (2, 4), "up_plain": (4, 8)}.get(kind, (H, W))
        x = torch.randn(N, hs, ws, C, generator=gen, device=DEV).to(dt)
        runs = [(r, None) for r in ((0,) if kind in ("plain", "up_plain") else (0, 1))]
        if kind == "up_act" and prec != "fp32" and C == 16:
            runs += [(r, "0") for r in (0, 1)]
        for relu, tile in runs:
            monkeypatch.delenv("UNET_MAT_TILE", raising=False)
            if tile is not None:
                monkeypatch.setenv("UNET_MAT_TILE", tile)
            p = ab = None
            if kind == "plain":
                s = _src(L.SRC_PLAIN, x, C)
                ref = RO.materialize("plain", x, H, W)
            elif kind == "up_plain":
                s = _src(L.SRC_UP_PLAIN, x, C)
                s.up_h, s.up_w, s.pad_t, s.pad_l = UP
                ref = RO.materialize("up_plain", x, H, W, up=UP)
            elif kind in ("act", "gated"):
                s = _src(L.SRC_ACT, x, C, scale, shift, relu)
                if kind == "gated":
                    p = torch.randn(N, H, W, generator=gen, device=DEV) * 2
                    ab = torch.tensor([1.3, -0.2], device=DEV)
                    s.gate_p, s.gate_ab = R.vp(p), R.vp(ab)
                ref = RO.materialize("act", x, H, W, scale, shift, relu, p, ab)
            elif kind == "pool_act":
                s = _src(L.SRC_POOL_ACT, x, C, scale, shift, relu)
                ref = RO.materialize("pool_act", x, H, W, scale, shift, relu)
            else:
                s = _src(L.SRC_UP_ACT, x, C, scale, shift, relu)
                s.up_h, s.up_w, s.pad_t, s.pad_l = UP
                s.sh, s.sw = R.up_scale(2, 4), R.up_scale(4, 8)
                ref = RO.materialize("up_act", x, H, W, scale, shift, relu, up=UP)
            n = N * H * W * C
            buf = torch.full((n + _vec(prec),), NAN, dtype=dt, device=DEV)
            L.call("unet_materialize", _code(prec), s, N, H, W, R.vp(buf), R.stream())
            torch.cuda.synchronize()
            out, what = buf[:n].view(N, H, W, C), (kind, prec, C, relu, tile)
            assert bool(buf[n:].isnan().all()), what
            if kind in ("plain", "up_plain"):
                assert torch.equal(out.view(BITS[prec]), ref.out.to(dt).view(BITS[prec])), what
            elif kind == "up_act":
                mag = ((x.double() * scale.double()).abs() + shift.double().abs()).permute(0, 3, 1, 2)
                t = RO.resize_terms(mag, UP[0], UP[1])
                e = U24 * (8 * t.sum_w + 4 * 4 * t.max_a).permute(0, 2, 3, 1)
                _close(out, ref.out, _out_tol(ref.out, RO.place(e, H, W, UP[2], UP[3]), prec), what)
            elif kind == "gated":
                gate = torch.sigmoid(ref.q).unsqueeze(-1)
                e = U23 * ref.abs_terms * gate + (GATE_SIG + U24) * ref.out.abs()
                _close(out, ref.out, _out_tol(ref.out, e, prec), what)
                s32 = torch.sigmoid(p * ab[0] + ab[1]).double()
                sig = max(sig, float(((s32 - torch.sigmoid(ref.q)).abs() / torch.sigmoid(ref.q)).max()))
            else:
                _close(out, ref.out, _out_tol(ref.out, U23 * ref.abs_terms, prec), what)
            if kind in ("up_act", "up_plain"):
                inside = torch.zeros(H, W, dtype=torch.bool, device=DEV)
                inside[UP[2]:UP[2] + UP[0], UP[3]:UP[3] + UP[1]] = True
                assert bool((out[:, ~inside] == 0).all()), "the padding must be exact zeros"
    if kind == "gated":
        print(f"\nmaterialize gated {prec}: fp32 torch sigmoid within {sig:.3e} (relative) of fp64")


# ---- layout ----------------------------------------------------------------------------------------------

LAYOUT_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 3, 1000, 701)]     # the last: 2103000 > 8192·256 elements


def _specials(prec):
    """rounding ties of the 16-bit type (to even, both ways), its subnormals and their ties, signed zeros"""
    if prec == "bf16":
        v = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 2.0 ** -133, 3 * 2.0 ** -134,
             2.0 ** -134, 1e-39, -1e-39, 3.3895e38]
    elif prec == "fp16":
        v = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 2.0 ** -24, 3 * 2.0 ** -25,
             2.0 ** -25, 1e-6, -1e-6, 65519.0]
    else:
        v = [1e-39, -1e-39, 2.0 ** -149]
    return torch.tensor(v + [0.0, -0.0], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_to_nhwc(shape, prec):
    """bit-exact against permute + round-to-nearest-even cast, with rounding ties and subnormals among the values"""
    L, R = _lr()
    N, C, H, W = shape
    torch.manual_seed(81)
    x = torch.randn(N, C, H, W, device=DEV)
    sp = _specials(prec)
    flat = x.view(-1)
    if flat.numel() >= sp.numel():
        flat[:: max(1, flat.numel() // sp.numel())][:sp.numel()] = sp
    else:
        flat[0] = sp[0]
    n = x.numel()
    buf = torch.full((n + 8,), NAN, dtype=DT[prec], device=DEV)
    L.call("unet_nchw_to_nhwc", _code(prec), N, C, H, W, R.vp(x), R.vp(buf), R.stream())
    torch.cuda.synchronize()
    want = RO.nchw_to_nhwc(x).contiguous().to(DT[prec])
    assert torch.equal(buf[:n].view(N, H, W, C).view(BITS[prec]), want.view(BITS[prec]))
    assert bool(buf[n:].isnan().all())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nhwc_to_nchw(shape, prec):
    """without the affine: an exact widening copy; with it: relu?(x·s + b) within 2^-23·(|x·s| + |b|); ReLU 0 / 1"""
    L, R = _lr()
    N, C, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(82)
    x = torch.randn(N, H, W, C, generator=gen, device=DEV).to(DT[prec])
    scale, shift = torch.randn(C, generator=gen, device=DEV), torch.randn(C, generator=gen, device=DEV) * 0.3
    n = x.numel()
    for affine, relu in ((0, 0), (0, 1), (1, 0), (1, 1)):
        buf = torch.full((n + 4,), NAN, device=DEV)
        L.call("unet_nhwc_to_nchw", _code(prec), N, C, H, W, R.vp(x), R.vp(scale) if affine else None,
               R.vp(shift) if affine else None, relu, R.vp(buf), R.stream())
        torch.cuda.synchronize()
        ref = RO.nhwc_to_nchw(x, scale if affine else None, shift if affine else None, relu)
        _close(buf[:n].view(N, C, H, W), ref.out, U23 * ref.abs_terms * affine, (affine, relu))
        assert bool(buf[n:].isnan().all())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gated_to_nchw(shape, prec):
    """relu?(x·s + b)·sigmoid(p·a + b') as NCHW fp32: 2^-23·(|x·s| + |b|)·sigmoid for the affine, 2^-24·|ref| for the
    product and GATE_SIG·|ref| for the sigmoid (__expf, and q = p·a + b' in fp32).  Measured on these inputs
    (MI355X): the sigmoid formed in plain fp32 torch is within 7.1e-7 (relative) of fp64 (the largest shape; 4.9e-7
    on test_materialize_kinds' inputs); GATE_SIG = 4 × 7.1e-7 = 2.84e-6."""
    L, R = _lr()
    N, C, H, W = shape
    gen = torch.Generator(device=DEV).manual_seed(83)
    x = torch.randn(N, H, W, C, generator=gen, device=DEV).to(DT[prec])
    scale, shift = torch.randn(C, generator=gen, device=DEV), torch.randn(C, generator=gen, device=DEV) * 0.3
    p = (torch.randn(N, H, W, generator=gen, device=DEV) * 2).contiguous()
    ab = torch.tensor([1.3, -0.2], device=DEV)
    n = x.numel()
    sig = 0.0
    for relu in (0, 1):
        buf = torch.full((n + 4,), NAN, device=DEV)
        L.call("unet_gated_to_nchw", _code(prec), N, C, H, W, R.vp(x), R.vp(scale), R.vp(shift), relu, R.vp(p), R.vp(ab),
               R.vp(buf), R.stream())
        torch.cuda.synchronize()
        ref = RO.gated_to_nchw(x, scale, shift, relu, p, ab)
        gate = torch.sigmoid(ref.q)
        tol = U23 * ref.abs_terms * gate + (GATE_SIG + U24) * ref.out.abs()
        _close(buf[:n].view(N, C, H, W), ref.out, tol, relu)
        assert bool(buf[n:].isnan().all())
        s32 = torch.sigmoid(p * ab[0] + ab[1]).double().unsqueeze(1)
        sig = max(sig, float(((s32 - gate).abs() / gate).max()))
    print(f"\ngated_to_nchw {prec} {shape}: fp32 torch sigmoid within {sig:.3e} (relative) of fp64")


@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 3])
def test_fill_f32(n):
    """n values written, the 32 guard elements on either side untouched"""
    L, R = _lr()
    buf = torch.full((n + 64,), 7.0, device=DEV)
    buf[32:32 + n] = NAN
    L.call("unet_fill_f32", buf[32:].data_ptr(), n, -2.5, R.stream())
    torch.cuda.synchronize()
    assert bool((buf[32:32 + n] == -2.5).all())
    assert bool((buf[:32] == 7.0).all()) and bool((buf[32 + n:] == 7.0).all())
