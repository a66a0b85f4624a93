"""CPU: the case tables of the exact-grid convolution tests (tests/conv_cases.py) are sound before any of them runs
on a GPU.  Every case reaches the kernel instantiation it names (the route queries launch nothing), every variant
name of tests/golden/routes.json is covered by a case or listed in UNREACHED with a reason, every case's operands
meet the exactness condition Σ|terms| / unit < 2^24 by the fp64 reference alone, and the tables hold the partial
tiles, channel tails, epilogues and source kinds each kernel family serves."""

import json
import math
from collections import Counter, defaultdict
from pathlib import Path

import pytest
import torch

import conv_cases as CC
import ref_ops as RO

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def lib():
    from unet._hip import lib as L
    assert L.library_path().exists(), "libunet_hip.so not built (run __graft_entry__.build())"
    return L, L.load()


def family(variant):
    for prefix, fam in (("smallcin", "smallcin"), ("pw_", "pw"), ("conv_generic", "generic"), ("conv5w", "conv5w"),
                        ("conv3", "conv3"), ("conv2", "conv2"), ("wgrad5", "wgrad5"), ("wgrad2", "wgrad2"),
                        ("wgrad_kernel", "wgrad")):
        if variant.startswith(prefix):
            return fam
    assert variant.startswith("conv5_kernel"), variant
    return "conv5_splitk" if "+splitk" in variant else "conv5"


def test_tables_are_well_formed():
    ids = [c["id"] for c in CC.CONV_CASES + CC.WGRAD_CASES]
    assert len(set(ids)) == len(ids)
    for c in CC.CONV_CASES + CC.WGRAD_CASES:
        N, H, W = c["shape"]
        assert N * H * W <= CC.MAX_PIXELS and CC.cin(c) <= CC.MAX_CHANNELS and c["cout"] <= CC.MAX_CHANNELS, c["id"]
        assert set(c["env"]) <= set(CC.SWITCHES), c["id"]
        assert c["gate"] == CC.exact_and_elem(c), c["id"]
    # the inexact-by-construction cases (fp32 through a gate's sigmoid, the conventional up = 2·s): at most one in ten
    n = len(ids)
    assert sum(c["gate"] == "elem" for c in CC.CONV_CASES + CC.WGRAD_CASES) * 10 <= n
    assert any(c["gate"] == "elem" and c["dt"] == "fp32" and any(s["gate"] for s in c["srcs"]) for c in CC.CONV_CASES)
    assert any(c["gate"] == "elem" and any(s["up"] == "conv" for s in c["srcs"]) for c in CC.CONV_CASES)
    assert any(c["gate"] == "elem" for c in CC.WGRAD_CASES)
    # the conventional up-sampling runs in fp32 only: a 16-bit kernel rounds the blended value to its operand type,
    # and a value the reference rounds the other way is an operand error no output tolerance of check_elem covers
    assert all(c["dt"] == "fp32" for c in CC.CONV_CASES + CC.WGRAD_CASES if any(s["up"] == "conv" for s in c["srcs"]))


def test_every_case_routes_to_its_variant(lib, monkeypatch):
    L, so = lib
    bad = []
    for wg, cases in ((False, CC.CONV_CASES), (True, CC.WGRAD_CASES)):
        for c in cases:
            CC.set_env(c, monkeypatch)
            d = CC.wgrad_desc(L, c) if wg else CC.conv_desc(L, c)
            got = CC.variant_of(so, d, wg)
            if got != c["variant"]:
                bad.append((c["id"], c["variant"], got))
            if not wg and c["act_out"]:
                assert so.unet_conv_act_out_ok(d), c["id"]
            if not wg and "+splitk" in c["variant"]:
                assert c["ws"] and so.unet_conv_workspace(d) > 0, c["id"]
    assert not bad, f"{len(bad)} cases route elsewhere; first: {bad[:5]}"


def test_every_route_variant_is_covered_or_listed():
    names = json.loads((GOLDEN / "routes.json").read_text())["variants"]
    covered = {c["variant"] for c in CC.CONV_CASES + CC.WGRAD_CASES}
    missing = [n for n in names if n not in covered and n not in CC.UNREACHED]
    assert not missing, missing
    assert all(isinstance(r, str) and len(r) > 10 for r in CC.UNREACHED.values())
    assert not set(CC.UNREACHED) & covered, "a listed variant is reached after all: drop it from UNREACHED"
    assert set(CC.UNREACHED) <= set(names)


def _units(a, u):
    return RO.exact_units(a, u)


def test_every_case_meets_the_exactness_condition():
    """Σ|terms| / unit of every output element and every exactly-gated sum is below 2^24, from the fp64 reference's
    absolute-term sums alone; the recorded gate of each stats / bnb sum is the one this computes; every reference
    value is on its unit's grid"""
    worst = 0.0
    for c in CC.CONV_CASES:
        r = CC.conv_reference(c, CC.conv_operands(c))
        if c["gate"] == "exact":
            for name, (ref, a, u, dt) in r.outs.items():
                n = _units(a, u)
                worst = max(worst, n)
                assert n < RO.EXACT_CAP, (c["id"], name, n)
                assert torch.equal((ref / u).round() * u, ref), (c["id"], name, "off the grid")
        gates = []
        for name in ("stats", "bnb"):
            if name in r.sums:
                ref, a, units = r.sums[name]
                for i in range(2):
                    exact = c["gate"] == "exact" and _units(a[i], units[i]) < RO.EXACT_CAP
                    gates.append("eq" if exact else "tol")
        assert tuple(gates) == tuple(c["sums"]), (c["id"], gates, c["sums"])
    for c in CC.WGRAD_CASES:
        ref, a, u, dt = CC.wgrad_reference(c, CC.wgrad_operands(c)).outs["dw"]
        if c["gate"] == "exact":
            n = _units(a, u)
            worst = max(worst, n)
            assert n < RO.EXACT_CAP, (c["id"], n)
            assert torch.equal((ref / u).round() * u, ref), (c["id"], "off the grid")
    assert worst < 2 ** 22, math.log2(worst)   # the grids leave a factor of four


def test_operands_hold_the_edges():
    """negative BN scales, exact zeros at the ReLU, both gate values, 2x2 ties and all-zero pooled windows"""
    c = next(c for c in CC.CONV_CASES if c["srcs"][0]["kind"] == "act" and c["srcs"][0]["gate"] and c["dt"] == "bf16")
    t = CC.conv_operands(c).srcs[0]
    assert (t.scale < 0).any() and (t.scale == 2).any()
    pre = t.x.double() * t.scale.double() + t.shift.double()
    assert (pre == 0).any() and (pre < 0).any() and (pre > 0).any()
    assert set(t.gate_p.unique().tolist()) == {0.0, 1.0}
    q = t.gate_p.double() * CC.GATE_AB[0] + CC.GATE_AB[1]
    assert set(q.unique().tolist()) == {0.0, 40.0} and float(torch.sigmoid(torch.tensor(40.0))) == 1.0
    c = next(c for c in CC.CONV_CASES if c["out"] == "pool_bwd" and not c["pool_code"] and c["shape"][1] > 8)
    o = CC.conv_operands(c)
    N, H, W = c["shape"]
    m = RO.maxpool_act(o.pool.x, o.pool.scale, o.pool.shift, 1, H, W)
    ties = (m.win == m.out.unsqueeze(3)).sum(3)
    assert (ties >= 2).any() and ((m.out == 0) & (ties == 4)).any() and (m.code > 0).any()
    c = next(c for c in CC.CONV_CASES if c["srcs"][0]["kind"] == "up_act" and c["srcs"][0]["up"] == "half")
    g = CC.src_geom(c["srcs"][0], *c["shape"][1:])
    assert g.sh == 0.5 and g.sw == 0.5 and g.up_h == 2 * g.H - 1 and g.up_w == 2 * g.W - 1


_MISSING = []


def _has(cases, pred, what):
    if not any(pred(c) for c in cases):
        _MISSING.append(what)


def test_tables_cover_what_each_family_serves():
    by = defaultdict(list)
    for c in CC.CONV_CASES + CC.WGRAD_CASES:
        by[family(c["variant"])].append(c)
    _MISSING.clear()
    conv_fams = ("smallcin", "pw", "generic", "conv5w", "conv5", "conv5_splitk", "conv3", "conv2")
    for fam in conv_fams + ("wgrad5", "wgrad2", "wgrad"):
        cs = by[fam]
        assert len(cs) >= 8, (fam, len(cs))
        _has(cs, lambda c: c["shape"][0] == 1, (fam, "N = 1"))
        _has(cs, lambda c: c["shape"][0] >= 3, (fam, "N >= 3"))
        if fam == "pw":   # tiles of 32 or 64 consecutive pixels, whatever the map's shape
            _has(cs, lambda c: (c["shape"][0] * c["shape"][1] * c["shape"][2]) % 64 not in (0, 32), (fam, "a partial pixel tile"))
            continue
        # partial tiles: one more and one less than the tile in both directions
        _has(cs, lambda c: c["shape"][1] % 8 == 1 and c["shape"][2] % 16 == 1, (fam, "H, W one more than a tile"))
        _has(cs, lambda c: c["shape"][1] % 8 == 7 or c["shape"][2] % 16 == 15, (fam, "one less than a tile"))
    for fam in ("generic", "conv2", "conv3", "conv5_splitk", "smallcin", "wgrad", "wgrad2", "wgrad5"):
        _has(by[fam], lambda c: c["shape"][1] < 8 and c["shape"][2] < 16, (fam, "a map smaller than one tile"))
    # channel tails
    for fam in ("conv2", "conv3", "conv5", "wgrad2", "wgrad"):
        _has(by[fam], lambda c: CC.cin(c) in (40, 48, 72, 96), (fam, "Cin tail"))
        _has(by[fam], lambda c: c["cout"] in (40, 48, 96, 192), (fam, "Cout tail"))
    for b in (16, 32, 48):
        _has(CC.CONV_CASES, lambda c: len(c["srcs"]) == 2 and c["srcs"][0]["C"] == b, ("concat boundary", b))
    # epilogues
    y_modes = [lambda c: c["out"] == "y" and c["stats"], lambda c: c["out"] == "y" and c["bnb"]]
    f_modes = [lambda c: c["out"] == "f32" and c["split"] in (None, c["cout"]),
               lambda c: c["out"] == "f32" and c["split"] not in (None, c["cout"])]
    for fam in ("generic", "conv2", "conv3", "conv5", "conv5_splitk", "pw", "conv5w"):
        for i, m in enumerate(y_modes + f_modes):
            _has(by[fam], m, (fam, "epilogue", i))
    for fam in ("generic", "conv2", "conv3", "conv5", "pw"):
        for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
            _has(by[fam] + by["conv5_splitk"] if fam == "conv5" else by[fam],
                 lambda c: c["out"] == "f32" and (c["accum"], c["accum2"]) == acc, (fam, "accum", acc))
    for fam in ("generic", "conv2", "conv3"):
        _has(by[fam], lambda c: c["out"] == "pool_bwd" and c["pool_code"], (fam, "pool_bwd by code"))
        _has(by[fam], lambda c: c["out"] == "pool_bwd" and not c["pool_code"] and c["pool_extra"] != (0, 0),
             (fam, "pool_bwd, odd pre-pool size"))
    for fam in ("generic", "conv2"):
        _has(by[fam], lambda c: c["out"] == "shuffle2" and c["bias"], (fam, "shuffle2 + bias"))
        _has(by[fam], lambda c: c["out"] == "shuffle2" and not c["bias"], (fam, "shuffle2"))
    for acc in (0, 1):
        _has(by["pw"], lambda c: c["out"] == "f32_gated" and c["accum"] == acc, ("f32_gated", acc))
    for fam in ("conv5", "conv5w"):
        _has(by[fam], lambda c: c["act_out"], (fam, "act_out"))
    # bnb: reduced in the epilogue (conv5 forms, conv3's 16-channel wave tiles) and by the separate reduction
    _has(by["conv3"], lambda c: c["bnb"] and c["cout"] <= 32, "conv3 bnb in the epilogue")
    _has(by["conv3"], lambda c: c["bnb"] and c["cout"] > 32, "conv3 bnb, separate reduction")
    # source kinds, gate on and off, one and two sources
    kinds = lambda c: {(s["kind"], s["gate"]) for s in c["srcs"]}
    for fam, want in (("generic", [("plain", 0), ("act", 0), ("act", 1), ("pool_act", 0), ("up_act", 0), ("up_plain", 0),
                                   ("nchw", 0)]),
                      ("conv2", [("plain", 0), ("act", 0), ("act", 1), ("pool_act", 0), ("up_act", 0), ("up_plain", 0)]),
                      ("conv3", [("plain", 0), ("act", 0), ("act", 1), ("pool_act", 0), ("up_act", 0), ("up_plain", 0)]),
                      ("conv5", [("plain", 0), ("act", 0), ("act", 1)]), ("conv5_splitk", [("plain", 0), ("act", 0), ("act", 1)]),
                      ("conv5w", [("plain", 0), ("act", 0), ("act", 1)]), ("pw", [("plain", 0), ("act", 0), ("act", 1)]),
                      ("smallcin", [("nchw", 0)]), ("wgrad5", [("plain", 0), ("act", 0), ("act", 1)]),
                      ("wgrad2", [("plain", 0), ("act", 0), ("act", 1), ("pool_act", 0), ("up_act", 0), ("up_plain", 0)]),
                      ("wgrad", [("plain", 0), ("act", 0), ("act", 1), ("pool_act", 0), ("up_act", 0), ("up_plain", 0),
                                 ("nchw", 0)])):
        for kg in want:
            _has(by[fam], lambda c: kg in kinds(c), (fam, "source", kg))
    for fam in ("generic", "conv2", "conv3", "conv5", "conv5_splitk", "conv5w", "wgrad5", "wgrad2", "wgrad"):
        _has(by[fam], lambda c: len(c["srcs"]) == 2, (fam, "two sources"))
    # weight gradients: both kernel sizes, stored and accumulated (the split counts: test_wgrad_split_plans)
    assert {(c["k"], c["accum"]) for c in CC.WGRAD_CASES} == {(1, 0), (1, 1), (3, 0), (3, 1)}
    # every dtype in every family that has it
    for fam in conv_fams + ("wgrad2", "wgrad5", "wgrad"):
        want = {"bf16", "fp16"} if fam in ("pw", "conv5w", "conv5", "conv5_splitk", "conv3", "wgrad2", "wgrad5") else \
            {"bf16", "fp16", "fp32"}
        assert want <= {c["dt"] for c in by[fam]}, fam
    assert Counter(c["out"] for c in CC.CONV_CASES)["y"] > 100
    assert not _MISSING, _MISSING


def test_persistent_loops_are_entered():
    """conv5 and conv5w run a fixed number of workgroups over the tiles: cases with two or more rounds and with a
    ragged last round (tile and workgroup counts as the launchers in conv5.hip and conv5w.hip compute them); the
    loops of wgrad5 and wgrad2 over the tiles of a split are in test_wgrad_split_plans.  pw's
    512-block cap is not reached below the pixel budget (at most 2048 wave tiles on 4 x 512 waves), so its waves
    never loop here; its cases end in a partly filled last block instead."""
    cdiv = lambda a, b: -(-a // b)

    def conv5_rounds(c):
        N, H, W = c["shape"]
        mi = int(c["variant"].split(",")[1].rstrip(">"))
        tiles, gy = N * cdiv(H, 4 * mi) * cdiv(W, 32), cdiv(c["cout"], 64)
        return tiles / min(cdiv(256, gy), tiles)

    def conv5w_rounds(c):
        N, H, W = c["shape"]
        mi = 4 if c["variant"].endswith(",4>") else 8
        tiles, gy = N * cdiv(H, 2 * mi) * cdiv(W, 32), c["cout"] // 128
        return tiles / min(cdiv(256, gy), tiles)

    def pw_fill(c):
        N, H, W = c["shape"]
        tiles = cdiv(N * H * W, 16 * (2 if c["cout"] % 64 == 0 else 4))
        return tiles / (4 * min(cdiv(tiles, 4), 512))

    for fam, rounds in (("conv5", conv5_rounds), ("conv5w", conv5w_rounds)):
        r = [rounds(c) for c in CC.CONV_CASES if family(c["variant"]) == fam]
        assert any(x > 1 and x != int(x) for x in r), (fam, "no ragged last round", sorted(set(r)))
        assert any(x >= 2 for x in r), (fam, "no second round", sorted(set(r)))
    r = [pw_fill(c) for c in CC.CONV_CASES if family(c["variant"]) == "pw"]
    assert max(r) == 1.0 and min(r) < 1.0, sorted(set(r))


def _cdiv(a, b):
    return -(-a // b)


def wgrad_split_plan(c):
    """(pixel tiles, tiles per split, splits, workspace bytes) of a weight-gradient case, by the arithmetic of
    wgrad5_plan (wgrad5.hip), wgrad2_plan (wgrad2.hip) and wg_plan (wgrad.hip)"""
    (N, H, W), Cin, Cout, k = c["shape"], CC.cin(c), c["cout"], c["k"]
    fam = family(c["variant"])
    slab = Cout * Cin * k * k * 4
    if fam == "wgrad5":   # 64 x 64 channel blocks, 4-row x 32-column stages; the split count a multiple of 8 above 8
        mtiles, tiles_out = N * _cdiv(W, 32) * _cdiv(H, 4), (Cout // 64) * (Cin // 64)
        s = _cdiv(256, tiles_out)
        if s > 8:
            s = _cdiv(s, 8) * 8
        s = max(1, min(s, (160 << 20) // slab, mtiles))
    elif fam == "wgrad2":
        raw4 = any(x["kind"] in ("pool_act", "up_act") for x in c["srcs"])
        if Cout <= 64 and k == 3 and not raw4:
            bco, bci = 64, 64
        elif Cout <= 64:
            bco, bci = 64, 64
        elif k == 3 and not raw4:
            bco, bci = 128, 32
        elif Cin >= 64:
            bco, bci = 128, 64
        else:
            bco, bci = 128, 32
        mtiles, tiles_out = N * _cdiv(W, 16) * _cdiv(H, 8), _cdiv(Cout, bco) * _cdiv(Cin, bci)
        s = max(1, min(_cdiv(256, tiles_out), (160 << 20) // slab, mtiles))
    else:
        assert fam == "wgrad", fam
        kc = 16 if c["dt"] == "fp32" else 32
        mtiles, tiles = N * _cdiv(W, 16) * _cdiv(H, 8), _cdiv(Cin, 2 * kc) * _cdiv(Cout, 64)
        s = max(1, min(_cdiv(1024, tiles), max((160 << 20) // slab, 1), mtiles))
    per = _cdiv(mtiles, s)
    splits = _cdiv(mtiles, per)
    ws = slab * (splits + (32 if fam != "wgrad" and splits > 32 else 0))
    return mtiles, per, splits, ws


def test_wgrad_split_plans(lib, monkeypatch):
    """The split-K kernels give each workgroup `per_split` pixel tiles; the last split is short where the tiles do
    not divide.  From the plans' own arithmetic (proved against unet_wgrad_workspace, which is a function of the
    split count): wgrad5 and wgrad2 each have a case that loops (per_split >= 2) with a ragged last split, wgrad5
    on its default route has last blocks shorter than its 6-stage minimum and shorter than its 3-stage prologue,
    and each of wgrad5, wgrad2 and the generic kernel has a case with more than 32 slabs."""
    L, so = lib
    plans = defaultdict(list)
    for c in CC.WGRAD_CASES:
        fam = family(c["variant"])
        if fam not in ("wgrad5", "wgrad2", "wgrad"):
            continue
        mtiles, per, splits, ws = wgrad_split_plan(c)
        CC.set_env(c, monkeypatch)
        assert so.unet_wgrad_workspace(CC.wgrad_desc(L, c)) == ws, (c["id"], mtiles, per, splits, ws)
        plans[fam].append((c, mtiles, per, splits))
    for fam in ("wgrad5", "wgrad2"):
        ragged = [(c["id"], per, mt % per) for c, mt, per, sp in plans[fam] if per >= 2 and mt % per]
        assert ragged, (fam, "no case with per_split >= 2 and a ragged last split")
        assert any(per >= 3 for _, per, _ in ragged) and any(per >= 2 and not mt % per for c, mt, per, sp in plans[fam])
    last = {mt % per for c, mt, per, sp in plans["wgrad5"] if not c["env"] and mt % per}
    assert any(r < 3 for r in last) and any(3 <= r < 6 for r in last), last
    for fam in ("wgrad5", "wgrad2", "wgrad"):
        assert any(sp > 32 for c, mt, per, sp in plans[fam]), (fam, "no case with more than 32 split-K slabs")
