"""GPU: FusedClipAdamW and ModelEMA (csrc/optim.hip) against the update formulas evaluated in fp64 from the same fp32
inputs, with torch's own fp32 clip_grad_norm_ + AdamW (and mul_/add_ EMA) on the same device as the yardstick:
every element of ours is within 2 x the yardstick's largest error + 1 fp32 ulp of the fp64 value (two correct fp32
evaluations differ by an ulp or so per operation: fma contraction, the order of the norm's sum)."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 8192
SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7]
GROUPS = [dict(lr=1e-3, weight_decay=0.0), dict(lr=3e-3, weight_decay=0.1)]   # params [:5] and [5:]
B1, B2, EPS = 0.9, 0.999, 1e-8


def adamw_fp64(p, g, m, v, t, lr, wd, coef):
    g = g * coef
    p = p * (1 - lr * wd)
    m = m + (1 - B1) * (g - m)
    v = B2 * v + (1 - B2) * g * g
    return p - lr / (1 - B1 ** t) * m / (v.sqrt() / math.sqrt(1 - B2 ** t) + EPS), m, v


def clip_fp64(grads, clip):
    norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads))
    return norm, (min(1.0, clip / (norm + 1e-6)) if clip else 1.0)


def within_bound(ours, yard, ref, what):
    """|ours - ref| <= 2 max|yard - ref| + ulp_fp32(ref), element by element; prints the two errors"""
    ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref.float())[1] - 24)
    eo, ey = (ours.double() - ref).abs(), float((yard.double() - ref).abs().max())
    print(f"{what}: max err ours {float(eo.max()):.3e}, torch {ey:.3e}, ratio {float(eo.max()) / max(ey, 1e-300):.2f}")
    return bool((eo <= 2 * ey + ulp).all())


def param_set(gen, dtype=torch.float32):
    """flat tensors of SIZES, a view at a 4-byte storage offset, one that loses its gradient, one frozen"""
    data = [torch.randn(n, generator=gen) for n in SIZES + [1001, 7, 9]]
    ps = [torch.nn.Parameter(d.to(DEV, dtype)) for d in data[:len(SIZES)]]
    ps.append(torch.nn.Parameter(data[-3].to(DEV, dtype)[1:]))
    ps.append(torch.nn.Parameter(data[-2].to(DEV, dtype)))
    ps.append(torch.nn.Parameter(data[-1].to(DEV, dtype), requires_grad=False))
    return ps


def groups_of(ps):
    return [dict(params=ps[:5], **GROUPS[0]), dict(params=ps[5:], **GROUPS[1])]


def run_steps(kind, scale, clip, steps):
    """`steps` steps of one implementation on seeded inputs -> (params, state, last norm, snapshot after step 1).
    ps[-2] has a gradient on the first of several steps only; ps[-1] is frozen."""
    from unet.utils.optim import FusedClipAdamW
    gen = torch.Generator().manual_seed(7)
    dtype = torch.float64 if kind == "fp64" else torch.float32
    ps = param_set(gen, dtype)
    if kind == "ours":
        opt = FusedClipAdamW(groups_of(ps), max_grad_norm=clip)
    elif kind == "torch":
        opt = torch.optim.AdamW(groups_of(ps))
    state = {} if kind == "fp64" else opt.state
    norm = snap = None
    for k in range(steps):
        for p in ps[:-1]:
            g = (scale * torch.randn(p.numel(), generator=gen)).to(DEV, dtype)
            p.grad = None if (p is ps[-2] and (k > 0 or steps == 1)) else g
        if kind == "ours":
            opt.step()
            norm = None if opt.last_grad_norm is None else opt.last_grad_norm.clone()
        elif kind == "torch":
            if clip:
                norm = torch.nn.utils.clip_grad_norm_(ps, clip)
            opt.step()
        else:
            norm, coef = clip_fp64([p.grad for p in ps if p.grad is not None], clip)
            for i, p in enumerate(ps):
                if p.grad is not None:
                    st = state.setdefault(p, dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)))
                    st["step"] += 1
                    h = GROUPS[0 if i < 5 else 1]
                    new = adamw_fp64(p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"], h["lr"],
                                     h["weight_decay"], coef)
                    p.data, st["exp_avg"], st["exp_avg_sq"] = new
        if k == 0:
            snap = [t.detach().clone() for t in (ps[-2], ps[-1], *[v for v in state.get(ps[-2], {}).values()
                                                                   if isinstance(v, torch.Tensor)])]
    return ps, state, norm, snap


def cat(ps, state, key=None):
    return torch.cat([(p.detach() if key is None else state[p][key]).reshape(-1) for p in ps if key is None or p in state
                      and len(state[p])])


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("clip", [1.0, None])
@pytest.mark.parametrize("scale", [1e-3, 4.88e-3, 1.0, 30.0])   # total norm 0.2, 1.000 (the clip's edge), 205, 6100
def test_step_against_fp64(scale, clip, steps):
    ours, torch_, ref = (run_steps(k, scale, clip, steps) for k in ("ours", "torch", "fp64"))
    for key in (None, "exp_avg", "exp_avg_sq"):
        assert within_bound(cat(ours[0], ours[1], key), cat(torch_[0], torch_[1], key), cat(ref[0], ref[1], key),
                            f"scale {scale} clip {clip} steps {steps} {key or 'p'}")
    if clip:
        assert within_bound(ours[2].reshape(1), torch_[2].reshape(1), torch.tensor([ref[2]], device=DEV,
                                                                                   dtype=torch.float64), "grad norm")
    else:
        assert ours[2] is None
    # step counts: one per step with a gradient; the parameter without one keeps its count, the frozen one has none
    ps, state, _, snap = ours
    assert all(float(state[p]["step"]) == steps for p in ps[:-2])
    now = [ps[-2], ps[-1], *[v for v in state.get(ps[-2], {}).values() if isinstance(v, torch.Tensor)]]
    assert len(now) == len(snap) == (2 if steps == 1 else 5) and all(torch.equal(a, b) for a, b in zip(now, snap))
    assert float(state[ps[-2]]["step"]) == 1 if steps > 1 else not state.get(ps[-2])
    assert not state.get(ps[-1])
    # a second fresh optimizer on the same inputs: the same bits
    again = run_steps("ours", scale, clip, steps)
    for key in (None, "exp_avg", "exp_avg_sq"):
        assert torch.equal(cat(ours[0], ours[1], key), cat(again[0], again[1], key))
    assert clip is None or torch.equal(ours[2], again[2])


def test_gradscaler_contract():
    """grad_scale / found_inf as GradScaler.step sets them, consumed on the device; no call of step() synchronises"""
    from unet.utils.optim import FusedClipAdamW

    def fresh(mult):
        gen = torch.Generator().manual_seed(11)
        ps = param_set(gen)[:-2]
        grads = [(0.01 * torch.randn(p.numel(), generator=gen) * mult).to(DEV) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps, FusedClipAdamW(groups_of(ps), max_grad_norm=1.0)

    def bits(ps, opt):
        return [t.clone() for p in ps for t in (p.detach(), *opt.state[p].values())]

    def step(opt):
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")

    one, zero = torch.ones((), device=DEV), torch.zeros((), device=DEV)
    ps, opt = fresh(1.0)
    step(opt)
    plain, plain_norm = bits(ps, opt), opt.last_grad_norm.clone()
    ps, opt = fresh(1024.0)
    opt.grad_scale, opt.found_inf = one * 1024.0, zero
    step(opt)
    scaled = bits(ps, opt)
    assert len(scaled) == 4 * len(ps) and all(torch.equal(a, b) for a, b in zip(plain, scaled))
    assert torch.equal(plain_norm, opt.last_grad_norm)
    ps[5].grad[17] = float("inf")            # an overflowed gradient: the device-side check skips the step
    step(opt)
    assert all(torch.equal(a, b) for a, b in zip(scaled, bits(ps, opt)))
    ps[5].grad[17] = 0.0
    opt.found_inf = one                      # the scaler's own flag (another optimizer's, or unscale_'s)
    step(opt)
    assert all(torch.equal(a, b) for a, b in zip(scaled, bits(ps, opt)))
    opt.found_inf = zero
    step(opt)
    assert not torch.equal(scaled[0], ps[0].detach()) and float(opt.state[ps[0]]["step"]) == 2


def test_state_interchange_with_torch_adamw():
    from unet.utils.optim import FusedClipAdamW
    gen = torch.Generator().manual_seed(5)
    ps = param_set(gen)[:-2]
    topt = torch.optim.AdamW(groups_of(ps), capturable=True)
    for k in range(3):
        for p in ps:
            p.grad = torch.randn(p.numel(), generator=gen).to(DEV)
        if k < 2:
            topt.step()
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    for q, p in zip(mine, ps):
        q.grad = p.grad.clone()
    opt = FusedClipAdamW(groups_of(mine), max_grad_norm=1.0)
    opt.load_state_dict(copy.deepcopy(topt.state_dict()))
    norm, coef = clip_fp64([p.grad for p in ps], 1.0)
    ref = [adamw_fp64(p.detach().double(), p.grad.double(), topt.state[p]["exp_avg"].double(),
                      topt.state[p]["exp_avg_sq"].double(), 3, GROUPS[0 if i < 5 else 1]["lr"],
                      GROUPS[0 if i < 5 else 1]["weight_decay"], coef) for i, p in enumerate(ps)]
    torch.nn.utils.clip_grad_norm_(ps, 1.0)
    topt.step()
    opt.step()
    for j, key in enumerate((None, "exp_avg", "exp_avg_sq")):
        assert within_bound(cat(mine, opt.state, key), cat(ps, topt.state, key),
                            torch.cat([r[j].reshape(-1) for r in ref]), f"third step {key or 'p'}")
    assert all(float(opt.state[q]["step"]) == 3 for q in mine)
    back = torch.optim.AdamW(groups_of(ps), capturable=True)
    back.load_state_dict(copy.deepcopy(opt.state_dict()))
    back.step()
    assert float(back.state[ps[0]]["step"]) == 4


def test_ema_against_fp64():
    from unet.models import AttentionUNet
    from unet.utils.general import ModelEMA
    torch.manual_seed(0)
    model = AttentionUNet(1, 2, base_features=4, deep_supervision=True).to(DEV)
    ema = ModelEMA(model, decay=0.999, warmup_steps=2)
    assert not ema.ema_model.training and not any(p.requires_grad for p in ema.ema_model.parameters())
    names = [k for k, _ in model.named_parameters()]
    ref = [p.detach().double() for p in model.parameters()]
    yard = [p.detach().clone() for p in model.parameters()]
    gen = torch.Generator(device=DEV).manual_seed(3)
    for u in range(1, 5):
        if u == 4:   # what the reference script does at the warm-up boundary: copies in place, pointers survive
            ema.ema_model.load_state_dict(model.state_dict())
            ref = [p.detach().double() for p in model.parameters()]
            yard = [p.detach().clone() for p in model.parameters()]
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                t.add_(1 if t.dtype == torch.int64 else 0.1 * torch.randn(t.shape, generator=gen, device=DEV))
        ema.update(model)
        d = min(0.999, (1 + u) / (10 + u)) if u <= 2 else 0.999
        for i, p in enumerate(model.parameters()):
            ref[i] = d * ref[i] + (1 - d) * p.detach().double()
            yard[i].mul_(d).add_(p.detach(), alpha=1 - d)
        if u >= 3:
            got = dict(ema.ema_model.named_parameters())
            assert within_bound(torch.cat([got[k].reshape(-1) for k in names]), torch.cat([y.reshape(-1) for y in yard]),
                                torch.cat([r.reshape(-1) for r in ref]), f"EMA after update {u}")
            ebuf = dict(ema.ema_model.named_buffers())
            for k, b in model.named_buffers():
                assert ebuf[k].dtype == b.dtype and torch.equal(ebuf[k], b), k
    assert ema.updates == 4 and set(ema.state_dict()) == {"ema_state_dict", "decay", "updates"}
    assert any(b.dtype == torch.int64 for b in model.buffers()) and any(p.numel() == 1 for p in model.parameters())


def test_reference_loop_with_fused_tail():
    """train_one_epoch of scripts/train.py:103-161 with its EMA hook (the tqdm bar aside), once with torch's clip +
    AdamW + the formula EMA and once with FusedClipAdamW + ModelEMA; bounds of tests/test_gpu_train_loop.py."""
    from unet.models import AttentionUNet
    from unet.utils.general import ModelEMA
    from unet.utils.loss import DiceBCELoss
    from unet.utils.optim import FusedClipAdamW
    lr, wd, clip, accum, n, decay = 5e-5, 1e-4, 1.0, 2, 5, 0.999
    batches = []
    for i in range(n):
        g = torch.Generator().manual_seed(900 + i)
        x = torch.rand(2, 1, 64, 64, generator=g) * 2 - 1
        t = torch.zeros(2, 64, 64, dtype=torch.int64)
        t[0, 10 + i:30, 12:40] = 1
        t[1, 30:52, 8 + 3 * i:30 + 3 * i] = 1
        batches.append((x.to(DEV), t.to(DEV)))

    def epoch(fused):
        torch.manual_seed(0)
        model = AttentionUNet(1, 2, base_features=8).to(DEV).train()
        model.hip_precision = "fp32"
        criterion = DiceBCELoss()
        if fused:
            opt, ema = FusedClipAdamW(model.parameters(), lr=lr, weight_decay=wd, max_grad_norm=clip), ModelEMA(model, decay)
            avg = ema.ema_model
        else:
            opt, avg = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd), copy.deepcopy(model)

        def tail():
            if not fused:
                torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            opt.step()
            opt.zero_grad()
            if fused:
                ema.update(model)
            else:
                with torch.no_grad():
                    for e, p in zip(avg.parameters(), model.parameters()):
                        e.mul_(decay).add_(p, alpha=1 - decay)
        losses = []
        opt.zero_grad()
        for i, (images, masks) in enumerate(batches):
            loss = criterion(model(images), masks) / accum
            loss.backward()
            if (i + 1) % accum == 0:
                tail()
            losses.append(loss.item() * accum)
        if len(batches) % accum != 0:
            tail()
        return losses, [p.detach() for p in model.parameters()], [p.detach() for p in avg.parameters()]

    (l_t, p_t, e_t), (l_f, p_f, e_f) = epoch(False), epoch(True)
    steps = math.ceil(n / accum)
    for a, b in zip(l_f, l_t):
        assert abs(a - b) <= 2e-5 * abs(b) + 1e-6, (l_f, l_t)
    for what, xs, ys in (("parameters", p_f, p_t), ("EMA parameters", e_f, e_t)):
        diffs = torch.cat([(x - y).abs().reshape(-1) for x, y in zip(xs, ys)])
        tight = float((diffs <= 1e-6).float().mean())
        print(f"{what} after {steps} steps: max |d| {float(diffs.max()):.2e}, within 1e-6: {tight:.4f}")
        assert float(diffs.max()) <= 2 * lr * steps + 1e-6 and tight >= 0.99
