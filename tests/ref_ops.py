"""fp64 references of the streaming kernels around the convolutions (csrc/bn.hip, csrc/gate.hip, csrc/loss.hip and
csrc/misc.hip: OutConv, resampling, the ConvTranspose2d backward prep, max-pool, materialised sources, layouts),
written from the maths of nn.BatchNorm2d, ReLU, AttentionGate (layers.py:126-192), the Dice / balanced
cross-entropy losses (loss.py:18-229), bilinear interpolation and MaxPool2d, not from the kernels.  Pure torch; every
function takes the kernels' own operands (any dtype, any device), evaluates in float64 and returns what the matching
entry point must produce, plus the sums of absolute terms ("natural scales") that the tests gate the fp32 sums against.

Layouts: activations [P, C] (NHWC flattened over pixels) or [N, H, W, C], per-channel vectors [C], affine pairs
[2, C] (scale, shift), coefficient triples [3, C] (A, B, Cc), OutConv logits [N, K, H, W], loss logits [N, K, HW].
tests/test_ref_ops_cpu.py proves the formulas against torch autograd, nn.functional and the oracle's losses."""

from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F


def d(t):
    return None if t is None else t.double()


# ---- BatchNorm2d ------------------------------------------------------------------------------------

def bn_finalize(stats, count, gamma, beta, running_mean=None, running_var=None, nbt=None, momentum=0.1, eps=1e-5):
    """stats [2][C][rows] partial (Σx, Σx²) -> batch statistics, the affine and the running-statistics update.
    Biased variance (clamped at 0) normalises; the unbiased one goes into running_var (count == 1: biased);
    momentum < 0: cumulative average 1 / (nbt + 1) (nn.BatchNorm2d(momentum=None))."""
    st = d(stats)
    s, ss = st[0].sum(-1), st[1].sum(-1)
    mean = s / count
    var = (ss / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = d(gamma) * invstd
    shift = d(beta) - mean * scale
    r = NS(mean=mean, invstd=invstd, scale=scale, shift=shift, var=var, running_mean=None, running_var=None,
           nbt=None, abs_mean=st[0].abs().sum(-1) / count)
    if running_mean is not None and running_var is not None:
        f = float(momentum)
        if momentum < 0:
            f = 1.0 / (int(nbt) + 1) if nbt is not None else 1.0
        unb = var * count / (count - 1) if count > 1 else var
        r.running_mean = (1 - f) * d(running_mean) + f * mean
        r.running_var = (1 - f) * d(running_var) + f * unb
        r.abs_running_mean = abs(1 - f) * d(running_mean).abs() + abs(f) * mean.abs()
    if nbt is not None:
        r.nbt = int(nbt) + 1
    return r


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5):
    invstd = 1.0 / torch.sqrt(d(running_var) + eps)
    scale = d(gamma) * invstd
    return NS(scale=scale, shift=d(beta) - d(running_mean) * scale, mean=d(running_mean), invstd=invstd)


def act(y, scale, shift, relu):
    """relu?(y * scale + shift); scale / shift None: identity affine"""
    a = d(y)
    if scale is not None:
        a = a * d(scale)
    if shift is not None:
        a = a + d(shift)
    return a.clamp_min(0) if relu else a


def bn_bwd_sums(da, y, scale, shift, relu, mean, invstd):
    """g = da where the ReLU passed (y * scale + shift > 0), else 0; Σg, Σg·x̂ and Σ|g|, Σ|g·x̂| per channel"""
    g, yv = d(da), d(y)
    if relu:
        g = torch.where(yv * d(scale) + d(shift) > 0, g, torch.zeros_like(g))
    gx = g * (yv - d(mean)) * d(invstd)
    return NS(g=g, sum_g=g.sum(0), sum_gx=gx.sum(0), abs_g=g.abs().sum(0), abs_gx=gx.abs().sum(0))


def bn_bwd_coef(sum_g, sum_gx, count, gamma, mean, invstd):
    """dγ = Σg·x̂, dβ = Σg and dy = A·g + B·y + Cc: A = γ·invstd, B = −A·invstd·Σgx̂/M, Cc = −A·Σg/M − B·mean
    (count == 0, eval mode: the statistics are constants, (γ·invstd, 0, 0)).  abs_cc: Cc's largest term."""
    sg, sgx = d(sum_g), d(sum_gx)
    A = d(gamma) * d(invstd)
    if count > 0:
        B = -A * d(invstd) * sgx / count
        t1, t2 = -A * sg / count, -B * d(mean)
        Cc = t1 + t2
        abs_cc = torch.maximum(t1.abs(), t2.abs())
    else:
        B, Cc, abs_cc = torch.zeros_like(A), torch.zeros_like(A), torch.zeros_like(A)
    return NS(coef=torch.stack([A, B, Cc]), dgamma=sgx, dbeta=sg, abs_cc=abs_cc)


def bn_bwd_apply(g, y, coef):
    """dy = A·g + B·y + Cc and the sum of the absolute terms"""
    c, g, yv = d(coef), d(g), d(y)
    t0, t1 = c[0] * g, c[1] * yv
    return NS(dy=t0 + t1 + c[2], abs_terms=t0.abs() + t1.abs() + c[2].abs())


# ---- AttentionGate ----------------------------------------------------------------------------------

def gate_act(gw, xw, gab, xab):
    """a = relu(BN_g(gw) + BN_x(xw)) with the BNs given as affine pairs"""
    gab, xab = d(gab), d(xab)
    return (d(gw) * gab[0] + gab[1] + d(xw) * xab[0] + xab[1]).clamp_min(0)


def gate_psi(gw, xw, gab, xab, wpsi):
    a = gate_act(gw, xw, gab, xab)
    t = a * d(wpsi)
    p = t.sum(-1)
    return NS(a=a, p=p, abs_p=t.abs().sum(-1), sum_p=p.sum(), sum_pp=(p * p).sum(), abs_sum_p=p.abs().sum())


def gate_bwd1(dxs, yx, sx, bx, relu, p, psi_ab, psi_mean, psi_invstd, dx_old=None):
    """out = x·s, s = sigmoid(q), q = p·pa + pb.  dx (+)= d·s; dq = (Σ_c d·x)·s·(1−s); Σdq, Σdq·p̂"""
    dv, p, ab = d(dxs), d(p), d(psi_ab).reshape(-1)
    x = act(yx, sx, bx, relu)
    s = torch.sigmoid(p * ab[0] + ab[1])
    t = dv * x
    ds = t.sum(-1)
    ss = s * (1 - s)
    dq = ds * ss
    ph = (p - d(psi_mean).reshape(())) * d(psi_invstd).reshape(())
    dx = dv * s.unsqueeze(-1)
    if dx_old is not None:
        dx = dx + d(dx_old)
    return NS(x=x, s=s, ds=ds, dq=dq, abs_dq=t.abs().sum(-1) * ss, dx=dx, sum_dq=dq.sum(), sum_dqp=(dq * ph).sum(),
              abs_sum_dq=dq.abs().sum(), abs_sum_dqp=(dq * ph).abs().sum())


def gate_bwd2(gw, xw, gab, xab, g_mean, g_invstd, x_mean, x_invstd, wpsi, dq, p, psi_coef):
    """dp = psi-BN backward of dq; dz = dp·wpsi·[a > 0]; the four [Ci] sums (Σdz, Σdz·ĝ, Σdz·x̂, Σdp·a) and
    the sums of their absolute terms"""
    a = gate_act(gw, xw, gab, xab)
    c = d(psi_coef).reshape(-1)
    dp = (c[0] * d(dq) + c[1] * d(p) + c[2]).unsqueeze(-1)
    dz = torch.where(a > 0, dp * d(wpsi), torch.zeros_like(a))
    gh = (d(gw) - d(g_mean)) * d(g_invstd)
    xh = (d(xw) - d(x_mean)) * d(x_invstd)
    terms = [dz, dz * gh, dz * xh, dp * a]
    abs_dp = ((c[0] * d(dq)).abs() + (c[1] * d(p)).abs() + c[2].abs()).unsqueeze(-1)
    abs_dz = torch.where(a > 0, abs_dp * d(wpsi).abs(), torch.zeros_like(a))
    return NS(a=a, dp=dp.squeeze(-1), dz=dz, abs_dz=abs_dz, sums=torch.stack([t.sum(0) for t in terms]),
              abs_sums=torch.stack([t.abs().sum(0) for t in terms]))


def gate_bwd3(gw, xw, gab, xab, wpsi, dq, p, psi_coef, gcoef, xcoef):
    """dgw, dxw: the two projections' BatchNorm backward of dz, and their absolute terms |A·dz| + |B·g| + |Cc|.
    wide_*: the same with dz's own terms expanded, |A·wpsi|·(|pA·dq| + |pB·p| + |pCc|) in place of |A·dz| —
    dp = pA·dq + pB·p + pCc is itself a sum, which cancels when psi_coef is a real BatchNorm backward's"""
    zero = torch.zeros(gab.shape[-1], dtype=torch.float64, device=gab.device)
    r2 = gate_bwd2(gw, xw, gab, xab, zero, zero, zero, zero, wpsi, dq, p, psi_coef)
    dz = r2.dz
    rg, rx = bn_bwd_apply(dz, gw, gcoef), bn_bwd_apply(dz, xw, xcoef)
    wide = r2.abs_dz - dz.abs()
    return NS(dgw=rg.dy, dxw=rx.dy, abs_dgw=rg.abs_terms, abs_dxw=rx.abs_terms, dz=dz,
              wide_dgw=rg.abs_terms + d(gcoef)[0].abs() * wide, wide_dxw=rx.abs_terms + d(xcoef)[0].abs() * wide)


def gate_autograd(gw, xw, x, dout, wpsi, bn_g, bn_x, bn_psi, eps=1e-5, mask=None, dtype=torch.float64):
    """The whole gate in fp64 under torch autograd, batch statistics everywhere: a = relu(BN_g(gw) + BN_x(xw)),
    p = a·wpsi, s = sigmoid(BN_psi(p)), out = x·s, loss = Σ out·dout.  bn_* = (γ, β).  mask (optional): where
    the ReLU passes, for inputs whose pre-activation is known exactly (an fp64 BatchNorm is a rounding away from
    it, which matters only where it is exactly 0).  dtype float32: the same in plain fp32 torch, for measuring what
    fp32 evaluation costs.  Returns the gradients by name."""
    leaves = {"gw": gw, "xw": xw, "x": x, "wpsi": wpsi, "g_gamma": bn_g[0], "g_beta": bn_g[1],
              "x_gamma": bn_x[0], "x_beta": bn_x[1], "psi_gamma": bn_psi[0], "psi_beta": bn_psi[1]}
    L = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
    z = (F.batch_norm(L["gw"], None, None, L["g_gamma"], L["g_beta"], True, 0.0, eps)
         + F.batch_norm(L["xw"], None, None, L["x_gamma"], L["x_beta"], True, 0.0, eps))
    a = F.relu(z) if mask is None else z * mask.to(dtype)
    p = a @ L["wpsi"]
    q = F.batch_norm(p.unsqueeze(-1), None, None, L["psi_gamma"].reshape(1), L["psi_beta"].reshape(1), True, 0.0, eps)
    out = L["x"] * torch.sigmoid(q)
    (out * dout.to(dtype)).sum().backward()
    return NS(out=out.detach(), p=p.detach(), q=q.detach().squeeze(-1), **{"d_" + k: v.grad for k, v in L.items()})


# ---- OutConv ----------------------------------------------------------------------------------------

def outconv_fwd(y, scale, shift, relu, w, b):
    """y [N,H,W,C] -> logits [N,K,H,W] = b + W·act(y); abs_terms = |b| + Σ_c |w·a|"""
    a = act(y, scale, shift, relu)
    w, b = d(w), d(b)
    out = torch.einsum("nhwc,kc->nkhw", a, w) + b.view(1, -1, 1, 1)
    return NS(logits=out, abs_terms=torch.einsum("nhwc,kc->nkhw", a.abs(), w.abs()) + b.abs().view(1, -1, 1, 1))


def outconv_bwd(y, scale, shift, relu, w, dl):
    """da [N,H,W,C] = W^T dl, dW [K,C] = Σ dl·act(y), db [K] = Σ dl"""
    a, dl = act(y, scale, shift, relu), d(dl)
    return NS(da=torch.einsum("nkhw,kc->nhwc", dl, d(w)), dw=torch.einsum("nkhw,nhwc->kc", dl, a),
              db=dl.sum((0, 2, 3)))


def outconv_bwd_bn(y, scale, shift, relu, w, dl, mean, invstd):
    """OutConv backward fused with the BatchNorm backward sums of its input: outconv_bwd + bn_bwd_sums(W^T dl)"""
    r = outconv_bwd(y, scale, shift, relu, w, dl)
    C = y.shape[-1]
    r.bn = bn_bwd_sums(r.da.reshape(-1, C), y.reshape(-1, C), scale, shift, relu, mean, invstd)
    return r


def outconv_bn_apply(y, scale, shift, relu, w, dl, coef):
    """dy = A·g_m + B·y + Cc with g = W^T dl recomputed; g is itself a sum here, so A·g's absolute term is
    |A|·Σ_k|w_k·dl_k| (the classes' contributions may cancel)"""
    C = y.shape[-1]
    g = torch.einsum("nkhw,kc->nhwc", d(dl), d(w)).reshape(-1, C)
    ag = torch.einsum("nkhw,kc->nhwc", d(dl).abs(), d(w).abs()).reshape(-1, C)
    yv = d(y).reshape(-1, C)
    if relu:
        m = yv * d(scale) + d(shift) > 0
        g, ag = torch.where(m, g, torch.zeros_like(g)), torch.where(m, ag, torch.zeros_like(g))
    r = bn_bwd_apply(g, yv, coef)
    r.narrow_terms = r.abs_terms
    r.abs_terms = r.abs_terms + d(coef)[0].abs() * (ag - g.abs())
    return r


# ---- DiceBCE / Dice / BalancedCE loss (csrc/loss.hip) -----------------------------------------------
# Fields of one image, [4 + 3K]: n0 = #[t=0], n1 = #[t=1], S0 = Σ_{t=0} ce, S1 = Σ_{t=1} ce, then per class
# (I_c = Σ p_c·[t=c], P_c = Σ p_c, T_c = #[t=c]).  A label outside [0, K) is a pixel with an all-zero one-hot row
# and cross-entropy weight 0; its softmax still counts in P_c.  Every term is >= 0, so a field is its own
# natural scale.

def loss_cfg(ce_w=1.0, dice_w=1.0, class_w=0.5, ce_smooth=1e-6, dice_smooth=1.0, ignore_bg=1, reduction=0):
    """reduction: 0 mean, 1 sum, 2 none (the Dice term per (n, c); the cross-entropy term is always a mean)"""
    return NS(ce_w=ce_w, dice_w=dice_w, class_w=class_w, ce_smooth=ce_smooth, dice_smooth=dice_smooth,
              ignore_bg=int(ignore_bg), reduction=int(reduction))


def loss_pixel_fields(z, t, dtype=torch.float64):
    """z [N, K, HW] logits, t [N, HW] integer labels -> the per-pixel terms of the fields [N, 4 + 3K, HW]
    (differentiable in z) and their absolute terms: the fields' own, except S0 / S1, whose ce = lse − z_t is a
    difference (|lse| + |z_t|).  dtype float32: the same in plain fp32 torch, for measuring what fp32 costs."""
    z = z.to(dtype)
    N, K, HW = z.shape
    valid = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1)
    oh = F.one_hot(tc, K).permute(0, 2, 1).to(dtype) * valid.unsqueeze(1).to(dtype)
    p = torch.softmax(z, 1)
    lse, zt = torch.logsumexp(z, 1), z.gather(1, tc.unsqueeze(1)).squeeze(1)
    ce, ace = (lse - zt) * valid.to(dtype), (lse.abs() + zt.abs()) * valid.to(dtype)
    m0, m1 = (t == 0).to(dtype), (t == 1).to(dtype) * float(K > 1)
    per_class = torch.stack([p * oh, p, oh], 2).reshape(N, 3 * K, HW)
    px = torch.cat([torch.stack([m0, m1, ce * m0, ce * m1], 1), per_class], 1)
    return px, torch.cat([torch.stack([m0, m1, ace * m0, ace * m1], 1), per_class], 1).detach()


def loss_fields(z, t, dtype=torch.float64):
    """fields [N, 4 + 3K]"""
    return loss_pixel_fields(z, t, dtype)[0].sum(-1)


def loss_partial(z, t, rows, dtype=torch.float64):
    """the partial table [N, rows, 4 + 3K] and its absolute terms: row r holds the fields of the pixels
    [r·per, (r+1)·per), per = ceil(HW / rows)"""
    HW = z.shape[-1]
    per = (HW + rows - 1) // rows
    out = []
    for px in loss_pixel_fields(z, t, dtype):
        px = F.pad(px, [0, rows * per - HW])
        out.append(px.reshape(px.shape[0], px.shape[1], rows, per).sum(-1).permute(0, 2, 1))
    return NS(part=out[0], abs_terms=out[1])


def _loss_split(fields, K):
    f = fields
    pc = f[:, 4:].reshape(f.shape[0], K, 3)
    return f[:, 0], f[:, 1], f[:, 2], f[:, 3], pc[..., 0], pc[..., 1], pc[..., 2]


def loss_value(fields, K, cfg):
    """the loss from the per-image fields: ce_w·mean_n((1−cw)·S0/(n0+cs) + cw·S1/(n1+cs)) + dice_w·dice, with
    D_nc = (2I + ds)/(P + T + ds) over the classes c >= c_lo: mean 1 − mean(D), sum Σ(1 − D); none: the
    [N, K − c_lo] table 1 − D alone (DiceLoss(reduction='none'); no scalar to add a cross-entropy to).
    Also the largest term (abs), for a gate where the terms cancel."""
    n0, n1, S0, S1, I, P, T = _loss_split(fields, K)
    c_lo = 1 if (cfg.ignore_bg and K > 1) else 0
    D = ((2 * I + cfg.dice_smooth) / (P + T + cfg.dice_smooth))[:, c_lo:]
    if cfg.reduction == 2:
        return NS(loss=1 - D, abs=1 + D.abs())
    ce = ((1 - cfg.class_w) * S0 / (n0 + cfg.ce_smooth) + cfg.class_w * S1 / (n1 + cfg.ce_smooth)).mean()
    dl = 1 - D.mean() if cfg.reduction == 0 else (1 - D).sum()
    return NS(loss=cfg.ce_w * ce + cfg.dice_w * dl,
              abs=abs(cfg.ce_w) * ce.abs() + abs(cfg.dice_w) * (1 + D.abs().mean() if cfg.reduction == 0 else D.numel() + D.abs().sum()))


def loss_coef(fields, K, cfg, set_w=1.0):
    """the coefficient table [N, 2 + 2K] = (w0, w1, gA[K], gB[K]) of
    dz_k = w_t·(p_k − [k=t]) + G_k·p_k − p_k·Σ_c G_c·p_c,  G_c = gA_c·[t=c] + gB_c:
    w_i = set_w·ce_w·cw_i/(n_i + cs)/N; with U = P + T + ds and r = dice_w·set_w·(1/(N·nd) for mean, else 1):
    gA = −2r/U, gB = r·(2I + ds)/U² (∂(1−D)/∂p at a pixel = −2[t=c]/U + (2I+ds)/U²); 0 for c < c_lo"""
    n0, n1, S0, S1, I, P, T = _loss_split(d(fields), K)
    N = fields.shape[0]
    c_lo = 1 if (cfg.ignore_bg and K > 1) else 0
    r = cfg.dice_w * set_w * (1.0 / (N * (K - c_lo)) if cfg.reduction == 0 else 1.0)
    U = P + T + cfg.dice_smooth
    gA, gB = -2 * r / U, r * (2 * I + cfg.dice_smooth) / (U * U)
    gA[:, :c_lo] = 0
    gB[:, :c_lo] = 0
    w0 = set_w * cfg.ce_w * (1 - cfg.class_w) / (n0 + cfg.ce_smooth) / N
    w1 = set_w * cfg.ce_w * cfg.class_w / (n1 + cfg.ce_smooth) / N
    return torch.cat([w0.unsqueeze(-1), w1.unsqueeze(-1), gA, gB], -1)


def loss_dz(z, t, cfg, gout, set_w=1.0, dtype=torch.float64):
    """dz = gout · ∂loss/∂z by torch autograd through loss_fields and loss_value.  gout: a scalar, or [N, K − c_lo]
    for reduction none, where it multiplies the Dice table (the cross-entropy term, a scalar, keeps factor 1)"""
    K = z.shape[1]
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    f = loss_fields(zz, t, dtype)
    go = torch.as_tensor(gout, dtype=dtype, device=z.device)
    if cfg.reduction == 2:
        mean = loss_cfg(cfg.ce_w, 0.0, cfg.class_w, cfg.ce_smooth, cfg.dice_smooth, cfg.ignore_bg, 0)
        total = cfg.dice_w * (loss_value(f, K, cfg).loss * go).sum() + loss_value(f, K, mean).loss
    else:
        total = loss_value(f, K, cfg).loss * go
    (set_w * total).backward()
    return zz.grad


def loss_dz_terms(z, t, coef, gout, per_elem, ignore_bg):
    """dz from a coefficient table by the formula of loss_coef, and the sum of its absolute terms"""
    z, coef = d(z), d(coef)
    N, K, HW = z.shape
    c_lo = 1 if (ignore_bg and K > 1) else 0
    valid = (t >= 0) & (t < K)
    oh = F.one_hot(t.clamp(0, K - 1), K).permute(0, 2, 1).double() * valid.unsqueeze(1)
    p = torch.softmax(z, 1)
    wt = coef[:, 0:1] * (t == 0) + coef[:, 1:2] * ((t == 1) & (K > 1))                # [N, HW]
    G = coef[:, 2:2 + K].unsqueeze(-1) * oh + coef[:, 2 + K:].unsqueeze(-1)         # [N, K, HW]
    go = torch.as_tensor(gout, dtype=torch.float64, device=z.device)
    if per_elem:
        G[:, c_lo:] = G[:, c_lo:] * go.reshape(N, K - c_lo, 1)
        go = torch.ones((), dtype=torch.float64, device=z.device)
    sgp, asgp = (G * p).sum(1, keepdim=True), (G * p).abs().sum(1, keepdim=True)
    dz = go * (wt.unsqueeze(1) * (p - oh) + G * p - p * sgp)
    terms = go.abs() * (wt.abs().unsqueeze(1) * (p + oh) + (G * p).abs() + p * asgp)
    return NS(dz=dz, abs_terms=terms)


# ---- bilinear resampling, align_corners=True (csrc/misc.hip) ----------------------------------------

def resize(x, Ho, Wo):
    """x [..., Hi, Wi] (NCHW) -> [..., Ho, Wo]"""
    return F.interpolate(d(x), size=(Ho, Wo), mode="bilinear", align_corners=True)


def resize_bwd(dy, Hi, Wi, dx_old=None):
    """the adjoint of resize at dy [NC..., Ho, Wo], by autograd"""
    dy = d(dy)
    x = torch.zeros(*dy.shape[:-2], Hi, Wi, dtype=torch.float64, device=dy.device, requires_grad=True)
    resize(x, dy.shape[-2], dy.shape[-1]).backward(dy)
    return x.grad if dx_old is None else x.grad + d(dx_old)


def lin_axis(n_in, n_out, device="cpu"):
    """the taps of one axis: i0, i1, λ per destination index, the dense weight matrix [n_out, n_in] and its support"""
    o = torch.arange(n_out, dtype=torch.float64, device=device)
    s = o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = s.floor().clamp(0, n_in - 1).long()
    i1 = (i0 + 1).clamp(max=n_in - 1)
    lam = (s - i0).clamp(0, 1)
    Wm = torch.zeros(n_out, n_in, dtype=torch.float64, device=device)
    r = torch.arange(n_out, device=device)
    Wm[r, i0] += 1 - lam
    Wm[r, i1] += lam
    Sm = torch.zeros_like(Wm)
    Sm[r, i0] = 1
    Sm[r, i1] = 1
    return NS(i0=i0, i1=i1, lam=lam, W=Wm, S=Sm)


def resize_terms(x, Ho, Wo):
    """Σ_taps w·|x| and max_taps |x| per destination element (the a-priori fp32 bound's operands)"""
    a = d(x).abs()
    ay, ax = lin_axis(x.shape[-2], Ho, x.device), lin_axis(x.shape[-1], Wo, x.device)
    c = [a[..., iy, :][..., ix] for iy in (ay.i0, ay.i1) for ix in (ax.i0, ax.i1)]
    return NS(sum_w=ay.W @ a @ ax.W.T, max_a=torch.stack(c).amax(0))


def resize_bwd_terms(dy, Hi, Wi):
    """the same summed over the destination taps of each source element: Σ w·|dy| and Σ_{taps} |dy|"""
    a = d(dy).abs()
    ay, ax = lin_axis(Hi, dy.shape[-2], dy.device), lin_axis(Wi, dy.shape[-1], dy.device)
    return NS(sum_w=ay.W.T @ a @ ax.W, sum_a=ay.S.T @ a @ ax.S)


def upsample_bwd(d_up, Hs, Ws, up_h, up_w, pad_t, pad_l, dx_old=None):
    """d_up [N, Hp, Wp, C] (NHWC): the adjoint of F.pad(resize(x, up_h, up_w)) at the padded frame -> [N, Hs, Ws, C]"""
    g = d(d_up).permute(0, 3, 1, 2)
    N, C, Hp, Wp = g.shape
    x = torch.zeros(N, C, Hs, Ws, dtype=torch.float64, device=g.device, requires_grad=True)
    u = F.pad(resize(x, up_h, up_w), [pad_l, Wp - up_w - pad_l, pad_t, Hp - up_h - pad_t])
    u.backward(g)
    r = x.grad.permute(0, 2, 3, 1)
    return r if dx_old is None else r + d(dx_old)


# ---- ConvTranspose2d(k=2, s=2) backward prep ---------------------------------------------------------

def convt_bwd_prep(d_up, h, w, pad_t, pad_l):
    """d_up [N, Hp, Wp, Ct] -> s2d [N, h, w, 4·Ct], channel (2a+b)·Ct + c = d_up[n, pad_t+2y+a, pad_l+2x+b, c]
    (a selection: exact), the bias gradient Σ over the placed region [Ct] and Σ|·|"""
    N, _, _, Ct = d_up.shape
    g = d(d_up)[:, pad_t:pad_t + 2 * h, pad_l:pad_l + 2 * w]
    s2d = g.reshape(N, h, 2, w, 2, Ct).permute(0, 1, 3, 2, 4, 5).reshape(N, h, w, 4 * Ct)
    return NS(s2d=s2d, bias=g.sum((0, 1, 2)), abs_bias=g.abs().sum((0, 1, 2)))


# ---- MaxPool2d(2) of an activation, materialised sources, layouts -----------------------------------

def pool_windows(a, H, W):
    """a [N, Hs, Ws, C] (Hs >= 2H, Ws >= 2W) -> [N, H, W, 4, C], the windows in row-major order"""
    N, _, _, C = a.shape
    return a[:, :2 * H, :2 * W].reshape(N, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4, C)


def maxpool_act(y, scale, shift, relu, H, W):
    """max over the 2x2 windows of relu?(y·scale + shift) and the argmax code 0..3: the first maximum wins, and a
    NaN replaces whatever came before it (ATen's `val > max || isnan(val)`)"""
    win = pool_windows(act(y, scale, shift, relu), H, W)
    best, code = win[..., 0, :], torch.zeros_like(win[..., 0, :], dtype=torch.uint8)
    for q in range(1, 4):
        v = win[..., q, :]
        upd = (v > best) | v.isnan()
        best, code = torch.where(upd, v, best), torch.where(upd, torch.full_like(code, q), code)
    return NS(out=best, code=code, win=win)


def place(u, H, W, pad_t, pad_l):
    """F.pad of u [N, uh, uw, C] into an [N, H, W, C] frame at (pad_t, pad_l)"""
    return F.pad(u, [0, 0, pad_l, W - u.shape[2] - pad_l, pad_t, H - u.shape[1] - pad_t])


def materialize(kind, x, H, W, scale=None, shift=None, relu=0, gate_p=None, gate_ab=None, up=None):
    """the six source kinds as a plain [N, H, W, C] map.  kind: 'plain', 'act' (gate_p [N, H, W], gate_ab [2]:
    times sigmoid(p·a + b)), 'pool_act', 'up_act' and 'up_plain' (up = (up_h, up_w, pad_t, pad_l)).
    abs_terms: the absolute terms of the affine, carried through the same map (None for plain copies)"""
    x = d(x)
    aff = scale is not None
    a = act(x, scale, shift, relu) if aff else x
    mag = (x * d(scale)).abs() + d(shift).abs() if aff else x.abs()
    if kind == "plain":
        return NS(out=x, abs_terms=None)
    if kind == "act":
        if gate_p is None:
            return NS(out=a, abs_terms=mag, q=None)
        ab = d(gate_ab)
        q = d(gate_p) * ab[0] + ab[1]
        return NS(out=a * torch.sigmoid(q).unsqueeze(-1), abs_terms=mag, q=q, act=a,
                  abs_q=(d(gate_p) * ab[0]).abs() + ab[1].abs())
    if kind == "pool_act":
        return NS(out=maxpool_act(x, scale, shift, relu, H, W).out, abs_terms=pool_windows(mag, H, W).amax(3))
    up_h, up_w, pad_t, pad_l = up
    if kind == "up_plain":
        return NS(out=place(x[:, :up_h, :up_w], H, W, pad_t, pad_l), abs_terms=None)
    assert kind == "up_act"
    u = resize(a.permute(0, 3, 1, 2), up_h, up_w).permute(0, 2, 3, 1)
    t = resize_terms(a.permute(0, 3, 1, 2), up_h, up_w)
    return NS(out=place(u, H, W, pad_t, pad_l), sum_w=place(t.sum_w.permute(0, 2, 3, 1), H, W, pad_t, pad_l),
              max_a=place(t.max_a.permute(0, 2, 3, 1), H, W, pad_t, pad_l))


def nchw_to_nhwc(x):
    return x.permute(0, 2, 3, 1)


def nhwc_to_nchw(x, scale=None, shift=None, relu=0):
    """relu?(x·scale + shift) as NCHW, and |x·scale| + |shift|"""
    r = act(x, scale, shift, relu).permute(0, 3, 1, 2)
    mag = d(x).abs() if scale is None else (d(x) * d(scale)).abs() + d(shift).abs()
    return NS(out=r, abs_terms=mag.permute(0, 3, 1, 2))


def gated_to_nchw(x, scale, shift, relu, p, ab):
    """act(x)·sigmoid(p·a + b) as NCHW; p [N, H, W]"""
    r = materialize("act", x, x.shape[1], x.shape[2], scale, shift, relu, p, ab)
    return NS(out=r.out.permute(0, 3, 1, 2), act=r.act.permute(0, 3, 1, 2), abs_terms=r.abs_terms.permute(0, 3, 1, 2),
              q=r.q.unsqueeze(1), abs_q=r.abs_q.unsqueeze(1))


def ulp(x, dtype):
    """spacing of `dtype` at |x| (the subnormal spacing below the normal range)"""
    fi = torch.finfo(dtype)
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dtype]
    _, e = torch.frexp(x.abs().clamp_min(fi.tiny))
    return torch.ldexp(torch.ones_like(x), (e - 1 - mant).to(torch.int32)).clamp_min(fi.tiny * fi.eps)


# ---- gates of the GPU op tests ----------------------------------------------------------------------
# eps of a 16-bit output: one rounding of the fp32 value plus a rounding flip from fp32 noise
EPS16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


def _worst(err, tol):
    i = int((err - tol).argmax())
    return float(err.flatten()[i]), float(tol.flatten()[i])


def check_sums(got, ref, abs_terms, what, rel=2e-5, atol=1e-6):
    """a sum accumulated in fp32 against fp64, relative to the sum of its absolute terms"""
    got = got.double()
    assert torch.isfinite(got).all(), (what, "not finite")
    err, tol = (got - ref).abs(), rel * abs_terms + atol
    assert (err <= tol).all(), (what,) + _worst(err, tol)


def check_fin(got, ref, what, scale=None, rtol=1e-6):
    """fp64 arithmetic rounded once to fp32, relative to the reference's largest term where it cancels"""
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), (what, "not finite")
    err = (got - ref).abs()
    tol = rtol * (ref.abs() if scale is None else torch.maximum(ref.abs(), scale.reshape(ref.shape)))
    assert (err <= tol).all(), (what,) + _worst(err, tol)


def check_elem(got, ref, abs_terms, prec, what, rel32=1e-5):
    """an element-wise output: 16-bit eps·|ref| + eps·1e-3·max|ref|; fp32 rel32·Σ|terms|"""
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), (what, "not finite")
    err = (got - ref).abs()
    if prec in EPS16:
        tol = EPS16[prec] * ref.abs() + EPS16[prec] * 1e-3 * ref.abs().max()
    else:
        tol = rel32 * abs_terms
    assert (err <= tol).all(), (what,) + _worst(err, tol)


# ---- convolutions (csrc/conv*.hip, pw.hip, smallcin.hip, wgrad*.hip) ---------------------------------
# Written from the sums, as k·k shifted matrix products in the operands' own precision (fp64 in the tests), with
# zero 'same' padding and no bias.  Each returns the result and abs_terms, the same sum over |operands|.

def _shifted(x, dh, dw):
    """z[n, h, w] = x[n, h + dh, w + dw], zero outside the map; x [N, H, W, C]"""
    H, W = x.shape[1], x.shape[2]
    z = torch.zeros_like(x)
    h0, h1, w0, w1 = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
    if h0 < h1 and w0 < w1:
        z[:, h0:h1, w0:w1] = x[:, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
    return z


def conv_fwd(x, w, k):
    """y[n,h,w,co] = Σ_{kh,kw,ci} x[n, h+kh−p, w+kw−p, ci]·w[co,ci,kh,kw], p = k // 2.  x [N,H,W,Cin] as the conv
    reads it, w OIHW"""
    p = k // 2
    y = torch.zeros(*x.shape[:3], w.shape[0], dtype=x.dtype, device=x.device)
    a = torch.zeros_like(y)
    for kh in range(k):
        for kw in range(k):
            xs, wt = _shifted(x, kh - p, kw - p), w[:, :, kh, kw].T
            y += xs @ wt
            a += xs.abs() @ wt.abs()
    return NS(y=y, abs_terms=a)


def conv_dgrad(dy, w, k):
    """dx[n,h,w,ci] = Σ_{kh,kw,co} dy[n, h+p−kh, w+p−kw, co]·w[co,ci,kh,kw]"""
    p = k // 2
    dx = torch.zeros(*dy.shape[:3], w.shape[1], dtype=dy.dtype, device=dy.device)
    a = torch.zeros_like(dx)
    for kh in range(k):
        for kw in range(k):
            ds, wt = _shifted(dy, p - kh, p - kw), w[:, :, kh, kw]
            dx += ds @ wt
            a += ds.abs() @ wt.abs()
    return NS(dx=dx, abs_terms=a)


def conv_wgrad(x, dy, k):
    """dw[co,ci,kh,kw] = Σ_{n,h,w} dy[n,h,w,co]·x[n, h+kh−p, w+kw−p, ci]  (OIHW)"""
    p = k // 2
    Cin, Cout = x.shape[-1], dy.shape[-1]
    dw = torch.zeros(Cout, Cin, k, k, dtype=x.dtype, device=x.device)
    a = torch.zeros_like(dw)
    g = dy.reshape(-1, Cout)
    for kh in range(k):
        for kw in range(k):
            xs = _shifted(x, kh - p, kw - p).reshape(-1, Cin)
            dw[:, :, kh, kw] = g.T @ xs
            a[:, :, kh, kw] = g.abs().T @ xs.abs()
    return NS(dw=dw, abs_terms=a)


def convt_k2s2(x, w4, bias=None):
    """ConvTranspose2d(k=2, s=2) in the UNET_OUT_SHUFFLE2 convention: the 1x1 conv w4 [4·Ct, Cin, 1, 1] of x
    [N,H,W,Cin], whose output channel (2a+b)·Ct + c of pixel (y, x) lands at out[n, 2y+a, 2x+b, c] (+ bias[c])"""
    N, H, W, _ = x.shape
    Ct = w4.shape[0] // 4
    r = conv_fwd(x, w4, 1)

    def shuffle(t):
        return t.reshape(N, H, W, 2, 2, Ct).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Ct)

    out, a = shuffle(r.y), shuffle(r.abs_terms)
    if bias is not None:
        out, a = out + bias.to(out.dtype), a + bias.to(out.dtype).abs()
    return NS(out=out, abs_terms=a)


def convt_weight4(wt):
    """nn.ConvTranspose2d weight [Cin, Ct, 2, 2] -> the equivalent 1x1 weight [4·Ct, Cin, 1, 1]"""
    Cin, Ct = wt.shape[:2]
    return wt.permute(2, 3, 1, 0).reshape(4 * Ct, Cin, 1, 1)


def conv_input(srcs, N, H, W, dtype):
    """The conv's concatenated input [N,H,W,ΣC] in fp64 from unet_src-like specs: each an NS / dict with kind
    ('plain', 'act', 'pool_act', 'up_act', 'up_plain', 'nchw'), x (the stored tensor; [N,C,H,W] for nchw) and, by
    kind, scale, shift, relu, gate_p, gate_ab, up = (up_h, up_w, pad_t, pad_l).  Each source is materialised by the
    references above (zero outside a placed map) and rounded once to the op dtype, as the kernels stage it."""
    parts = []
    for s in srcs:
        s = s if isinstance(s, dict) else vars(s)
        if s["kind"] == "nchw":
            v = d(s["x"]).permute(0, 2, 3, 1)
        else:
            v = materialize(s["kind"], s["x"], H, W, s.get("scale"), s.get("shift"), s.get("relu", 0),
                            s.get("gate_p"), s.get("gate_ab"), s.get("up")).out
        assert tuple(v.shape[:3]) == (N, H, W), (s["kind"], tuple(v.shape))
        parts.append(v.to(dtype).double())
    return torch.cat(parts, -1)


def conv_stats(y):
    """BN partial-sum expectations of the y epilogue: Σy, Σy² per channel from the unrounded y (the header's "from
    the fp32 accumulators") and the sums of their absolute terms"""
    y2 = y.reshape(-1, y.shape[-1])
    return NS(sum=y2.sum(0), sumsq=(y2 * y2).sum(0), abs_sum=y2.abs().sum(0), abs_sumsq=(y2 * y2).sum(0))


def conv_bnb(g_stored, bnb_y, scale, shift, relu, mean, invstd):
    """the bnb_* sums of a dgrad's y epilogue (unet_conv_desc): g = out as stored where relu?(bnb_y·scale+shift) > 0,
    Σg and Σg·(bnb_y − mean)·invstd.  abs_gx bounds the distributed form too: Σ|g|·(|y| + |mean|)·invstd"""
    C = g_stored.shape[-1]
    r = bn_bwd_sums(g_stored.reshape(-1, C), bnb_y.reshape(-1, C), scale, shift, relu, mean, invstd)
    r.abs_gx = (r.g.abs() * (d(bnb_y).reshape(-1, C).abs() + d(mean).abs()) * d(invstd).abs()).sum(0)
    return r


def pool_bwd(g, code, Hs, Ws, old=None):
    """MaxPool2d(2) backward: g [N,H,W,C] added at the window position code (0..3, row-major) selects, into a
    [N,Hs,Ws,C] map (Hs >= 2H, Ws >= 2W; rows / columns past the windows keep `old`)"""
    N, H, W, C = g.shape
    out = torch.zeros(N, Hs, Ws, C, dtype=torch.float64, device=g.device) if old is None else d(old).clone()
    for q in range(4):
        out[:, (q >> 1):2 * H:2, (q & 1):2 * W:2] += torch.where(code == q, d(g), torch.zeros_like(d(g)))
    return out


# ---- the exact-grid method ---------------------------------------------------------------------------
# Operands drawn on a dyadic grid make every product a multiple of one unit u.  Where Σ|terms| / u < 2^24 for an
# output element, every partial sum of those terms, in any order and any split, is an integer multiple of u below
# 2^24·u and so exactly representable in fp32: a kernel that accumulates in fp32 must return the fp64 value itself.

EXACT_CAP = float(2 ** 24)


def grid(shape, step, kmax, dtype, generator, device="cpu"):
    """k·step with k uniform on the integers [−kmax, kmax] (kmax·step and step must be exact in dtype)"""
    k = torch.randint(-kmax, kmax + 1, tuple(shape), generator=generator, device=generator.device)
    v = (k.double() * step).to(dtype)
    assert torch.equal(v.double(), k.double() * step), "grid not representable in the dtype"
    return v.to(device)


def exact_units(abs_terms, unit):
    """the largest Σ|terms| / unit over the outputs: below 2^24 every fp32 partial sum is exact"""
    return float(abs_terms.max() / unit) if abs_terms.numel() else 0.0


def check_exact(got, ref64, dtype, what, names=("n", "h", "w", "c"), mods=(0, 16, 32, 16)):
    """got must be ref64 rounded once (to nearest even) to dtype, bit for bit apart from the sign of zero.  On a
    mismatch: how many, the first wrong index, expected and got there, and the residues of the wrong indices
    (h mod 16, w mod 32, c mod 16 for an NHWC map), which name the tile edge, tap or channel fragment at fault."""
    r32 = ref64.to(torch.float32)
    assert torch.equal(r32.double(), ref64), (what, "the reference is not exact in fp32: the exactness condition fails")
    want = r32.to(dtype)
    got = got.reshape(want.shape)
    assert got.dtype == dtype, (what, got.dtype, dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    res = {}
    for dim, (nm, m) in enumerate(zip(names, mods)):
        if m and dim < idx.shape[1]:
            res[f"{nm}%{m}"] = sorted(set((idx[:, dim] % m).tolist()))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} wrong; first at {dict(zip(names, first))}: "
                         f"expected {float(want[first])!r}, got {float(got[first])!r}; residues {res}")
