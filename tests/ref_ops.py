"""fp64 references of the streaming kernels around the convolutions (csrc/bn.hip, csrc/gate.hip and the
OutConv part of csrc/misc.hip), written from the maths of nn.BatchNorm2d, ReLU and AttentionGate
(layers.py:126-192), not from the kernels.  Pure torch; every function takes the kernels' own operands (any
dtype, any device), evaluates in float64 and returns what the matching entry point must produce, plus the
sums of absolute terms ("natural scales") that the tests gate the fp32 sums against.

Layouts: activations [P, C] (NHWC flattened over pixels), per-channel vectors [C], affine pairs [2, C]
(scale, shift), coefficient triples [3, C] (A, B, Cc), OutConv logits [N, K, H, W].
tests/test_ref_ops_cpu.py proves the formulas against torch autograd."""

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
