"""The fp64 references of tests/ref_ops.py against torch autograd (CPU, float64), so that the GPU op tests
that use them do not rest on formulas checked only against themselves."""

import torch
import torch.nn.functional as F

import ref_ops as RO

EPS = 1e-5


def _close(got, ref, what, tol=1e-12):
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    assert err <= tol * scale, (what, err, scale)


def test_bn_backward_matches_autograd():
    """bn_bwd_sums -> bn_bwd_coef -> bn_bwd_apply reproduce autograd's input gradient, dγ and dβ of
    F.batch_norm + ReLU: training mode (count = P) and eval mode (count = 0, running statistics)."""
    g = torch.Generator().manual_seed(0)
    P, C = 257, 7
    y0 = torch.randn(P, C, generator=g, dtype=torch.float64) * 2 + 0.5
    da = torch.randn(P, C, generator=g, dtype=torch.float64)
    gamma0 = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta0 = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    rm = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    rv = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    for training in (True, False):
        for relu in (1, 0):
            y, gamma, beta = (t.clone().requires_grad_(True) for t in (y0, gamma0, beta0))
            out = F.batch_norm(y, None if training else rm, None if training else rv, gamma, beta, training, 0.0, EPS)
            if relu:
                out = F.relu(out)
            (out * da).sum().backward()
            if training:
                mean = y0.mean(0)
                invstd = 1.0 / torch.sqrt(y0.var(0, unbiased=False) + EPS)
                scale, shift = gamma0 * invstd, beta0 - mean * gamma0 * invstd
            else:
                e = RO.bn_eval_affine(gamma0, beta0, rm, rv, EPS)
                mean, invstd, scale, shift = e.mean, e.invstd, e.scale, e.shift
            s = RO.bn_bwd_sums(da, y0, scale, shift, relu, mean, invstd)
            c = RO.bn_bwd_coef(s.sum_g, s.sum_gx, P if training else 0, gamma0, mean, invstd)
            dy = RO.bn_bwd_apply(s.g, y0, c.coef).dy
            _close(dy, y.grad, ("dy", training, relu))
            _close(c.dgamma, gamma.grad, ("dgamma", training, relu))
            _close(c.dbeta, beta.grad, ("dbeta", training, relu))
            if not training:
                assert float(c.coef[1:].abs().max()) == 0.0


def test_gate_chain_matches_autograd():
    """gate_psi -> gate_bwd1 -> coef (C = 1) -> gate_bwd2 -> two coefs -> gate_bwd3 reproduce autograd's gradients
    of out = x·sigmoid(BN_psi(relu(BN_g(gw) + BN_x(xw))·wpsi)) with respect to gw, xw, x, wpsi and all six BatchNorm
    parameters (batch statistics everywhere)."""
    g = torch.Generator().manual_seed(1)
    P, Cx, Ci = 301, 6, 5

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)

    gw, xw, yx, dout = rn(P, Ci) * 1.5 + 0.3, rn(P, Ci) - 0.2, rn(P, Cx), rn(P, Cx)
    sx, bx = torch.rand(Cx, generator=g, dtype=torch.float64) + 0.5, rn(Cx) * 0.2
    wpsi = rn(Ci) * 0.5
    bn_g, bn_x, bn_p = (rn(Ci) * 0.3 + 1, rn(Ci) * 0.2), (rn(Ci) * 0.3 + 1, rn(Ci) * 0.2), (rn(1) * 0.1 + 1.2, rn(1) * 0.3)
    x = RO.act(yx, sx, bx, 1)
    ref = RO.gate_autograd(gw, xw, x, dout, wpsi, bn_g, bn_x, bn_p, EPS)

    def stats(t, bn):
        mean = t.mean(0)
        invstd = 1.0 / torch.sqrt(t.var(0, unbiased=False) + EPS)
        return mean, invstd, torch.stack([bn[0] * invstd, bn[1] - mean * bn[0] * invstd])

    gm, gi, gab = stats(gw, bn_g)
    xm, xi, xab = stats(xw, bn_x)
    f = RO.gate_psi(gw, xw, gab, xab, wpsi)
    _close(f.p, ref.p, "p")
    pm, pi, pab = stats(f.p.unsqueeze(-1), bn_p)
    _close(f.sum_p / P, pm.reshape(()), "mean(p)")
    b1 = RO.gate_bwd1(dout, yx, sx, bx, 1, f.p, pab, pm, pi)
    _close(b1.dx, ref.d_x, "dx")
    pc = RO.bn_bwd_coef(b1.sum_dq.reshape(1), b1.sum_dqp.reshape(1), P, bn_p[0], pm, pi)
    _close(pc.dgamma, ref.d_psi_gamma, "psi dgamma")
    _close(pc.dbeta, ref.d_psi_beta, "psi dbeta")
    b2 = RO.gate_bwd2(gw, xw, gab, xab, gm, gi, xm, xi, wpsi, b1.dq, f.p, pc.coef)
    gc = RO.bn_bwd_coef(b2.sums[0], b2.sums[1], P, bn_g[0], gm, gi)
    xc = RO.bn_bwd_coef(b2.sums[0], b2.sums[2], P, bn_x[0], xm, xi)
    _close(b2.sums[3], ref.d_wpsi, "dwpsi")
    _close(gc.dgamma, ref.d_g_gamma, "W_g dgamma")
    _close(gc.dbeta, ref.d_g_beta, "W_g dbeta")
    _close(xc.dgamma, ref.d_x_gamma, "W_x dgamma")
    _close(xc.dbeta, ref.d_x_beta, "W_x dbeta")
    b3 = RO.gate_bwd3(gw, xw, gab, xab, wpsi, b1.dq, f.p, pc.coef, gc.coef, xc.coef)
    _close(b3.dgw, ref.d_gw, "dgw", 1e-11)
    _close(b3.dxw, ref.d_xw, "dxw", 1e-11)
    # the accumulating form of dx
    old = rn(P, Cx)
    _close(RO.gate_bwd1(dout, yx, sx, bx, 1, f.p, pab, pm, pi, dx_old=old).dx, ref.d_x + old, "dx accum")


def test_bn_finalize_matches_batchnorm2d():
    """bn_finalize's statistics, affine and running statistics against nn.BatchNorm2d in double: momentum 0.1 and
    momentum=None (cumulative average) over two steps; count == 1 keeps the biased variance; the clamp."""
    g = torch.Generator().manual_seed(2)
    N, C, H, W, rows = 3, 4, 5, 7, 6
    for momentum in (0.1, None):
        bn = torch.nn.BatchNorm2d(C, momentum=momentum, eps=EPS).double().train()
        with torch.no_grad():
            bn.weight.copy_(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=g, dtype=torch.float64))
        rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
        for step in range(2):
            x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * (1 + step) + 0.7
            out = bn(x)
            xp = x.permute(0, 2, 3, 1).reshape(-1, C)            # [P, C]
            chunks = xp.split((xp.shape[0] + rows - 1) // rows)
            stats = torch.stack([torch.stack([c.sum(0) for c in chunks], -1),
                                 torch.stack([(c * c).sum(0) for c in chunks], -1)])
            r = RO.bn_finalize(stats, xp.shape[0], bn.weight.detach(), bn.bias.detach(), rm, rv, nbt,
                               -1.0 if momentum is None else momentum, EPS)
            _close(r.running_mean, bn.running_mean, ("running_mean", momentum, step))
            _close(r.running_var, bn.running_var, ("running_var", momentum, step))
            assert r.nbt == int(bn.num_batches_tracked)
            _close(xp * r.scale + r.shift, out.detach().permute(0, 2, 3, 1).reshape(-1, C), "affine", 1e-11)
            _close(r.mean, xp.mean(0), "mean")
            _close(r.invstd, 1.0 / torch.sqrt(xp.var(0, unbiased=False) + EPS), "invstd", 1e-11)
            rm, rv, nbt = r.running_mean, r.running_var, r.nbt
    # one sample: torch's unbiased variance would divide by 0; the biased value (0) is kept
    one = torch.tensor([[[2.0]], [[4.0]]], dtype=torch.float64)      # [2][C=1][rows=1]
    r = RO.bn_finalize(one, 1, torch.ones(1), torch.zeros(1), torch.zeros(1), torch.ones(1), 0, 0.1, EPS)
    assert float(r.var) == 0.0 and abs(float(r.running_var) - 0.9) < 1e-15 and abs(float(r.running_mean) - 0.2) < 1e-15
    # Σx²/count < mean² by rounding: clamped, invstd = 1/sqrt(eps)
    neg = torch.tensor([[[30.0]], [[89.99]]], dtype=torch.float64)
    r = RO.bn_finalize(neg, 10, torch.ones(1), torch.zeros(1))
    assert float(r.var) == 0.0 and abs(float(r.invstd) - EPS ** -0.5) < 1e-9 and r.running_mean is None
