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


# ---- loss -------------------------------------------------------------------------------------------

def _loss_case(seed, N, K, H, W, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, K, H, W, generator=g, dtype=torch.float64) * scale
    t = torch.randint(0, K, (N, H, W), generator=g)
    return z, t


def test_loss_fields_value_and_dz_match_oracle():
    """loss_fields -> loss_value against the oracle's dice_loss / balanced_ce_loss / dice_bce_loss (all three
    reductions, ignore_background on and off, non-default weights and smoothing), and loss_coef -> loss_dz_terms and
    loss_dz (autograd through the reference) against autograd through the oracle; K = 1, 2, 3, 5."""
    from oracle import unet_oracle as O
    for K in (1, 2, 3, 5):
        z, t = _loss_case(10 + K, 3, K, 7, 9)
        t[0] = 0                                   # an image without foreground
        if K > 1:
            t[1] = 1                               # and one without background
        zf, tf = z.flatten(2), t.flatten(1)
        f = RO.loss_fields(zf, tf)
        for ib in (1, 0):
            for red, name in enumerate(("mean", "sum", "none")):
                cfg = RO.loss_cfg(0.0, 1.0, 0.5, 1e-6, 0.7, ib, red)
                ref = O.dice_loss(z, t, 0.7, bool(ib), name)
                _close(RO.loss_value(f, K, cfg).loss, ref, ("dice", K, ib, name))
                nd = K - (1 if ib and K > 1 else 0)
                go = torch.linspace(0.3, 1.9, 3 * nd, dtype=torch.float64).reshape(3, nd) if red == 2 else 0.37
                zz = z.clone().requires_grad_(True)
                (O.dice_loss(zz, t, 0.7, bool(ib), name) * go).sum().backward()
                _close(RO.loss_dz(zf, tf, cfg, go).reshape(z.shape), zz.grad, ("dice dz", K, ib, name))
                r = RO.loss_dz_terms(zf, tf, RO.loss_coef(f, K, cfg), go, red == 2, ib)
                _close(r.dz.reshape(z.shape), zz.grad, ("dice dz by coef", K, ib, name), 1e-11)
                assert bool((r.abs_terms >= r.dz.abs() * (1 - 1e-12)).all())
        cfg = RO.loss_cfg(0.8, 1.3, 0.3, 1e-6, 1.0, 1, 0)
        zz = z.clone().requires_grad_(True)
        ref = O.dice_bce_loss(zz, t, 0.8, 1.3, 0.3)
        ref.backward()
        v = RO.loss_value(f, K, cfg)
        _close(v.loss, ref.detach(), ("dice_bce", K))
        assert float(v.abs) >= abs(float(v.loss))
        _close(RO.loss_dz(zf, tf, cfg, 1.0).reshape(z.shape), zz.grad, ("dice_bce dz", K))
        _close(RO.loss_dz_terms(zf, tf, RO.loss_coef(f, K, cfg), 1.0, 0, 1).dz.reshape(z.shape), zz.grad,
               ("dice_bce dz by coef", K), 1e-11)
        _close(RO.loss_value(f, K, RO.loss_cfg(1.0, 0.0, 0.3, 1e-3)).loss, O.balanced_ce_loss(z, t, 0.3, 1e-3),
               ("balanced ce", K))


def test_loss_deep_supervision_and_partial_rows():
    """Σ_s w_s·loss_s and the per-set dz (set weight in the coefficients) against the oracle's deep_supervision_loss;
    the partial table's rows add up to the fields, row r covering ceil(HW / rows) pixels."""
    from oracle import unet_oracle as O
    K, ws = 2, [1.0, 0.4, 0.2, 0.1]
    zs = [_loss_case(30 + s, 2, K, 5, 8)[0].requires_grad_(True) for s in range(4)]
    t = _loss_case(40, 2, K, 5, 8)[1]
    O.deep_supervision_loss(zs, t, O.dice_bce_loss, ws).backward()
    cfg, tf = RO.loss_cfg(), t.flatten(1)
    total = 0.0
    for z, w in zip(zs, ws):
        zf = z.detach().flatten(2)
        f = RO.loss_fields(zf, tf)
        total = total + w * RO.loss_value(f, K, cfg).loss
        _close(RO.loss_dz(zf, tf, cfg, 1.0, set_w=w).reshape(z.shape), z.grad, ("dz", w))
        _close(RO.loss_dz_terms(zf, tf, RO.loss_coef(f, K, cfg, w), 1.0, 0, 1).dz.reshape(z.shape), z.grad,
               ("dz by coef", w), 1e-11)
        for rows in (1, 3, 40):
            part = RO.loss_partial(zf, tf, rows).part
            assert part.shape == (2, rows, 4 + 3 * K)
            _close(part.sum(1), f, ("partial", rows))
    _close(total, O.deep_supervision_loss([z.detach() for z in zs], t, O.dice_bce_loss, ws), "deep supervision")
    part = RO.loss_partial(zf, tf, 3).part     # HW = 40, per = 14: rows of 14, 14 and 12 pixels
    assert part[0, :, 4 + 2::3].sum(-1).tolist() == [14.0, 14.0, 12.0]


def test_loss_out_of_range_labels():
    """a label < 0 or >= K: an all-zero one-hot row and cross-entropy weight 0, still counted in P_c — the fields
    equal those of the in-range pixels plus the out-of-range pixels' softmax in P_c; dz there is the Dice
    gradient through P alone (autograd), and the coefficient formula agrees."""
    K = 3
    z, t = _loss_case(50, 2, K, 6, 7)
    zf, tf = z.flatten(2), t.flatten(1).clone()
    bad = torch.zeros_like(tf, dtype=torch.bool)
    bad[:, ::5] = True
    tf[bad] = torch.tensor([-1, K, 255, -7])[torch.arange(int(bad.sum())) % 4]
    f = RO.loss_fields(zf, tf)
    keep = [RO.loss_fields(zf[n:n + 1][..., ~bad[n]], tf[n:n + 1][..., ~bad[n]])[0] for n in range(2)]
    extra = torch.zeros_like(f)
    for n in range(2):
        extra[n, 5::3] = torch.softmax(zf[n][:, bad[n]], 0).sum(-1)
    _close(f, torch.stack(keep) + extra, "fields")
    for ib in (0, 1):
        cfg = RO.loss_cfg(0.8, 1.3, 0.3, 1e-6, 1.0, ib, 1)
        dz = RO.loss_dz(zf, tf, cfg, 0.37)
        r = RO.loss_dz_terms(zf, tf, RO.loss_coef(f, K, cfg), 0.37, 0, ib)
        _close(r.dz, dz, ("dz", ib), 1e-11)
        assert float(dz[0][:, bad[0]].abs().max()) > 0


# ---- resampling -------------------------------------------------------------------------------------

RESIZE_GEO = [(8, 12, 16, 24), (8, 12, 64, 96), (7, 9, 15, 17), (9, 11, 9, 11), (1, 5, 8, 10), (5, 7, 1, 1),
              (9, 11, 4, 5)]


def test_resize_and_adjoints_match_dense_weight_matrices():
    """resize (F.interpolate), resize_bwd and upsample_bwd (autograd) against Wy·x·Wxᵀ and its transpose with the
    dense tap matrices of lin_axis (an index-level formulation); the bound operands of resize_terms /
    resize_bwd_terms dominate the values they bound."""
    g = torch.Generator().manual_seed(3)
    for Hi, Wi, Ho, Wo in RESIZE_GEO:
        x = torch.randn(2, 3, Hi, Wi, generator=g, dtype=torch.float64)
        dy = torch.randn(2, 3, Ho, Wo, generator=g, dtype=torch.float64)
        ay, ax = RO.lin_axis(Hi, Ho), RO.lin_axis(Wi, Wo)
        assert bool((ay.W.sum(1) - 1).abs().max() < 1e-15) and bool((ax.W.sum(1) - 1).abs().max() < 1e-15)
        y = RO.resize(x, Ho, Wo)
        _close(y, ay.W @ x @ ax.W.T, ("resize", Hi, Wi, Ho, Wo))
        old = torch.randn(2, 3, Hi, Wi, generator=g, dtype=torch.float64)
        _close(RO.resize_bwd(dy, Hi, Wi), ay.W.T @ dy @ ax.W, ("resize_bwd", Hi, Wi, Ho, Wo))
        _close(RO.resize_bwd(dy, Hi, Wi, old), ay.W.T @ dy @ ax.W + old, ("resize_bwd accum", Hi, Wi, Ho, Wo))
        t = RO.resize_terms(x, Ho, Wo)
        assert bool((t.sum_w >= y.abs() - 1e-14).all()) and bool((t.max_a >= t.sum_w - 1e-14).all())
        tb = RO.resize_bwd_terms(dy, Hi, Wi)
        assert bool((tb.sum_w >= RO.resize_bwd(dy, Hi, Wi).abs() - 1e-13).all()) and bool((tb.sum_a >= tb.sum_w - 1e-13).all())
        # the padded NHWC form: unequal pads on the four sides
        pt, pl, Hp, Wp = 1, 2, Ho + 4, Wo + 3
        d_up = torch.randn(2, Hp, Wp, 3, generator=g, dtype=torch.float64)
        inner = d_up[:, pt:pt + Ho, pl:pl + Wo].permute(0, 3, 1, 2)
        _close(RO.upsample_bwd(d_up, Hi, Wi, Ho, Wo, pt, pl), (ay.W.T @ inner @ ax.W).permute(0, 2, 3, 1),
               ("upsample_bwd", Hi, Wi, Ho, Wo))


# ---- ConvTranspose2d backward prep, max-pool, materialised sources, layouts ---------------------------

def test_convt_bwd_prep_matches_pixel_unshuffle_and_autograd():
    g = torch.Generator().manual_seed(4)
    N, h, w, Ct, pt, pl = 2, 3, 5, 4, 1, 2
    Hp, Wp = 2 * h + pt + 1, 2 * w + pl + 3
    d_up = torch.randn(N, Hp, Wp, Ct, generator=g, dtype=torch.float64)
    r = RO.convt_bwd_prep(d_up, h, w, pt, pl)
    inner = d_up[:, pt:pt + 2 * h, pl:pl + 2 * w].permute(0, 3, 1, 2)
    pu = F.pixel_unshuffle(inner, 2).reshape(N, Ct, 4, h, w).permute(0, 3, 4, 2, 1).reshape(N, h, w, 4 * Ct)
    assert torch.equal(r.s2d, pu)
    # the s2d map is the output gradient of the equivalent 1x1 conv: with it, ConvTranspose2d's input and bias
    # gradients come out as a matrix product and a sum
    m = torch.nn.ConvTranspose2d(6, Ct, 2, 2).double()
    x = torch.randn(N, 6, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    m(x).backward(inner)
    wm = m.weight.detach().permute(2, 3, 1, 0).reshape(4 * Ct, 6)           # [(2a+b)·Ct + c][cin]
    _close((r.s2d @ wm).permute(0, 3, 1, 2), x.grad, "dx through s2d")
    _close(r.bias, m.bias.grad, "bias")
    assert bool((r.abs_bias >= r.bias.abs()).all())


def test_maxpool_act_matches_max_pool2d():
    """values and first-maximum codes against F.max_pool2d(return_indices=True) on tie-rich data (even and odd
    source sizes, ReLU on and off); a NaN comes out with its own position's code"""
    g = torch.Generator().manual_seed(5)
    for Hs, Ws in ((10, 14), (11, 15)):
        H, W, C = Hs // 2, Ws // 2, 3
        y = torch.randint(-32, 33, (2, Hs, Ws, C), generator=g).double() / 8
        scale = torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)
        shift = torch.tensor([1 / 64, -3 / 64, 0.0], dtype=torch.float64)
        for relu in (0, 1):
            r = RO.maxpool_act(y, scale, shift, relu, H, W)
            a = RO.act(y, scale, shift, relu).permute(0, 3, 1, 2)
            v, idx = F.max_pool2d(a, 2, return_indices=True)
            yy, xx = idx // Ws, idx % Ws
            oy = torch.arange(H).view(1, 1, H, 1)
            ox = torch.arange(W).view(1, 1, 1, W)
            code = 2 * (yy - 2 * oy) + (xx - 2 * ox)
            assert torch.equal(r.out, v.permute(0, 2, 3, 1))
            assert torch.equal(r.code.long(), code.permute(0, 2, 3, 1))
            if relu:
                assert int(((r.win == 0).all(3) & (r.code == 0)).sum()) > 0      # whole windows tie at 0
    y = torch.zeros(1, 2, 8, 1, dtype=torch.float64)
    for q in range(4):
        y[0, q >> 1, 2 * q + (q & 1), 0] = float("nan")
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    r = RO.maxpool_act(y, one, zero, 1, 1, 4)
    v, idx = F.max_pool2d(torch.relu(y.permute(0, 3, 1, 2)), 2, return_indices=True)
    assert bool(r.out.isnan().all()) and bool(v.isnan().all()) and r.code.flatten().tolist() == [0, 1, 2, 3]
    assert (2 * (idx // 8) + idx % 8 - 2 * torch.arange(4)).flatten().tolist() == [0, 1, 2, 3]


def test_materialize_kinds_and_layouts():
    """the six source kinds against nn.functional on NCHW tensors, and the three layout maps element by element"""
    g = torch.Generator().manual_seed(6)
    N, H, W, C = 2, 6, 10, 5
    scale, shift = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    nchw = x.permute(0, 3, 1, 2)
    aff = nchw * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)
    assert torch.equal(RO.materialize("plain", x, H, W).out, x)
    for relu in (0, 1):
        a = F.relu(aff) if relu else aff
        _close(RO.materialize("act", x, H, W, scale, shift, relu).out, a.permute(0, 2, 3, 1), ("act", relu))
        p, ab = torch.randn(N, H, W, generator=g, dtype=torch.float64), torch.tensor([1.3, -0.2], dtype=torch.float64)
        gate = torch.sigmoid(p * 1.3 - 0.2)
        r = RO.materialize("act", x, H, W, scale, shift, relu, p, ab)
        _close(r.out, (a * gate.unsqueeze(1)).permute(0, 2, 3, 1), ("gated", relu))
        rg = RO.gated_to_nchw(x, scale, shift, relu, p, ab)
        _close(rg.out, a * gate.unsqueeze(1), ("gated_to_nchw", relu))
        _close(RO.nhwc_to_nchw(x, scale, shift, relu).out, a, ("nhwc_to_nchw", relu))
        assert bool((RO.nhwc_to_nchw(x, scale, shift, relu).abs_terms >= a.abs() - 1e-14).all())
        r = RO.materialize("pool_act", x, H // 2, W // 2, scale, shift, relu)
        _close(r.out, F.max_pool2d(a, 2).permute(0, 2, 3, 1), ("pool_act", relu))
        up = (2 * H, 2 * W, 1, 2)
        r = RO.materialize("up_act", x, 2 * H + 3, 2 * W + 3, scale, shift, relu, up=up)
        ref = F.pad(F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=True), [2, 1, 1, 2])
        _close(r.out, ref.permute(0, 2, 3, 1), ("up_act", relu))
        assert bool((r.sum_w >= r.out.abs() - 1e-14).all()) and bool((r.max_a >= r.sum_w - 1e-14).all())
    r = RO.materialize("up_plain", x, H + 3, W + 3, up=(H, W, 1, 2))
    assert torch.equal(r.out, F.pad(nchw, [2, 1, 1, 2]).permute(0, 2, 3, 1))
    assert torch.equal(RO.nhwc_to_nchw(x).out, nchw)
    back = RO.nchw_to_nhwc(nchw.contiguous())
    for n, h, w, c in ((0, 0, 0, 0), (1, 5, 9, 4), (1, 2, 7, 3)):
        assert float(back[n, h, w, c]) == float(nchw[n, c, h, w])
    # ulp: the spacing at 1 and just below, and the subnormal spacing
    one = torch.tensor([1.0, 0.99, 0.0], dtype=torch.float64)
    assert RO.ulp(one, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -8, 2.0 ** -133]
    assert RO.ulp(one, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -11, 2.0 ** -24]


# ---- convolutions and the exact-grid method ----------------------------------------------------------

CONV_REF_SHAPES = [(2, 5, 7, 5, 6, 3), (1, 4, 9, 20, 3, 1), (3, 6, 4, 7, 33, 3), (1, 1, 3, 4, 2, 3), (2, 9, 5, 33, 17, 1)]


def _conv_operands(shape, seed):
    N, H, W, Cin, Cout, k = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
    dy = torch.randn(N, H, W, Cout, generator=g, dtype=torch.float64)
    return x, w, dy


def test_conv_references_match_torch():
    """conv_fwd / conv_dgrad / conv_wgrad (shifted matrix products) against fp64 F.conv2d, F.conv_transpose2d and
    torch.nn.grad.conv2d_weight: non-square maps, channel counts off every multiple of 16, k = 1 and 3"""
    for i, shape in enumerate(CONV_REF_SHAPES):
        x, w, dy = _conv_operands(shape, 40 + i)
        k, p = shape[-1], shape[-1] // 2
        xc, dyc = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        r = RO.conv_fwd(x, w, k)
        _close(r.y, F.conv2d(xc, w, padding=p).permute(0, 2, 3, 1), ("fwd", shape))
        _close(r.abs_terms, F.conv2d(xc.abs(), w.abs(), padding=p).permute(0, 2, 3, 1), ("fwd abs", shape))
        r = RO.conv_dgrad(dy, w, k)
        _close(r.dx, F.conv_transpose2d(dyc, w, padding=p).permute(0, 2, 3, 1), ("dgrad", shape))
        _close(r.abs_terms, F.conv_transpose2d(dyc.abs(), w.abs(), padding=p).permute(0, 2, 3, 1), ("dgrad abs", shape))
        r = RO.conv_wgrad(x, dy, k)
        _close(r.dw, torch.nn.grad.conv2d_weight(xc, w.shape, dyc, padding=p), ("wgrad", shape))
        _close(r.abs_terms, torch.nn.grad.conv2d_weight(xc.abs(), w.shape, dyc.abs(), padding=p), ("wgrad abs", shape))
        # the three are one bilinear form: <dy, conv(x, w)> = <x, dgrad(dy, w)> = <w, wgrad(x, dy)>
        s = (dy * RO.conv_fwd(x, w, k).y).sum()
        _close((x * RO.conv_dgrad(dy, w, k).dx).sum(), s, ("adjoint dx", shape), 1e-11)
        _close((w * RO.conv_wgrad(x, dy, k).dw).sum(), s, ("adjoint dw", shape), 1e-11)


def test_convt_k2s2_matches_torch():
    g = torch.Generator().manual_seed(50)
    for N, H, W, Cin, Ct in ((2, 3, 5, 6, 4), (1, 4, 2, 5, 3)):
        x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
        wt = torch.randn(Cin, Ct, 2, 2, generator=g, dtype=torch.float64)
        b = torch.randn(Ct, generator=g, dtype=torch.float64)
        for bias in (b, None):
            r = RO.convt_k2s2(x, RO.convt_weight4(wt), bias)
            ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), wt, bias, stride=2).permute(0, 2, 3, 1)
            _close(r.out, ref, ("convt", N, H, W, bias is None))
            ra = F.conv_transpose2d(x.permute(0, 3, 1, 2).abs(), wt.abs(), None if bias is None else b.abs(), stride=2)
            _close(r.abs_terms, ra.permute(0, 2, 3, 1), ("convt abs", N, H, W))


def test_conv_input_concat_with_placed_map():
    """a gated BN activation next to the padded bilinear up-sampling of another, rounded to the op dtype, against
    plain torch; then through conv_fwd against F.conv2d of the same concat"""
    g = torch.Generator().manual_seed(51)
    N, H, W, C0, C1 = 2, 7, 10, 5, 6
    y0 = torch.randn(N, H, W, C0, generator=g).bfloat16()
    y1 = torch.randn(N, 3, 4, C1, generator=g).bfloat16()
    ab0, ab1 = torch.randn(2, C0, generator=g), torch.randn(2, C1, generator=g)
    p, pab = torch.randn(N, H, W, generator=g), torch.tensor([0.7, -0.2])
    up = (5, 7, 1, 2)
    srcs = [dict(kind="act", x=y0, scale=ab0[0], shift=ab0[1], relu=1, gate_p=p, gate_ab=pab),
            dict(kind="up_act", x=y1, scale=ab1[0], shift=ab1[1], relu=0, up=up)]
    x = RO.conv_input(srcs, N, H, W, torch.bfloat16)
    a0 = (y0.double() * ab0[0].double() + ab0[1].double()).clamp_min(0)
    a0 = a0 * torch.sigmoid(p.double() * pab[0].double() + pab[1].double()).unsqueeze(-1)
    a1 = (y1.double() * ab1[0].double() + ab1[1].double()).permute(0, 3, 1, 2)
    a1 = F.interpolate(a1, size=up[:2], mode="bilinear", align_corners=True)
    a1 = F.pad(a1, [up[3], W - up[1] - up[3], up[2], H - up[0] - up[2]]).permute(0, 2, 3, 1)
    want = torch.cat([a0, a1], -1).bfloat16().double()
    assert torch.equal(x, want)
    assert (x[:, 0, :, C0:] == 0).all() and (x[:, :, :2, C0:] == 0).all()   # zero outside the placed map
    w = torch.randn(4, C0 + C1, 3, 3, generator=g, dtype=torch.float64)
    _close(RO.conv_fwd(x, w, 3).y, F.conv2d(want.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1), "concat conv")
    # an NCHW source is transposed, a pooled one is the first-maximum max-pool
    xn = torch.randn(N, 3, H, W, generator=g)
    assert torch.equal(RO.conv_input([dict(kind="nchw", x=xn)], N, H, W, torch.float32), xn.double().permute(0, 2, 3, 1))
    yp = torch.randn(N, 2 * H + 1, 2 * W, C0, generator=g)
    xp = RO.conv_input([dict(kind="pool_act", x=yp, scale=ab0[0], shift=ab0[1], relu=1)], N, H, W, torch.float32)
    ap = (yp.double() * ab0[0].double() + ab0[1].double()).clamp_min(0).permute(0, 3, 1, 2)
    assert torch.equal(xp, F.max_pool2d(ap, 2).permute(0, 2, 3, 1).float().double())


def test_conv_stats_bnb_and_pool_bwd():
    g = torch.Generator().manual_seed(52)
    y = torch.randn(2, 4, 5, 3, generator=g, dtype=torch.float64)
    st = RO.conv_stats(y)
    _close(st.sum, y.sum((0, 1, 2)), "Σy")
    _close(st.sumsq, (y * y).sum((0, 1, 2)), "Σy²")
    by = torch.randn(2, 4, 5, 3, generator=g, dtype=torch.float64)
    sc, sf, mu, iv = (torch.randn(3, generator=g, dtype=torch.float64) for _ in range(4))
    b = RO.conv_bnb(y, by, sc, sf, 1, mu, iv)
    m = (by * sc + sf > 0).double()
    _close(b.sum_g, (y * m).sum((0, 1, 2)), "Σg")
    _close(b.sum_gx, (y * m * (by - mu) * iv).sum((0, 1, 2)), "Σg·x̂")
    assert (b.abs_gx >= b.sum_gx.abs()).all()
    # pool_bwd with the reference's own codes is autograd's max_pool2d backward (no ties in random data)
    a = torch.randn(2, 9, 10, 3, generator=g, dtype=torch.float64)
    code = RO.maxpool_act(a, None, None, 0, 4, 5).code
    gp = torch.randn(2, 4, 5, 3, generator=g, dtype=torch.float64)
    old = torch.randn(2, 9, 10, 3, generator=g, dtype=torch.float64)
    ac = a.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(ac, 2).backward(gp.permute(0, 3, 1, 2))
    _close(RO.pool_bwd(gp, code, 9, 10, old), ac.grad.permute(0, 2, 3, 1) + old, "pool_bwd")


def _emulate(x, w, k, dtype, order_seed, splits, mutate=None, kc=8):
    """A correct kernel on the CPU: the k·k·ceil(Cin / kc) chunk products of a 'same' conv, accumulated in fp32 in
    a shuffled order into `splits` slabs that are then added in fp32, and rounded once to dtype (nearest even).
    mutate: one of the five subtle errors the exact gate must reject."""
    N, H, W, Cin = x.shape
    Cout, p = w.shape[0], k // 2
    xf, wf = x.float(), w.float()
    if mutate == "last_channel":
        xf = xf.clone()
        xf[..., Cin - 1] = 0
    chunks = [(kh, kw, c0) for kh in range(k) for kw in range(k) for c0 in range(0, Cin, kc)]
    order = torch.randperm(len(chunks), generator=torch.Generator().manual_seed(order_seed)).tolist()
    slabs = [torch.zeros(N, H, W, Cout) for _ in range(splits)]
    for j, ci in enumerate(order):
        kh, kw, c0 = chunks[ci]
        xs = RO._shifted(xf, kh - p, kw - p)
        if mutate == "halo_row" and (kh, kw) == (0, 1):   # pixel (0, 2, 3) reads its upper neighbour from its own row
            xs = xs.clone()
            xs[0, 2, 3] = xf[0, 2, 3]
        t = xs[..., c0:c0 + kc] @ wf[:, c0:c0 + kc, kh, kw].T
        if mutate == "drop_tap" and (kh, kw) == (1, 2):   # the right-hand tap of border pixel (0, 0, 2)
            t[0, 0, 2] = 0
        slabs[j % splits] += t
    if mutate == "slab_twice":
        slabs[0][0, 3, 1] *= 2
    acc = slabs[0]
    for s in slabs[1:]:
        acc = acc + s
    if mutate == "truncate" and dtype != torch.float32:
        bits = 16
        return acc, (acc.view(torch.int32) >> bits << bits).view(torch.float32).to(dtype)
    return acc, acc.to(dtype)


def test_exact_gate_is_sharp():
    """On grid operands a correct kernel — any chunk order, 1-, 2- or 8-way split-K — equals fp64 bit for bit, and each
    of five one-term errors is rejected, in the fp32 accumulator and in the rounded 16-bit output"""
    g = torch.Generator().manual_seed(53)
    N, H, W, Cin, Cout, k = 1, 6, 7, 20, 12, 3
    x = RO.grid((N, H, W, Cin), 0.25, 12, torch.bfloat16, g).double()
    w = RO.grid((Cout, Cin, k, k), 0.125, 4, torch.float32, g).double()
    ref = RO.conv_fwd(x, w, k)
    assert RO.exact_units(ref.abs_terms, 0.25 * 0.125) < 2 ** 22
    assert ((ref.y.float().to(torch.bfloat16).double() - ref.y) != 0).any()        # the rounding is exercised,
    tie = (ref.y.abs() * 32).to(torch.int64)                                          # ... with ties among it
    assert ((ref.y.abs() >= 8) & (ref.y.abs() < 16) & (tie % 4 == 2)).any()
    for seed in range(3):
        for splits in (1, 2, 8):
            acc, out = _emulate(x, w, k, torch.bfloat16, seed, splits)
            RO.check_exact(acc, ref.y, torch.float32, "accumulator")
            RO.check_exact(out, ref.y, torch.bfloat16, "bf16 output")
    for mutate in ("drop_tap", "last_channel", "halo_row", "slab_twice", "truncate"):
        acc, out = _emulate(x, w, k, torch.bfloat16, 0, 2, mutate)
        for got, dt in ((acc, torch.float32), (out, torch.bfloat16)):
            if mutate == "truncate" and dt == torch.float32:
                continue
            try:
                RO.check_exact(got, ref.y, dt, mutate)
            except AssertionError as e:
                msg = str(e)
                assert "wrong; first at" in msg and "h%16" in msg and "c%16" in msg, msg
                if mutate == "drop_tap":
                    assert "'h': 0, 'w': 2" in msg and "'w%32': [2]" in msg, msg
                if mutate == "slab_twice":
                    assert "'h': 3, 'w': 1" in msg, msg
            else:
                raise AssertionError(f"the exact gate passed the mutation {mutate} ({dt})")


def test_grid_and_exact_units():
    g = torch.Generator().manual_seed(54)
    v = RO.grid((1000,), 0.25, 12, torch.bfloat16, g)
    assert v.dtype == torch.bfloat16 and float(v.abs().max()) == 3.0 and float(v.min()) == -3.0
    assert torch.equal(v.double() * 4, (v.double() * 4).round())
    assert (v == 0).any()
    assert RO.exact_units(torch.tensor([1.0, 8.0]), 0.125) == 64.0
    try:
        RO.grid((4,), 1.0 / 1024, 1000, torch.bfloat16, g)
    except AssertionError:
        pass
    else:
        raise AssertionError("a grid the dtype cannot hold was accepted")
