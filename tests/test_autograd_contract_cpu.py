"""CPU: the reference side of tests/test_gpu_autograd_contract.py.

Runs the fp64 oracle of every case of the GPU file (its tables and its `oracle_run`, imported from it) and checks that
each reference means something: finite values, a non-zero gradient for every parameter the loss reaches, the
expected set of unreached parameters for each partial-output loss, freeze sets that name existing parameters and
together cover every parameter, and conversion ops whose autograd gives a gradient of the leaf's dtype and shape.
No GPU and no HIP library."""

import pytest
import torch

import test_gpu_autograd_contract as G


def _meaningful(ref, unused=(), dx=False):
    for o in ref.outs:
        assert torch.isfinite(o).all() and float(o.abs().max()) > 0
    assert ref.loss == ref.loss and abs(ref.loss) < float("inf")
    assert sorted(k for k, g in ref.grads.items() if g is None) == sorted(unused)
    for k, g in ref.grads.items():
        if g is not None:
            assert g.dtype == torch.float64 and torch.isfinite(g).all(), k
    if dx:
        assert torch.isfinite(ref.dx).all() and float(ref.dx.norm()) > 0
        # every input channel and every image carries gradient
        assert float(ref.dx.abs().amax(dim=(0, 2, 3)).min()) > 0 and float(ref.dx.abs().amax(dim=(1, 2, 3)).min()) > 0


def _conditioned(kind, n_ch, data, ref, **kw):
    """two fp32 executions of the oracle (oneDNN convolutions, and ATen's own with oneDNN off: different summation
    orders) both agree with its fp64 run `ref` within 1e-4 (a tenth of the GPU file's fp32 gate) on every gradient
    and on dx, by the gate's measure: no ReLU mask or pool argmax that matters sits within fp32 rounding of a tie"""
    for onednn in (True, False):
        with torch.backends.mkldnn.flags(enabled=onednn):
            r32 = G.oracle_run(kind, n_ch, data, G.geometry(n_ch)[0], dtype=torch.float32, **kw)
        for o, r in zip(r32.outs, ref.outs):
            assert float((o - r).abs().max()) <= 5e-5
        for k, g in ref.grads.items():
            if g is not None:
                assert float((r32.grads[k] - g).abs().max()) <= 1e-4 * (float(g.abs().max()) + 1e-12), (onednn, k)
        if ref.dx is not None:
            assert float((r32.dx - ref.dx).abs().max()) <= 1e-4 * float(ref.dx.abs().max()), onednn


def _nonzero(ref, names):
    for k in names:
        assert float(ref.grads[k].norm()) > 0, k


@pytest.mark.parametrize("loss", ["linear", "dice_bce"])
@pytest.mark.parametrize("kind,n_ch", sorted({(k, c) for k, c, _ in G.DX_CASES}))
def test_input_gradient_references(kind, n_ch, loss):
    base, shape = G.geometry(n_ch)
    data = G.data_for(n_ch)
    assert data.x.shape == (shape[0], n_ch, shape[1], shape[2]) and 0 < int(data.t.sum()) < data.t.numel()
    ref = G.oracle_run(kind, n_ch, data, base, loss=loss, need_dx=True)
    _meaningful(ref, dx=True)
    _conditioned(kind, n_ch, data, ref, loss=loss, need_dx=True)
    _nonzero(ref, G.all_names(kind, n_ch, base))
    assert ref.dx.shape == data.x.shape
    assert all(int(b) == 1 for k, b in ref.bufs.items() if k.endswith("num_batches_tracked"))


def test_dx_cases_are_the_issue_s():
    fp32 = {(k, c) for k, c, p in G.DX_CASES if p == "fp32"}
    assert fp32 == {(k, c) for k in G.KINDS for c in (1, 3, 4, 5, 9, 16)}
    for p in ("bf16", "fp16"):
        assert {(k, c) for k, c, q in G.DX_CASES if q == p} >= {(k, c) for k in G.KINDS for c in (1, 3, 9)}
    assert {(p, c) for _, c, p in G.DX_CASES} == set(G.ROUTES)
    assert G.geometry(9) == (32, (2, 32, 32)) and G.geometry(3) == (8, (2, 32, 48))


@pytest.mark.parametrize("kind", ["unet", "attention"])
def test_freeze_sets(kind):
    names = G.all_names(kind)
    sets = {s: G.freeze_set(s, names) for s in G.FREEZE_SETS}
    cases = {s for k, _, s in G.FREEZE_CASES if k == kind}
    assert cases == {s for s, v in sets.items() if v}, (cases, {s: len(v) for s, v in sets.items()})
    assert cases >= set(G.FREEZE_SETS) - {"gates"} and ("gates" in cases) == (kind == "attention")
    covered = set()
    for s in cases:
        assert set(sets[s]) <= set(names) and len(set(sets[s])) == len(sets[s]) < len(names), s
        covered |= set(sets[s])
    assert covered == set(names), sorted(set(names) - covered)
    m = dict(G.build(kind).named_modules())
    for k in sets["bn_affine"]:
        assert isinstance(m[k.rsplit(".", 1)[0]], torch.nn.BatchNorm2d), k
    for k in sets["conv_weights"]:
        assert isinstance(m[k.rsplit(".", 1)[0]], torch.nn.Conv2d), k
    assert set(sets["bn_affine"]) | set(sets["conv_weights"]) == set(names) - {"outc.conv.bias"}
    assert {(k, p) for k, p, _ in G.FREEZE_CASES} == {(k, p) for k in ("unet", "attention") for p in ("fp32", "bf16")}


@pytest.mark.parametrize("loss", ["linear", "dice_bce"])
@pytest.mark.parametrize("kind", ["unet", "attention"])
def test_all_trainable_reference(kind, loss):
    ref = G.oracle_run(kind, 1, G.data_for(1), loss=loss)
    _meaningful(ref)
    _conditioned(kind, 1, G.data_for(1), ref, loss=loss)
    _nonzero(ref, G.all_names(kind))


@pytest.mark.parametrize("case", list(G.PARTIAL))
def test_partial_output_references(case):
    weights, modules = G.PARTIAL[case]
    names = G.all_names("attention_ds")
    unused = [k for k in names if k.split(".")[0] in modules]
    assert len(weights) == len(G.DS_OUTS) and all(any(k.startswith(mod + ".") for k in names) for mod in modules)
    ref = G.oracle_run("attention_ds", 1, G.data_for(1), weights=weights)
    assert len(ref.outs) == 4
    _meaningful(ref, unused)
    _conditioned("attention_ds", 1, G.data_for(1), ref, weights=weights)
    # a zero weight keeps the output in the graph: its own module's gradient is exactly zero, not missing
    zeroed = {"main": "outc", "ds1": "ds_out1", "ds2": "ds_out2", "ds3": "ds_out3"}
    zero_mods = [zeroed[o] for o, w in zip(G.DS_OUTS, weights) if w == 0.0]
    for k in names:
        if k in unused:
            continue
        if k.split(".")[0] in zero_mods:
            assert float(ref.grads[k].abs().max()) == 0.0, k
        elif not (zero_mods == ["outc"] and k.startswith("up4.")):   # up4 feeds outc alone
            assert float(ref.grads[k].norm()) > 0, k


def test_partial_cases_are_the_issue_s():
    w = {c: v[0] for c, v in G.PARTIAL.items()}
    assert w["main"] == [1.0, None, None, None] and w["main+ds2"] == [1.0, None, 1.0, None]
    assert [w[f"ds{i}"].index(1.0) for i in (1, 2, 3)] == [1, 2, 3]
    assert all(sum(x is None for x in w[f"ds{i}"]) == 3 for i in (1, 2, 3))
    assert any(sorted(map(str, v)) == ["0.0", "1.0", "1.0", "1.0"] for v in w.values())


@pytest.mark.parametrize("kind", ["unet", "attention"])
def test_two_forwards_reference(kind):
    d1, d2 = G.data_for(1), G.data_for(1, second=True)
    assert not torch.equal(d1.x, d2.x)
    ref = G.oracle_run(kind, 1, d1, extra=((d2, 2.0),))
    _meaningful(ref)
    _conditioned(kind, 1, d1, ref, extra=((d2, 2.0),))
    _nonzero(ref, G.all_names(kind))
    assert all(int(b) == 2 for k, b in ref.bufs.items() if k.endswith("num_batches_tracked"))
    # the accumulated gradient is the sum of the two single-forward gradients where BN state does not enter (train
    # mode normalises with batch statistics), and the loss is l1 + 2 l2
    a, b = G.oracle_run(kind, 1, d1), G.oracle_run(kind, 1, d2)
    assert abs(ref.loss - (a.loss + 2 * b.loss)) <= 1e-12 * (1 + abs(ref.loss))
    for k, g in ref.grads.items():
        assert torch.allclose(g, a.grads[k] + 2 * b.grads[k], rtol=1e-9, atol=1e-12 * float(g.abs().max())), k
    one = {k: v for k, v in a.bufs.items() if "running" in k}
    assert any(not torch.equal(ref.bufs[k], v) for k, v in one.items())


@pytest.mark.parametrize("form", G.FORMS)
def test_input_form_conversions(form):
    x = G.data_for(3).x
    leaf, xin = G.input_form(form, x, "cpu")
    assert leaf.is_leaf and leaf.requires_grad and xin.shape == x.shape
    assert form in ("fp16", "fp64") or not xin.is_contiguous()
    xc = xin.float().contiguous()
    assert xc.dtype == torch.float32 and xc.is_contiguous() and xc.requires_grad
    assert torch.equal(xc.detach(), x.half().float() if form == "fp16" else
                       x[:1].expand_as(x) if form == "expand" else x)
    dx = torch.randn(x.shape, generator=torch.Generator().manual_seed(9))
    xc.backward(dx)
    g = leaf.grad
    assert g is not None and g.dtype == leaf.dtype and g.shape == leaf.shape
    if form == "slice":
        assert torch.equal(g[:, :, 1:33, 2:50], dx) and float(g.abs().sum()) == float(dx.abs().sum())
    elif form == "expand":
        assert g.shape[0] == 1 and torch.allclose(g[0], dx.sum(0))
    else:
        assert torch.equal(g, dx.to(leaf.dtype))


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("kind", ["unet", "attention"])
def test_no_grad_train_forward_reference(kind, batch):
    before = dict(G.seeded_buffers(G.build(kind)).named_buffers())
    assert all(int(b) == 3 for k, b in before.items() if k.endswith("num_batches_tracked"))
    assert all(float(b.min()) >= 0.5 for k, b in before.items() if k.endswith("running_var"))
    p = G.oracle_params(G.seeded_buffers(G.build(kind)))
    with torch.no_grad():
        out = G.oracle_forward(kind, p, G.data_for(1).x[:batch].double())[0]
    assert out.shape == (batch, 2, G.H, G.W) and torch.isfinite(out).all() and not out.requires_grad
    for k, b in before.items():
        if k.endswith("num_batches_tracked"):
            assert int(p[k]) == 4
        else:
            assert torch.isfinite(p[k]).all() and not torch.equal(p[k].float(), b), k
