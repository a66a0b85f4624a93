"""CPU: descriptors of the first conv with 5 to 16 fp32 NCHW input channels route to csrc/stem.hip, and their
neighbours keep the routes they had.  The route queries launch nothing."""

import ctypes

import pytest

import conv_cases as CC


@pytest.fixture(scope="module")
def lib():
    from unet._hip import lib as L
    assert L.library_path().exists(), "libunet_hip.so not built (run __graft_entry__.build())"
    return L, L.load()


def _names(lib, dt, cin, cout, k=3):
    L, so = lib
    c = CC.conv("q", dt, k, (2, 40, 70), [CC.S("nchw", cin)], cout, "", stats=1)
    g = CC.wgrad("q", dt, k, (2, 40, 70), [CC.S("nchw", cin)], cout, "")
    dc, dg = CC.conv_desc(L, c), CC.wgrad_desc(L, g)
    return (CC.variant_of(so, dc), so.unet_conv_stats_rows(ctypes.byref(dc)), CC.variant_of(so, dg, True),
            so.unet_wgrad_workspace(ctypes.byref(dg)))


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("cin", [5, 16])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_stem_routes(lib, monkeypatch, dt, cin, cout):
    monkeypatch.delenv("UNET_STEM_MFMA", raising=False)
    fwd, rows, wg, ws = _names(lib, dt, cin, cout)
    assert fwd == f"stem_fwd_mfma_kernel<{dt},{cout}>" and wg == f"stem_wgrad_mfma_kernel<{dt},{cout}>", (fwd, wg)
    assert rows > 0 and ws > 0, (rows, ws)
    monkeypatch.setenv("UNET_STEM_MFMA", "0")
    assert _names(lib, dt, cin, cout)[::2] == (f"conv_generic_kernel<{dt},3,{cout}>", f"wgrad_kernel<{dt},3>")


@pytest.mark.parametrize("dt,cin,cout,k,fwd,wg", [
    ("bf16", 4, 64, 3, "smallcin_fwd_kernel<bf16>", "smallcin_wgrad_kernel<bf16>"),
    ("bf16", 17, 64, 3, "conv_generic_kernel<bf16,3,64>", "wgrad_kernel<bf16,3>"),
    ("fp16", 6, 16, 3, "conv_generic_kernel<fp16,3,32>", "wgrad_kernel<fp16,3>"),
    ("bf16", 6, 40, 3, "conv_generic_kernel<bf16,3,64>", "wgrad_kernel<bf16,3>"),
    ("fp16", 9, 128, 3, "conv_generic_kernel<fp16,3,64>", "wgrad_kernel<fp16,3>"),
    ("fp32", 9, 64, 3, "conv_generic_kernel<fp32,3,64>", "wgrad_kernel<fp32,3>"),
    ("bf16", 9, 64, 1, "conv_generic_kernel<bf16,1,64>", "wgrad_kernel<bf16,1>"),
])
def test_neighbours_keep_their_routes(lib, monkeypatch, dt, cin, cout, k, fwd, wg):
    monkeypatch.delenv("UNET_STEM_MFMA", raising=False)
    monkeypatch.delenv("UNET_SMALLCIN_MFMA", raising=False)
    assert _names(lib, dt, cin, cout, k)[::2] == (fwd, wg)
