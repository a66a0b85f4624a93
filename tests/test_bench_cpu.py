"""bench.py's --dump-outputs writer on CPU tensors: the arrays it names, float32, whole where they fit and the same
seeded sample in every call where they do not."""

import numpy as np
import torch


def _case():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(1, 3, 3), torch.nn.BatchNorm2d(3))
    return m, torch.tensor(0.25, dtype=torch.float64), torch.randn(2, 2, 5, 7).bfloat16()


def test_dump_outputs_arrays(tmp_path):
    import bench
    m, loss, logits = _case()
    shapes = bench.dump_outputs(str(tmp_path / "a" / "b"), loss, logits, m)
    got = {p.stem: np.load(p) for p in (tmp_path / "a" / "b").glob("*.npy")}
    assert set(got) == {"loss", "logits", "params", "buffers"} == set(shapes)
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [0.25]
    assert got["logits"].shape == (2, 2, 5, 7) and np.array_equal(got["logits"], logits.float().numpy())
    want = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy()
    assert np.array_equal(got["params"], want)
    assert got["buffers"].shape == (3 + 3 + 1,)          # running mean, running var, num_batches_tracked
    assert all(list(got[k].shape) == shapes[k] for k in got)


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 16)
    m, loss, logits = _case()
    bench.dump_outputs(str(tmp_path / "r1"), loss, logits, m)
    bench.dump_outputs(str(tmp_path / "r2"), loss, logits, m)
    for name in ("loss", "logits", "params", "buffers"):
        a, b = np.load(tmp_path / "r1" / f"{name}.npy"), np.load(tmp_path / "r2" / f"{name}.npy")
        assert np.array_equal(a, b) and a.size <= 16
    a = np.load(tmp_path / "r1" / "logits.npy")
    assert a.shape == (16,) and np.isin(a, logits.float().numpy()).all()
    assert np.load(tmp_path / "r1" / "buffers.npy").shape == (7,)
