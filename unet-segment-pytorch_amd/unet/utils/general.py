"""General training utilities with the reference's API (unet/utils/general.py of seagochen/unet-segment-pytorch),
so that `from unet.utils.general import set_seed, get_device, load_config, increment_path, ModelEMA`
(scripts/train.py:33) resolves against this package.

`ModelEMA.update` is the device part: the reference walks the parameters and buffers in Python (`mul_` + `add_` per
parameter, `copy_` per buffer: 274 launches for AttentionUNet); here it is one `unet_ema_update` launch over a
segment table built once (csrc/optim.hip).  The other helpers are short host utilities.
"""

from __future__ import annotations

import copy
import random
from itertools import chain
from pathlib import Path
from typing import Union

import numpy as np
import torch

from .._hip import lib as L
from .._hip.runtime import require_device, stream, vp
from .config import load_config  # noqa: F401  (re-export: the reference keeps load_config here)
from .optim import aligned16, build_chunk_map, upload


def set_seed(seed: int = 42) -> None:
    """Seed Python's, numpy's and torch's generators (every GPU's too)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def get_device(device: str = "") -> torch.device:
    """`device` if given, else the GPU when one is visible, else the CPU."""
    if device:
        return torch.device(device)
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def increment_path(path: Union[str, Path], exist_ok: bool = False) -> Path:
    """`path` if it is free (or `exist_ok`), else the first free one of path2, path3, ... (the number goes before
    the suffix)."""
    path = Path(path)
    if exist_ok or not path.exists():
        return path
    for n in range(2, 1000):
        candidate = path.with_name(f"{path.stem}{n}{path.suffix}")
        if not candidate.exists():
            return candidate
    raise RuntimeError(f"no free path next to {path}")


class ModelEMA:
    """Exponential moving average of a model's parameters, with its buffers copied (BatchNorm running statistics and
    counters).  `ema_model` is a deep copy in eval mode whose parameters take no gradient.

    `update(model)`: updates += 1; d = decay, or min(decay, (1 + updates) / (10 + updates)) during the first
    `warmup_steps` updates; every parameter of `ema_model` whose name the model has becomes d * ema + (1 - d) *
    model's, every such buffer a copy.  One launch, no host synchronise.  The table of tensor addresses is built on
    the first update and again whenever a tensor of either model moves; `ema_model.load_state_dict` copies in place
    and keeps it.  Parameters must be contiguous fp32 on the GPU (an error otherwise, no fallback)."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.999, warmup_steps: int = 0):
        self.decay = decay
        self.warmup_steps = warmup_steps
        self.updates = 0
        self.ema_model = copy.deepcopy(model)
        self.ema_model.eval()
        for p in self.ema_model.parameters():
            p.requires_grad_(False)
        self._root = self._key = None
        self._segs = self._map = None
        self._nchunks = 0

    def _snapshot(self, model):
        """The module trees of both models, flattened once: walking them (`parameters()` builds every name) costs
        more host time per update than the launch.  The modules are kept alive, so their ids stay theirs."""
        self._root = model
        self._mods = [m for root in (model, self.ema_model) for m in root.modules()]
        self._dicts = [d for m in self._mods for d in (m._parameters, m._buffers)]
        self._kids = [m._modules for m in self._mods]

    def _current_key(self):
        """children of every module (a replaced submodule changes it) and the address of every tensor"""
        return ([id(c) for d in self._kids for c in d.values()],
                [t.data_ptr() for d in self._dicts for t in d.values() if t is not None])

    def _build(self, model):
        src_p, src_b = dict(model.named_parameters()), dict(model.named_buffers())
        rows, numels = [], []
        for name, e in self.ema_model.named_parameters():
            p = src_p.get(name)
            if p is None:
                continue
            require_device(e, f"EMA parameter '{name}'")
            if e.dtype != torch.float32 or p.dtype != torch.float32 or p.device != e.device or p.shape != e.shape \
                    or not p.is_contiguous() or not e.is_contiguous():
                raise RuntimeError(f"ModelEMA: parameter '{name}' must be contiguous fp32 of one shape on one device "
                                   f"in both models ({p.dtype} {tuple(p.shape)} on {p.device} / {e.dtype} "
                                   f"{tuple(e.shape)} on {e.device}); there is no fallback path")
            ptrs = (e.data_ptr(), p.data_ptr())
            rows.append((*ptrs, 0, 0, 0, e.numel(), 0, L.OPT_EMA | (L.OPT_ALIGNED if aligned16(*ptrs) else 0)))
            numels.append(e.numel())
        for name, e in self.ema_model.named_buffers():
            b = src_b.get(name)
            if b is None:
                continue
            require_device(e, f"EMA buffer '{name}'")
            if e.dtype != b.dtype or b.device != e.device or b.shape != e.shape or not b.is_contiguous() \
                    or not e.is_contiguous():
                raise RuntimeError(f"ModelEMA: buffer '{name}' must be contiguous with one dtype, shape and device in "
                                   f"both models; there is no fallback path")
            nbytes = e.numel() * e.element_size()
            ptrs = (e.data_ptr(), b.data_ptr())
            rows.append((*ptrs, 0, 0, 0, nbytes, 0, L.OPT_COPY | (L.OPT_ALIGNED if aligned16(*ptrs) else 0)))
            numels.append(-(-nbytes // 4))     # a chunk of a COPY segment is 4 * CHUNK bytes
        if not rows:
            self._nchunks = 0
            return
        dev = next(chain(self.ema_model.parameters(), self.ema_model.buffers())).device
        self._segs = upload(np.array(rows, dtype=np.dtype(L.OptimSeg)), self._segs, dev)
        cmap = build_chunk_map(numels)
        self._map = upload(cmap, self._map, dev)
        self._nchunks = len(cmap)

    @torch.no_grad()
    def update(self, model: torch.nn.Module) -> None:
        self.updates += 1
        d = self.decay
        if self.updates <= self.warmup_steps:
            d = min(d, (1 + self.updates) / (10 + self.updates))
        if model is not self._root or self._current_key() != self._key:
            self._snapshot(model)
            self._build(model)
            self._key = self._current_key()
        if self._nchunks:
            L.call("unet_ema_update", vp(self._segs), vp(self._map), self._nchunks, d, 1 - d, stream())

    def state_dict(self) -> dict:
        return {"ema_state_dict": self.ema_model.state_dict(), "decay": self.decay, "updates": self.updates}

    def load_state_dict(self, state_dict: dict) -> None:
        self.ema_model.load_state_dict(state_dict["ema_state_dict"])
        self.decay = state_dict.get("decay", self.decay)
        self.updates = state_dict.get("updates", 0)
