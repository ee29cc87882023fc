"""`SepformerSeparator`: drop-in for the `self.separator` object of the reference
(SepformerSeparation.from_hparams at /root/reference/back/api.py:713-717; called at 1077 as
`separated = self.separator.separate_batch(subsegment)` with a [1, T] tensor, result indexed
`separated[..., idx]`).  All arithmetic runs in libccx (csrc/sepformer.hip).

The reference loads the two-speaker model; `SepDims.n_spk` in [1, 4] builds the same network with a mask head of `128 * n_spk`
rows (the layout of the 3-mix sibling checkpoint), and `separate_batch` then returns that many sources."""
from __future__ import annotations

import ctypes as C
from dataclasses import asdict
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from .weights import DualPathDims, SepDims


class _Separator:
    """What both separator families share: the context and the libccx handle, staging every tensor and finalizing (the handle is
    destroyed if either raises), `close` and `separate_batch`.  A subclass names its family (`_c` + `_create`, `_set_tensor`,
    `_finalize`, `_destroy`, `_separate` are libccx's entry points), its ctypes dims struct and its default capacity."""
    _c: str
    _cdims: type

    def __init__(self, dims, state_dict: Dict[str, torch.Tensor], max_tokens: int, max_utts: int, device: int, ctx: Optional[_lib.Context]):
        if not torch.cuda.is_available():
            raise _lib.CcxError(f"{type(self).__name__} needs a ROCm GPU: the HIP path has no CPU fallback")
        self.dims = dims
        self.n_spk = int(dims.n_spk)            # sources per utterance: the last axis of separate_batch's result
        self.max_tokens, self.max_utts = int(max_tokens) // dims.segment * dims.segment, int(max_utts)
        self.device = torch.device("cuda", device)
        self.ctx = ctx or _lib.Context(device)
        self.lib = self.ctx.lib
        h = C.c_void_p()
        cd = self._cdims(**asdict(dims))
        self.ctx.check(self._fn("create")(self.ctx.handle, C.byref(cd), int(max_tokens), int(max_utts), C.byref(h)), f"{self._c}_create")
        self.handle = h
        try:
            for name, t in state_dict.items():
                t = t.detach().to("cpu", torch.float32).contiguous()
                self.ctx.check(self._fn("set_tensor")(self.handle, name.encode(), t.data_ptr(), t.numel()), f"set_tensor({name})")
            self.ctx.check(self._fn("finalize")(self.handle), f"{self._c}_finalize")
        except Exception:
            self.close()
            raise

    def _fn(self, name: str):
        return getattr(self.lib, f"{self._c}_{name}")

    def close(self):
        if getattr(self, "handle", None):
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def separate_batch(self, mix: torch.Tensor, n_samples: Optional[Sequence[int]] = None) -> torch.Tensor:
        """mix [B, T] -> [B, T, n_spk] (2 for the default geometries).  Rows are independent utterances; `n_samples` gives their true
        lengths when the batch is ragged (zero padded to T); every source is zero past an utterance's length."""
        if mix.dim() == 1:
            mix = mix.unsqueeze(0)
        x = mix.to(self.device, torch.float32).contiguous()
        B, T = x.shape
        ns = (C.c_int * B)(*([T] * B if n_samples is None else [int(v) for v in n_samples]))
        out = torch.empty(B, T, self.n_spk, device=self.device, dtype=torch.float32)
        self.ctx.check(self._fn("separate")(self.handle, x.data_ptr(), T, ns, B, out.data_ptr(), _lib.current_stream_ptr()),
                       f"{self._c}_separate")
        return out


class SepformerSeparator(_Separator):
    _c, _cdims = "ccx_sepformer", _lib.SepformerDims

    def __init__(self, dims: SepDims, state_dict: Dict[str, torch.Tensor], max_tokens: int = 160_000, max_utts: int = 64,
                 device: int = 0, ctx: Optional[_lib.Context] = None):
        super().__init__(dims, state_dict, max_tokens, max_utts, device, ctx)

    def tokens_for(self, n_samples: int) -> int:
        """Encoder frames of one utterance after padding to whole chunks (capacity accounting)."""
        d = self.dims
        L = (int(n_samples) - d.kernel) // d.stride + 1
        return (L + (d.segment - L % d.segment))


class DualPathSeparator(_Separator):
    """The dual-path SepFormer (the published `sepformer-*` checkpoints: 256 filters, 8 heads of 32, chunks of K at 50 % overlap, an
    intra- and an inter-chunk transformer per block, a gated output) behind the surface of `SepformerSeparator`.  All arithmetic runs
    in libccx (csrc/dualpath.hip); semantics restated from recollection, parity unpinned (tests/dualpath_reference.py)."""
    _c, _cdims = "ccx_dualpath", _lib.DualPathDims

    def __init__(self, dims: DualPathDims, state_dict: Dict[str, torch.Tensor], max_tokens: int = 64_000, max_utts: int = 64,
                 device: int = 0, ctx: Optional[_lib.Context] = None):
        super().__init__(dims, state_dict, max_tokens, max_utts, device, ctx)

    def tokens_for(self, n_samples: int) -> int:
        """Chunk rows of one utterance, S * K (capacity accounting)."""
        d = self.dims
        L = (int(n_samples) - d.kernel) // d.stride + 1
        K, P = d.segment, d.segment // 2
        gap = K - (P + L % K) % K
        return 2 * (L + gap + P) // K * K
