"""``Baseline``: the model-free rows of a super-resolution table as a module for the model slot of the drivers.

``predict_images``, ``predict_sheet``, ``predict_collage`` and ``test_metrics`` score ``Baseline(scale)`` through exactly the code that
scores a network: it has no engine, so it takes the drivers' path for arbitrary ``nn.Module``s (the loop that calls ``model(lr)``), never
the captured replay of the ResUNet family."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .data import _slice_center


class Baseline(nn.Module):
    r"""``forward(lr)``: the centre ``channels`` planes of ``lr`` [N, n_frames * channels, h, w] (float on the 0 .. 255 scale as the
    drivers hand it to a model, or uint8), rounded half to even and clipped to uint8 (exact for what the datasets produce), optionally
    denoised by non-local means (``denoise``: ``None`` or a dict of ``util.nlm_denoise``'s keywords ``h`` (required), ``sigma``,
    ``patch_radius``, ``search_radius``), then enlarged ``scale`` times exactly as Pillow's 8-bit ``Image.resize`` does with ``filter``
    (``"bicubic"`` or ``"bilinear"``).  Returns float32 [N, channels, h scale, w scale] on the 0 .. 255 scale holding those integers, so
    the drivers' truncation gives back the kernels' bytes.  Two launches at most (``pssr_nlm_u8``, ``pssr_upsample_u8``); no
    parameters: ``state_dict()`` is empty.  A host input raises the package's ``RuntimeError``."""

    def __init__(self, scale: int = 4, channels: int = 1, *, filter: str = "bicubic", denoise=None):
        super().__init__()
        from .util import _check_nlm, _check_upsample
        self.scale = _check_upsample(scale, filter)
        if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
            raise ValueError(f"channels must be a positive int (the planes of the output). Given {channels!r}.")
        self.channels = channels
        self.filter = filter
        self._nlm = None
        if denoise is not None:
            if not isinstance(denoise, dict) or "h" not in denoise or set(denoise) - {"h", "sigma", "patch_radius", "search_radius"}:
                raise ValueError("denoise must be None or a dict of nlm_denoise's keywords h (required), sigma, patch_radius, search_radius. "
                                 f"Given {denoise!r}.")
            self._nlm = _check_nlm(denoise["h"], denoise.get("sigma", 0.0), denoise.get("patch_radius", 2), denoise.get("search_radius", 7))
        self.denoise = None if denoise is None else dict(denoise)

    def extra_repr(self):
        return f"scale={self.scale}, channels={self.channels}, filter={self.filter!r}, denoise={self.denoise!r}"

    def forward(self, lr):
        if not torch.is_tensor(lr) or not lr.is_cuda:
            raise RuntimeError("pssr2_amd.baselines.Baseline runs on an MI355X (HIP) device only; there is no CPU fallback")
        if lr.dim() != 4 or lr.shape[1] < self.channels:
            raise ValueError(f"Baseline takes [N, frames, h, w] with at least channels = {self.channels} frames. Its input's shape is {tuple(lr.shape)}.")
        x = _slice_center(lr.detach(), self.channels)
        if x.dtype != torch.uint8:
            x = torch.round(x.float()).clamp_(0, 255).to(torch.uint8)
        if self._nlm is not None:
            x = ops.nlm_u8(x, *self._nlm)
        return ops.upsample_u8(x, self.scale, self.filter).float()
