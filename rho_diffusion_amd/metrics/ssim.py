"""``StructuralSimilarityIndexMeasure``: the structural metric of torchmetrics, the package the reference's pipelines take their
metrics from (abstract_diffusion.py:31,79), as one fused HIP kernel (rho_ssim) for fields with 1, 2 or 3 spatial dimensions.

Three differences from torchmetrics' class.  ``return_map`` gives the index over the windows that lie wholly inside the field,
[B, C, *(size_d - k_d + 1)], not torchmetrics' ``return_full_image`` (its reflection-padded map); the reduced value is the same,
since torchmetrics crops its padding again before it reduces.  The kernel forms the second moments on data shifted by
``target[b, c, 0, .., 0]`` (the float32 sums of the plain form cancel for a small contrast on a large offset).  Each call stands
alone: the running state over calls (``update`` / ``compute``) is not reproduced."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from .. import hip
from ..engine import ops
from ..hip import RhoHipError

__all__ = ["StructuralSimilarityIndexMeasure", "ssim_window"]

REDUCTIONS = ("elementwise_mean", "sum", "none", None)


def ssim_window(gaussian_kernel: bool, sigma: float, kernel_size: int) -> np.ndarray:
    """One dimension's window as float32.  Gaussian: k = 2 int(3.5 sigma + 0.5) + 1 taps (``kernel_size`` is ignored, as torchmetrics
    does), g[j] = exp(-((j - (k - 1) / 2) / sigma)^2 / 2) normalised to sum 1, evaluated in float64 and rounded once.  Otherwise
    1 / k.  Both arguments are judged in either mode."""
    if not sigma > 0.0:
        raise RhoHipError(f"StructuralSimilarityIndexMeasure: sigma must be > 0, got {sigma}")
    if int(kernel_size) != kernel_size or kernel_size < 1 or kernel_size % 2 == 0:
        raise RhoHipError(f"StructuralSimilarityIndexMeasure: kernel_size must be odd and positive, got {kernel_size}")
    if gaussian_kernel:
        k = 2 * int(3.5 * sigma + 0.5) + 1
        x = (np.arange(k, dtype=np.float64) - (k - 1) / 2.0) / float(sigma)
        g = np.exp(-0.5 * x * x)
        g /= g.sum()
    else:
        g = np.full(int(kernel_size), 1.0 / int(kernel_size), dtype=np.float64)
    if len(g) > ops.SSIM_MAX_WINDOW:
        raise RhoHipError(f"StructuralSimilarityIndexMeasure: a window of {len(g)} taps exceeds the kernel's {ops.SSIM_MAX_WINDOW}")
    return g.astype(np.float32)


def _per_dim(value, nd: int, name: str) -> list:
    if isinstance(value, (list, tuple)):
        if len(value) != nd:
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: {name} has {len(value)} values for {nd} spatial dimensions")
        return list(value)
    return [value] * nd


class StructuralSimilarityIndexMeasure(nn.Module):
    """SSIM of ``preds`` against ``target`` [B, C, *spatial] (1 to 3 spatial dimensions) as a float32 GPU tensor: 0-dim for
    ``reduction`` "elementwise_mean" (mean over the batch) and "sum", [B] for "none" / None; the per-sample value is the mean of the
    index over the channels and windows of that sample.  ``sigma`` / ``kernel_size``: a scalar or one value per spatial dimension.
    ``data_range``: None (the larger extent of the two inputs, measured on the device), a float, or (lo, hi): both inputs are clamped.
    ``return_map``: also return the index itself, [B, C, *(size_d - k_d + 1)] - the valid windows only, not torchmetrics' padded
    ``return_full_image``."""

    def __init__(self, gaussian_kernel: bool = True, sigma: Union[float, Sequence[float]] = 1.5,
                 kernel_size: Union[int, Sequence[int]] = 11, reduction: Optional[str] = "elementwise_mean",
                 data_range: Union[None, float, Tuple[float, float]] = None, k1: float = 0.01, k2: float = 0.03,
                 return_map: bool = False):
        super().__init__()
        if reduction not in REDUCTIONS:
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: reduction must be one of {REDUCTIONS}, got {reduction!r}")
        self.clamp: Optional[Tuple[float, float]] = None
        if isinstance(data_range, (tuple, list)):
            if len(data_range) != 2 or not float(data_range[1]) > float(data_range[0]):
                raise RhoHipError(f"StructuralSimilarityIndexMeasure: data_range (lo, hi) needs hi > lo, got {data_range}")
            self.clamp = (float(data_range[0]), float(data_range[1]))
            self.range: Optional[float] = self.clamp[1] - self.clamp[0]
        elif data_range is not None:
            if not data_range > 0.0:
                raise RhoHipError(f"StructuralSimilarityIndexMeasure: data_range must be > 0, got {data_range}")
            self.range = float(data_range)
        else:
            self.range = None
        self.gaussian_kernel, self.sigma, self.kernel_size = bool(gaussian_kernel), sigma, kernel_size
        self.reduction, self.data_range, self.k1, self.k2, self.return_map = reduction, data_range, float(k1), float(k2), bool(return_map)
        lengths = {len(v) for v in (sigma, kernel_size) if isinstance(v, (list, tuple))}
        if len(lengths) > 1 or (lengths and not 1 <= min(lengths) <= 3):
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: sigma {sigma} and kernel_size {kernel_size} must name the same 1 to 3 "
                              "spatial dimensions")
        self.windows(lengths.pop() if lengths else 1)          # judged now, not at the first call
        self._cache: Dict[Tuple[str, int], List[Tensor]] = {}

    def windows(self, nd: int) -> List[np.ndarray]:
        """The float32 window of each of ``nd`` spatial dimensions."""
        sig, ks = _per_dim(self.sigma, nd, "sigma"), _per_dim(self.kernel_size, nd, "kernel_size")
        return [ssim_window(self.gaussian_kernel, s, k) for s, k in zip(sig, ks)]

    def _device_windows(self, device: torch.device, nd: int) -> List[Tensor]:
        key = (str(device), nd)
        if key not in self._cache:
            self._cache[key] = [torch.from_numpy(w).to(device) for w in self.windows(nd)]
        return self._cache[key]

    @torch.no_grad()
    def forward(self, preds: Tensor, target: Tensor):
        if preds.shape != target.shape:
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
        if not 3 <= preds.dim() <= 5:
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: inputs must be [B, C, *spatial] with 1 to 3 spatial dimensions, got "
                              f"{tuple(preds.shape)}")
        nd = preds.dim() - 2
        wins = self.windows(nd)
        for size, w in zip(preds.shape[2:], wins):
            if size < len(w):
                raise RhoHipError(f"StructuralSimilarityIndexMeasure: a spatial size of {size} is below its window of {len(w)} taps")
        if preds.shape[0] < 1 or preds.shape[1] < 1:
            raise RhoHipError(f"StructuralSimilarityIndexMeasure: empty input {tuple(preds.shape)}")
        hip.require_gpu(preds, "preds")
        hip.require_gpu(target, "target")
        per_sample, out, smap = ops.ssim(preds.float().contiguous(), target.float().contiguous(), self._device_windows(preds.device, nd),
                                         self.range, self.clamp, self.k1, self.k2, self.return_map)
        value = out[0] if self.reduction == "elementwise_mean" else out[1] if self.reduction == "sum" else per_sample
        return (value, smap) if self.return_map else value
