"""``PeakSignalNoiseRatio``: the metric the reference's pipelines carry (abstract_diffusion.py:79, torchmetrics' class there), as one
fused HIP reduction (rho_psnr).  Each call stands alone: torchmetrics' running state over calls (``update`` / ``compute``) is not
reproduced."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .. import hip
from ..engine import ops
from ..hip import RhoHipError

__all__ = ["PeakSignalNoiseRatio"]


class PeakSignalNoiseRatio(nn.Module):
    """10 log10(data_range^2 / mse(preds, target)) as a 0-dim float32 GPU tensor; ``data_range`` None: max - min of ``target``."""

    def __init__(self, data_range: Optional[float] = None):
        super().__init__()
        if data_range is not None and not data_range > 0.0:
            raise RhoHipError(f"PeakSignalNoiseRatio: data_range must be > 0, got {data_range}")
        self.data_range = data_range

    @torch.no_grad()
    def forward(self, preds: Tensor, target: Tensor) -> Tensor:
        if preds.shape != target.shape:
            raise RhoHipError(f"PeakSignalNoiseRatio: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
        hip.require_gpu(preds, "preds")
        hip.require_gpu(target, "target")
        return ops.psnr(preds.float().contiguous(), target.float().contiguous(), self.data_range)[0]
