"""rho_diffusion/metrics/geom.py on the device: ``WassersteinWrapper`` is geomloss's ``SamplesLoss("sinkhorn", p=1, blur=0.01)`` over
``flatten(1)`` (metrics/geom.py:28-37).  geomloss is not a dependency: the debiased Sinkhorn divergence with its epsilon-scaling
schedule is restated here (uniform weights, cost |x - y| for p = 1 and |x - y|^2 / 2 for p = 2) and runs as HIP kernels
(csrc/sinkhorn.hip; float32 in and out, the cost sums and the loop in float64), differentiable w.r.t. the first argument.  There is no torch fallback."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import hip
from ..engine import ops
from ..hip import RhoHipError
from ..registry import registry

__all__ = ["epsilon_schedule", "SinkhornDivergence", "WassersteinWrapper"]


def epsilon_schedule(diameter: float, p: int, blur: float, scaling: float) -> List[float]:
    """The temperatures of the epsilon-scaling loop: diameter^p, then a geometric descent by scaling^p down to blur^p (exclusive),
    then blur^p."""
    diameter, blur, scaling = float(diameter), float(blur), float(scaling)
    return ([diameter ** p]
            + [float(np.exp(e)) for e in np.arange(p * math.log(diameter), p * math.log(blur), p * math.log(scaling))]
            + [blur ** p])


class SinkhornDivergence(nn.Module):
    """loss = mean_i(f_ba - f_aa) + mean_j(g_ab - g_bb) of the symmetric Sinkhorn loop between the samples ``pred[i]`` and ``true[j]``
    (each flattened from dim 1), 1 <= batch <= 128.  ``diameter``: the largest distance the schedule starts from; None measures it on
    the device and reads it back (one host sync per call), a number makes the call free of host syncs and capturable in a HIP graph."""

    def __init__(self, p: int = 1, blur: float = 0.01, scaling: float = 0.5, debias: bool = True, diameter: Optional[float] = None):
        super().__init__()
        if p not in (1, 2):
            raise RhoHipError(f"SinkhornDivergence: p must be 1 or 2, got {p}")
        if not blur > 0.0 or not 0.0 < scaling < 1.0:
            raise RhoHipError(f"SinkhornDivergence: blur > 0 and 0 < scaling < 1 are required, got blur = {blur}, scaling = {scaling}")
        if diameter is not None and not diameter >= 0.0:
            raise RhoHipError(f"SinkhornDivergence: diameter must be >= 0, got {diameter}")
        self.p, self.blur, self.scaling, self.debias, self.diameter = int(p), float(blur), float(scaling), bool(debias), diameter
        self._eps_dev = {}          # device -> the fixed schedule of a given diameter

    def _prepare(self, pred: Tensor, true: Tensor) -> Tuple[Tensor, Tensor]:
        if pred.dim() < 2 or true.dim() < 2 or pred[0].numel() != true[0].numel():
            raise RhoHipError(f"SinkhornDivergence: [N, ...] and [M, ...] samples of one size are required, got {tuple(pred.shape)} "
                              f"and {tuple(true.shape)}")
        if not (1 <= pred.shape[0] <= ops.SINKHORN_MAX_SAMPLES and 1 <= true.shape[0] <= ops.SINKHORN_MAX_SAMPLES):
            raise RhoHipError(f"SinkhornDivergence: 1 <= batch <= {ops.SINKHORN_MAX_SAMPLES} samples a side, got {pred.shape[0]} "
                              f"and {true.shape[0]}")
        if true.requires_grad:
            raise RhoHipError("SinkhornDivergence is differentiable w.r.t. its first argument only: true.requires_grad must be False")
        hip.require_gpu(pred, "pred")
        hip.require_gpu(true, "true")
        return pred.flatten(1).float().contiguous(), true.flatten(1).float().contiguous()

    def _eps_list(self, x: Tensor, y: Tensor) -> Optional[Tensor]:
        """The schedule as a device tensor; None when every row of [x; y] is the same point."""
        if self.diameter is not None:
            if self.diameter == 0.0:
                return None
            eps = self._eps_dev.get(x.device)
            if eps is None:
                eps = torch.tensor(epsilon_schedule(self.diameter, self.p, self.blur, self.scaling), dtype=torch.float64, device=x.device)
                self._eps_dev[x.device] = eps
            return eps
        diameter = float(ops.max_diameter(x, y).item())
        if diameter == 0.0:
            return None
        return torch.tensor(epsilon_schedule(diameter, self.p, self.blur, self.scaling), dtype=torch.float64, device=x.device)

    def forward(self, pred: Tensor, true: Tensor) -> Tensor:
        assert pred.shape == true.shape
        return self.samples_loss(pred, true)

    def samples_loss(self, pred: Tensor, true: Tensor) -> Tensor:
        """``forward`` without the equal-shape assertion of the reference's wrapper: N samples against M of the same size."""
        from ..autograd import sinkhorn_loss
        x, y = self._prepare(pred, true)
        eps = self._eps_list(x, y)
        if eps is None:
            return (x * 0.0).sum()          # all samples equal: loss 0, gradient 0
        return sinkhorn_loss(x, y, eps, self.p, self.debias)

    def potentials(self, pred: Tensor, true: Tensor) -> Tuple[Tensor, Tensor]:
        """(f_ba - f_aa [N], g_ab - g_bb [M]): the dual potentials whose means add up to the loss."""
        x, y = self._prepare(pred.detach(), true.detach())
        eps = self._eps_list(x, y)
        if eps is None:
            return x.new_zeros(x.shape[0]), y.new_zeros(y.shape[0])
        out = ops.sinkhorn_loop(*ops.pairwise_cost(x, y, self.p, dtype=torch.float64), eps, self.p, self.debias)
        return out["f_ba"] - out["f_aa"], out["g_ab"] - out["g_bb"]


@registry.register_layer("WassersteinWrapper")
class WassersteinWrapper(SinkhornDivergence):
    """metrics/geom.py:28-37: ``SamplesLoss("sinkhorn", p=1, blur=0.01)`` of the flattened samples (geomloss's defaults otherwise:
    scaling 0.5, debiased)."""

    def __init__(self, *args, **kwargs) -> None:
        super().__init__(p=1, blur=0.01, scaling=0.5, debias=True, diameter=kwargs.pop("diameter", None))

    def forward(self, pred_data: Tensor, true_data: Tensor) -> Tensor:
        return super().forward(pred_data, true_data)
