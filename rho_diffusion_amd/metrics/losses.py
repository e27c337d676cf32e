"""rho_diffusion/metrics/losses.py (guided-diffusion's losses) on GPU tensors, float32, through librho_hip.so
(rho_normal_kl, rho_approx_normal_cdf, rho_discretized_gaussian_ll).

Broadcasting is narrower than torch's: each operand is a full tensor, a per-sample ``[B, 1, ..., 1]`` tensor of the same rank,
or a Python scalar; the result has the full shape.  Any other broadcast is refused (RhoHipError)."""
from __future__ import annotations

import numbers

import torch

from .. import hip
from ..engine import ops
from ..hip import RhoHipError

__all__ = ["normal_kl", "approx_standard_normal_cdf", "discretized_gaussian_log_likelihood"]

_FULL, _PER_SAMPLE, _SCALAR = 0, 1, 2


def _operands(fn: str, names, values):
    """(shape, batch, per_sample, [(tensor or None, mode, scalar)]) of the kernel operands."""
    tensors = [(n, v) for n, v in zip(names, values) if isinstance(v, torch.Tensor)]
    if not tensors:
        raise RhoHipError(f"{fn}: at least one argument must be a Tensor (metrics/losses.py:35-40)")
    for n, v in zip(names, values):
        if not isinstance(v, torch.Tensor) and (isinstance(v, bool) or not isinstance(v, numbers.Real)):
            raise RhoHipError(f"{fn}: {n} must be a GPU tensor or a Python scalar, got {type(v).__name__}")
    full = max((v for _, v in tensors), key=lambda v: v.numel()).shape
    if len(full) < 1:
        raise RhoHipError(f"{fn}: 0-dim tensors are not supported; pass a Python scalar")
    batch = int(full[0])
    per_sample = 1
    for d in full[1:]:
        per_sample *= int(d)
    sample_shape = (batch,) + (1,) * (len(full) - 1)
    out = []
    for n, v in zip(names, values):
        if not isinstance(v, torch.Tensor):
            out.append((None, _SCALAR, float(v)))
            continue
        if v.shape == full:
            mode = _FULL
        elif tuple(v.shape) == sample_shape:
            mode = _PER_SAMPLE
        else:
            raise RhoHipError(f"{fn}: {n} has shape {tuple(v.shape)}; supported operands are the full shape {tuple(full)}, the "
                              f"per-sample shape {sample_shape} or a Python scalar (no other broadcast)")
        out.append((v, mode, 0.0))
    for n, v in tensors:
        hip.require_gpu(v, n)
    out = [(v.float().contiguous() if v is not None else None, mode, s) for v, mode, s in out]
    return full, batch, per_sample, out


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL divergence between two Gaussians, elementwise (metrics/losses.py:28-53)."""
    full, batch, per_sample, ops_ = _operands("normal_kl", ("mean1", "logvar1", "mean2", "logvar2"), (mean1, logvar1, mean2, logvar2))
    dev = next(o[0].device for o in ops_ if o[0] is not None)
    out = torch.empty(full, dtype=torch.float32, device=dev)
    return ops.normal_kl(ops_, out, batch, per_sample)


def approx_standard_normal_cdf(x):
    """0.5 * (1 + tanh(sqrt(2/pi) * (x + 0.044715 x^3))) (metrics/losses.py:56-61)."""
    if not isinstance(x, torch.Tensor):
        raise RhoHipError("approx_standard_normal_cdf: x must be a GPU tensor")
    hip.require_gpu(x, "x")
    return ops.approx_normal_cdf(x.float().contiguous())


def discretized_gaussian_log_likelihood(x, *, means, log_scales):
    """Log-likelihood of a Gaussian discretized to 256 bins on [-1, 1], elementwise, in nats (metrics/losses.py:64-93)."""
    full, batch, per_sample, ops_ = _operands("discretized_gaussian_log_likelihood", ("x", "means", "log_scales"), (x, means, log_scales))
    dev = next(o[0].device for o in ops_ if o[0] is not None)
    out = torch.empty(full, dtype=torch.float32, device=dev)
    return ops.discretized_gaussian_ll(ops_, out, batch, per_sample)
