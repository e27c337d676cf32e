"""Dtype-generic form of the VisionTransformer restatement tests/vit_ref.py (TEST INFRASTRUCTURE), the counterpart of
tests/unet_ref64.py.

``vit_ref.Sinusoid`` is float32 by construction (``.float()``, the frequencies in the default dtype), so ``VitRef(...).double()`` stops
at the first Linear behind a sinusoid.  ``build(kwargs, state_dict, dtype)`` returns ``vit_ref.VitRef`` itself - the same modules, the
same forward - cast to ``dtype``, with its sinusoids replaced by the one below, in which every ``.float()`` is a ``.to(dtype)``.  At
``torch.float32`` that issues the same torch ops in the same order as ``vit_ref`` (tests/test_vit_sweep_host.py requires
``torch.equal`` on the prediction, on every parameter gradient and on the input gradient): this pins the twin to ``vit_ref``, which the
g23 / g25 digests pin to the reference.  At ``torch.float64`` everything, both sinusoids included (exponent, power, quotient, sin / cos),
is evaluated in float64: the reference the whole-ViT GPU tests compare with."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import vit_ref

INPUT = "<input>"


class Sinusoid(vit_ref.Sinusoid):
    """vit_ref.Sinusoid: interleaved sin / cos of t / wavelength^(2i / dim), exponent, power, quotient and sin / cos in ``dtype``."""

    def __init__(self, dim, dtype, wavelength=10000):
        super().__init__(dim, wavelength)
        self.dtype = dtype

    def forward(self, t):
        w = torch.pow(self.wavelength, (2 * torch.arange(self.dim // 2, device=t.device)).to(self.dtype) / self.dim)
        a = t.reshape(-1, 1).to(self.dtype) / w
        return torch.stack([a.sin(), a.cos()], dim=-1).reshape(t.numel(), self.dim)


def build(kwargs: dict, state_dict: dict, dtype=torch.float64) -> vit_ref.VitRef:
    m = vit_ref.build(kwargs, state_dict).to(dtype)
    for seq in [m.pos_embedding] + [blk.time_transform for blk in m.transformer_blocks]:
        seq[0] = Sinusoid(seq[0].dim, dtype, seq[0].wavelength)
    return m


def loss_and_grads(model: vit_ref.VitRef, x: torch.Tensor, t: torch.Tensor, target: torch.Tensor):
    """(prediction, mse loss, {name: gradient}) of a restatement (``vit_ref.build`` or this module's ``build``) in the dtype of its
    parameters; the gradient of the loss by the input goes under ``INPUT``."""
    dtype = next(model.parameters()).dtype
    model.zero_grad(set_to_none=True)
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    pred = model(xr, t)
    loss = F.mse_loss(pred, target.to(dtype))
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for k, p in model.named_parameters()}
    grads[INPUT] = xr.grad.detach()
    return pred.detach(), loss.detach(), grads
