"""torch.autograd glue: the UNet forward/backward run in the HIP engine, autograd only carries the
gradient of the prediction in and out.  Parameter gradients are accumulated by the kernels directly
into ``p.grad`` (so ``loss.backward(); optimizer.step()`` behaves as with stock autograd), which is why
the Function returns None for them."""
from __future__ import annotations

from typing import Callable, List, Optional

import torch
from torch import nn

from .engine import ops


class UNetFunction(torch.autograd.Function):
    """pred = UNet(x, t, y).  ``anchor`` is any parameter that requires grad: it only makes autograd call
    ``backward``; ``hooks`` is an optional object with ``on_ready(params)`` for gradient all-reduce overlap."""

    @staticmethod
    def forward(ctx, x, anchor, engine, timesteps, y, hooks):
        ctx.engine = engine
        ctx.hooks = hooks
        out = engine.forward(x, timesteps, y, train=True)
        ctx.generation = engine._train_generation      # this forward's number: backward refuses to run for an older one
        return out.clone()

    @staticmethod
    def backward(ctx, dout):
        cb = ctx.hooks.on_ready if ctx.hooks is not None else None
        ctx.engine.backward(dout.contiguous().float(), on_ready=cb, generation=ctx.generation)
        return None, None, None, None, None, None


class MSELossFunction(torch.autograd.Function):
    """mean((pred - target)^2) with the HIP reduction kernel (nn.MSELoss at ddpm.py:280)."""

    @staticmethod
    def forward(ctx, pred, target):
        loss, grad = ops.mse(pred.contiguous().float(), target.contiguous().float(), want_grad=True)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        # g is the scalar upstream gradient (1.0 for loss.backward()); applied on the device, no host sync
        from . import hip
        gs = g.reshape(1).float().contiguous()
        hip.check(hip.lib().rho_scale_by_device_scalar(grad.data_ptr(), gs.data_ptr(), grad.numel(), hip.stream()),
                  "rho_scale_by_device_scalar")
        return grad, None


def mse_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return MSELossFunction.apply(pred, target)


class PredLossFunction(torch.autograd.Function):
    """sum_b w[t_b] sum_i (pred - target)^2 / n for a backbone that predicts the noise, v or x0 (``pred_type`` 0 / 1 / 2), the target
    formed from (x0, noise, t) inside the kernel (rho_pred_loss_ws); ``w`` None weighs every timestep 1.  Only ``pred`` receives a
    gradient."""

    @staticmethod
    def forward(ctx, pred, x0, noise, t, alpha_bar, w, pred_type, err_flag):
        loss, grad = ops.pred_loss(pred.contiguous().float(), x0.contiguous().float(), noise.contiguous().float(), t, alpha_bar, w,
                                   pred_type, want_grad=True, err_flag=err_flag)
        ctx.save_for_backward(grad)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        # the scalar upstream gradient is applied on the device, as in MSELossFunction
        from . import hip
        gs = g.reshape(1).float().contiguous()
        hip.check(hip.lib().rho_scale_by_device_scalar(grad.data_ptr(), gs.data_ptr(), grad.numel(), hip.stream()),
                  "rho_scale_by_device_scalar")
        return grad, None, None, None, None, None, None, None


def pred_loss(pred: torch.Tensor, x0: torch.Tensor, noise: torch.Tensor, t: torch.Tensor, alpha_bar: torch.Tensor,
              w: Optional[torch.Tensor], pred_type: int, err_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    return PredLossFunction.apply(pred, x0, noise, t, alpha_bar, w, pred_type, err_flag)


class PerSampleMSEFunction(torch.autograd.Function):
    """mean_flat((target - pred)^2) -> [N] (gaussian_diffusion.py:925, training_losses' "mse" term) with the fixed-order HIP reduction;
    the backward applies the per-sample upstream gradient on the device."""

    @staticmethod
    def forward(ctx, pred, target):
        pred, target = pred.contiguous().float(), target.contiguous().float()
        ctx.save_for_backward(pred, target)
        return ops.gd_mse_per_sample(target, pred)

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return ops.gd_mse_per_sample_bwd(target, pred, g.contiguous().float()), None


def mse_per_sample(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return PerSampleMSEFunction.apply(pred, target)


class HybridLossFunction(torch.autograd.Function):
    """training_losses with a learned variance (gaussian_diffusion.py:893-930): per-sample (loss, mse, vb) from the [N, 2C, ...] model
    output in one fused HIP reduction; the backward writes the whole output gradient in one pass (the VLB term sees the mean half
    detached, as the reference's ``frozen_out``)."""

    @staticmethod
    def forward(ctx, model_out, x_start, x_t, target, t, tab, mean_type, var_type, vb_scale, err_flag):
        model_out = model_out.contiguous().float()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(model_out, x_start, x_t, target, t, tab)
        ctx.meta = (mean_type, var_type, vb_scale, err_flag)
        loss, mse, vb = ops.gd_hybrid_loss(x_start, x_t, target, model_out, t, tab, mean_type, var_type, vb_scale, err_flag=err_flag)
        return loss, mse, vb

    @staticmethod
    def backward(ctx, g_loss, g_mse, g_vb):
        model_out, x_start, x_t, target, t, tab = ctx.saved_tensors
        mean_type, var_type, vb_scale, err_flag = ctx.meta
        gs = [None if g is None else g.contiguous().float() for g in (g_loss, g_mse, g_vb)]
        grad = ops.gd_hybrid_loss_bwd(x_start, x_t, target, model_out, t, tab, mean_type, var_type, vb_scale, *gs, err_flag=err_flag)
        return (grad,) + (None,) * 9


def hybrid_loss(model_out, x_start, x_t, target, t, tab, mean_type: int, var_type: int, vb_scale: Optional[float], err_flag=None):
    return HybridLossFunction.apply(model_out, x_start, x_t, target, t, tab, mean_type, var_type, vb_scale, err_flag)


class SinkhornFunction(torch.autograd.Function):
    """The debiased Sinkhorn divergence between the rows of ``x`` [N, D] and ``y`` [M, D] (metrics/geom.py:28-37) on the HIP kernels:
    cost matrices in one streaming pass, the whole epsilon schedule in one launch, and - when ``x`` needs a gradient - the last
    step's weights, from which the backward writes grad_x in a second streaming pass.  ``eps_list`` is the schedule on the device."""

    @staticmethod
    def forward(ctx, x, y, eps_list, p, debias):
        need = ctx.needs_input_grad[0]
        cost = ops.pairwise_cost(x, y, p, dtype=torch.float64)
        out = ops.sinkhorn_loop(*cost, eps_list, p, debias, want_weights=need)
        if need:
            ctx.save_for_backward(x, y, out["wp"], out["wq"], out["rp"], out["rq"])
        return out["loss"].reshape(())

    @staticmethod
    def backward(ctx, g):
        x, y, wp, wq, rp, rq = ctx.saved_tensors
        return ops.rows_combine(x, y, wp, wq, rp, rq, g.reshape(1).float().contiguous()), None, None, None, None


def sinkhorn_loss(x: torch.Tensor, y: torch.Tensor, eps_list: torch.Tensor, p: int, debias: bool) -> torch.Tensor:
    return SinkhornFunction.apply(x, y, eps_list, p, debias)
