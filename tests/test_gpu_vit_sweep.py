"""-m gpu: forward + backward of the whole fp32 VisionTransformer against the float64 twin of its restatement (tests/vit_ref64.py), per
tensor, on the six configurations of tests/vit_sweep_cases.SWEEP_CASES (what the constructor accepts and no recorded case runs) and
the four of vit_cfg.VIT_CASES.

The prediction, the loss, every parameter gradient and the input gradient (``<input>``) are held against float64 in both norms; the
float32 restatement only sizes the bound (K = 4 times its own distance from float64, plus 16 float32 ulps of the tensor's size - the
bars of tests/unet_sweep_cases.py, imported) and is never the code under test.  A failure names case, tensor, both norms and the
index of the worst element.

ONE LAUNCH PATH.  The switches of test_gpu_training.PATHS (RHO_PHASE_UPSAMPLE / RHO_S2_SPLIT and their _BWD forms) are read by
``UNetEngine``'s plan builder only (engine/unet_engine.py, ``_PLAN_ENV``); the ViT calls ``ops.conv`` / ``ops.conv_wgrad`` with a
1x1x1 kernel directly, where no environment variable of that table is read.  They cannot change which kernel a launch here takes, so
each case runs once.

MEASURED on an MI355X: worst err / (the float32 restatement's own error) over prediction, loss and every gradient, per case, as
"l2 ratio | max-norm ratio" with the tensor that sets it:
    b1_tanh_hw64    1.20 | 1.94      (norm_2.weight | linear_block.0.bias)
    elu_hw128_2d    2.20 | 2.35      (output_conv.bias | transformer_blocks.1.norm_1.weight)
    sigmoid_hw256   2.71 | 2.61      (pos_embedding.1.bias | in_proj_bias)
    wide_e1024      1.52 | 1.67      (<loss> | out_proj.weight)
    n1_token        1.24 | 1.37      (norm_2.weight | norm_1.weight of block 0)
    long_ragged     1.68 | 1.96      (in_proj_bias | output_conv.bias)
    vit1d           1.40 | 1.96      (norm_2.weight | pos_embedding.1.bias)
    vit2d           1.01 | 1.14      (norm_1.weight of block 0)
    vit3d           2.14 | 4.30      (norm_1.weight of block 0, element 52)
    vit2d_long      2.11 | 2.11      (output_conv.bias, one channel: one number)
Every tensor meets K = 4 plus the floor; no tensor class has a K of its own.  The 4.30 is inside the floor: a 64-element LayerNorm
weight whose float32-restatement error happens to be 0.76e-7 of max|g| at its worst element against 3.2e-7 for the engine (error
1.15e-6, bound 4.45e-6; the l2 ratio of that tensor is 2.1).  The output-conv bias of the one-channel models (sigmoid_hw256,
wide_e1024, vit1d, vit2d_long) - one number, the mean of the residuals, the class that needed K = 16 on the UNet - stays at or
below 2.11 here.  ``n1_token`` and ``wide_e1024`` take the attention kernels to T = 1 and T = 2: both run clean.
"""
import pytest
import torch

import vit_sweep_cases as VC
from gpu_util import DEV

pytestmark = pytest.mark.gpu


def build_model(case: str, sd=None, dtype="fp32"):
    """The project's VisionTransformer for a case with the case's deterministic weights (or ``sd``), on the device."""
    from rho_diffusion_amd.models.vit import VisionTransformer
    model = VisionTransformer(**dict(VC.ALL_CASES[case][0]), compute_dtype=dtype)
    model.load_state_dict(sd if sd is not None else VC.sweep_inputs(case)[4])
    return model.to(DEV)


def train_step(model, x, t, target):
    """(prediction, loss, {name: gradient}) of one forward + backward in training mode; gradients are what the step ADDED to p.grad
    (the caller zeroes them), the input's under ``VC.INPUT``."""
    from rho_diffusion_amd.autograd import mse_loss
    model.train()
    xd = x.to(DEV).requires_grad_(True)
    pred = model(xd, t.to(DEV))
    loss = mse_loss(pred, target.to(DEV))
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    grads[VC.INPUT] = xd.grad.detach().clone()
    return pred.detach().clone(), loss.detach().clone(), grads


@pytest.mark.parametrize("case", list(VC.ALL_CASES))
def test_vit_fp32_per_tensor_vs_float64(case):
    kw, x, t, target, sd = VC.sweep_inputs(case)
    refs = VC.case_refs(case)
    model = build_model(case)
    assert set(n for n, _ in model.named_parameters()) | {VC.INPUT} == set(refs["f64"][2])
    pred, loss, grads = train_step(model, x, t, target)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == tuple(refs["f64"][0].shape)
    assert all(g.dtype == torch.float32 and tuple(g.shape) == tuple(refs["f64"][2][n].shape) for n, g in grads.items())
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    VC.check_against_refs(case, "fp32", refs, pred, loss, grads)
