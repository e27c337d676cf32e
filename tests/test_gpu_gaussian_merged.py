"""-m gpu: the two instantiations of the posterior and VLB kernels of csrc/gaussian.hip against each other, and the per-sample views of
the merged wrappers against contiguous copies.

A learned variance of type LEARNED whose values are, per sample, the table's float32 model_logvar[t[b]] is the fixed variance of that
table: the learned instantiation then evaluates per element what the fixed one hoists per thread (0.5*logvar, exp, the KL's
log-variance terms) from the same float32 operands in the same order, so every output agrees bit for bit.  The ``grad`` term is left
out on purpose: the fixed kernel reads the model_var row where the learned one computes expf(logvar).  A view and its copy hold the
same values, so the strided and the plain entry points agree bit for bit too.

Shapes: (3, 1, 7, 79) is 553 elements per sample, three workgroups of 256 with a ragged tail; (2, 1, 5) is one partial workgroup.
t = [0, 7, 19] (the first B of them): t == 0 masks the noise and selects the decoder NLL, 19 is the last row of the table.

Left to other files: the values themselves at the sizes where the grids loop again, with ``grad``, other strides, offset bases, err_flag
and the refusals of the step kernels are in test_gpu_gaussian_step_edges.py (restatement and bounds: gd_step_ref.py, checked on the
CPU by test_gd_step_ref_host.py); the loss side in test_gpu_gaussian_loss_bounds.py (gd_loss_ref.py)."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, det_normal
from gpu_util import DEV

pytestmark = pytest.mark.gpu
SHAPES = [(3, 1, 7, 79), (2, 1, 5)]
T = 20


@functools.lru_cache(maxsize=None)
def _table():
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType
    from rho_diffusion_amd.models import UNet
    pipe = GaussianDiffusionPipeline(UNet, dict(UNET_CASES["tiny2d"][0]), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T)
    pipe.model_var_type = ModelVarType.FIXED_SMALL
    return pipe._tab(DEV)


@functools.lru_cache(maxsize=None)
def _data(shape):
    """x_start, x_t, noise, t and a [B, 2, ...] model output whose variance half holds model_logvar[t[b]]; read-only."""
    from rho_diffusion_amd.engine.ops import GD_ROW
    B, tag = shape[0], "x".join(map(str, shape))
    t = torch.tensor([0, 7, 19][:B], dtype=torch.int64, device=DEV)
    scale = torch.tensor([0.3, 2.5, 3.5][:B]).view(-1, *([1] * (len(shape) - 1)))      # quantiles below and above the threshold's 1
    mean = (det_normal(shape, "gm_mean" + tag) * scale).to(DEV)
    logvar = _table()[GD_ROW["model_logvar"]][t].view(-1, *([1] * (len(shape) - 1))).expand(shape)
    d = {k: det_normal(shape, f"gm_{k}{tag}").to(DEV) for k in ("x_t", "noise")}
    d["x_start"] = det_normal(shape, "gm_xs" + tag).clamp(-1, 1).to(DEV)
    d["t"], d["mo"] = t, torch.cat([mean, logvar], dim=1).contiguous()
    return d


def _np(*tensors):
    return [x.cpu().numpy() for x in tensors]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("mean_type", ["START_X", "EPSILON"])
@pytest.mark.parametrize("shape", SHAPES)
def test_fixed_and_learned_instantiations_agree_bit_for_bit(shape, mean_type, clip):
    from rho_diffusion_amd.engine import ops
    d, tab, B = _data(shape), _table(), shape[0]
    code = getattr(ops, "GD_" + mean_type)
    mean, var = d["mo"][:, :1], d["mo"][:, 1:]
    assert not mean.is_contiguous() and not var.is_contiguous()
    q = ops.abs_quantile(mean, 0.9) if clip else None
    got = {}
    for kind, src, kw in (("fixed", mean.contiguous(), {}), ("learned", mean, {"var_values": var, "var_type": ops.GD_LEARNED})):
        vb, raw_kl, raw_nll, xstart_mse, mse = (torch.empty(B, device=DEV) for _ in range(5))
        px, out, px2 = (torch.empty(shape, device=DEV) for _ in range(3))
        ops.gd_vlb_terms(d["x_start"], d["x_t"], src, d["t"], tab, code, q, d["noise"], vb, xstart_mse, mse, raw_kl, raw_nll, px, **kw)
        ops.gd_posterior_step(d["x_t"], src, d["t"], tab, code, q, None, d["noise"], out, px2, **kw)
        got[kind] = dict(zip(("vb", "raw_kl", "raw_nll", "xstart_mse", "mse", "pred_xstart", "out", "step_pred_xstart"),
                             _np(vb, raw_kl, raw_nll, xstart_mse, mse, px, out, px2)))
    for k, v in got["fixed"].items():
        assert np.isfinite(v).all(), k
        assert np.array_equal(v, got["learned"][k]), (k, v, got["learned"][k])
    assert got["fixed"]["vb"][0] == got["fixed"]["raw_nll"][0] and got["fixed"]["vb"][1] == got["fixed"]["raw_kl"][1]


@pytest.mark.parametrize("shape", SHAPES)
def test_views_equal_copies(shape):
    from rho_diffusion_amd.engine import ops
    d, tab = _data(shape), _table()
    view = d["mo"][:, :1]
    copy = view.contiguous()
    assert not view.is_contiguous()
    q, qc = ops.abs_quantile(view, 0.9), ops.abs_quantile(copy, 0.9)
    assert np.array_equal(*_np(q, qc))
    assert float(q.max()) > 1.0 > float(q.min())
    for code in (ops.GD_START_X, ops.GD_EPSILON):
        for noise, eta, reverse in ((d["noise"], 0.5, False), (None, 0.0, True)):
            res = []
            for src in (view, copy):
                sample, px = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
                ops.gd_ddim_step(d["x_t"], src, d["t"], tab, code, q, None, noise, eta, reverse, sample, px)
                res.append(_np(sample, px))
            for a, b in zip(*res):
                assert np.isfinite(a).all() and np.array_equal(a, b), (code, reverse)
