"""GaussianDiffusionPipeline's guided-diffusion API, host side (no GPU): the enums and attributes of the reference class
(gaussian_diffusion.py:107-141, :211-233), the fixed-variance tables against g18 (recorded from the reference), the refusals of
what is not built, and the ``rho_diffusion.metrics.losses`` alias."""
import sys

import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, load_golden


def _pipe(T=20, case="tiny3d"):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES[case]
    return GaussianDiffusionPipeline(UNet, dict(kw), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T), xshape


def test_enums_and_attributes_match_the_reference():
    from rho_diffusion_amd.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType
    assert [(m.name, m.value) for m in ModelMeanType] == [("PREVIOUS_X", 1), ("START_X", 2), ("EPSILON", 3)]
    assert [(m.name, m.value) for m in ModelVarType] == [("LEARNED", 1), ("FIXED_SMALL", 2), ("FIXED_LARGE", 3), ("LEARNED_RANGE", 4)]
    assert [(m.name, m.value) for m in LossType] == [("MSE", 1), ("RESCALED_MSE", 2), ("KL", 3), ("RESCALED_KL", 4)]
    assert [m.is_vb() for m in LossType] == [False, False, True, True]
    pipe, _ = _pipe()
    assert pipe.model_mean_type is ModelMeanType.START_X
    assert pipe.model_var_type is ModelVarType.FIXED_LARGE
    assert pipe.loss_type is LossType.MSE
    for name in ("q_mean_variance", "q_posterior_mean_variance", "p_mean_variance", "_predict_xstart_from_eps", "_predict_eps_from_xstart",
                 "condition_mean", "condition_score", "p_sample", "p_sample_loop", "p_sample_loop_progressive", "ddim_sample",
                 "ddim_sample_loop", "ddim_sample_loop_progressive", "ddim_reverse_sample", "_vb_terms_bpd", "_prior_bpd", "calc_bpd_loop",
                 "training_losses"):
        assert callable(getattr(pipe, name)), name


@pytest.mark.parametrize("case,T", [("tiny2d", 50), ("tiny3d", 20)])
def test_fixed_variance_tables_bit_equal_to_reference(case, T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType, gd_table_rows, model_variance_tables
    from rho_diffusion_amd.engine.ops import GD_ROW
    g = load_golden("g18_gaussian_api.npz")
    pipe, _ = _pipe(T, case)
    tag = f"{case}_T{T}"
    for vt, key in ((ModelVarType.FIXED_LARGE, "fixed_large"), (ModelVarType.FIXED_SMALL, "fixed_small")):
        var, logvar = model_variance_tables(pipe.tables, vt)
        assert np.array_equal(var, g[f"{tag}/tab/{key}_var"]) and var.dtype == np.float64
        assert np.array_equal(logvar, g[f"{tag}/tab/{key}_logvar"])
        # the packed device table carries them cast to float32, as _extract_into_tensor does (:91-105)
        rows = gd_table_rows(pipe.tables, vt)
        assert rows.dtype == np.float32 and rows.shape == (len(GD_ROW), T)
        assert np.array_equal(rows[GD_ROW["model_var"]], g[f"{tag}/tab/{key}_var"].astype(np.float32))
        assert np.array_equal(rows[GD_ROW["model_logvar"]], g[f"{tag}/tab/{key}_logvar"].astype(np.float32))
    rows = gd_table_rows(pipe.tables, ModelVarType.FIXED_LARGE)
    assert np.array_equal(rows[GD_ROW["abar_next"]], pipe.alphas_cumprod_next.astype(np.float32))
    assert np.array_equal(rows[GD_ROW["1m_abar"]], (1.0 - pipe.alphas_cumprod).astype(np.float32))


def test_unbuilt_configurations_are_refused_naming_the_reference_lines():
    from rho_diffusion_amd.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType, model_variance_tables
    pipe, xshape = _pipe()
    for vt in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
        with pytest.raises(NotImplementedError, match="368-383"):
            model_variance_tables(pipe.tables, vt)
        pipe.model_var_type = vt
        with pytest.raises(NotImplementedError, match="368-383"):
            pipe._gd_table("cpu")
    pipe.model_var_type = ModelVarType.FIXED_LARGE
    pipe.model_mean_type = ModelMeanType.PREVIOUS_X
    with pytest.raises(NotImplementedError, match="417-422"):
        pipe._mean_code()
    pipe.model_mean_type = ModelMeanType.START_X
    for lt in (LossType.KL, LossType.RESCALED_KL):
        pipe.loss_type = lt
        with pytest.raises(NotImplementedError, match="877-889"):
            pipe.training_losses(pipe.backbone, torch.zeros(xshape), torch.zeros(xshape[0], dtype=torch.long))
    pipe.loss_type = LossType.MSE
    with pytest.raises(AssertionError, match="Reverse ODE"):
        pipe.ddim_reverse_sample(pipe.backbone, torch.zeros(xshape), torch.zeros(xshape[0], dtype=torch.long), eta=0.5)


def test_metrics_refuse_other_broadcasts():
    from rho_diffusion_amd.hip import RhoHipError
    from rho_diffusion_amd.metrics import discretized_gaussian_log_likelihood, normal_kl
    x = torch.zeros(3, 2, 4, 5)
    with pytest.raises(RhoHipError, match="no other broadcast"):
        normal_kl(x, torch.zeros(1, 2, 1, 1), 0.0, 0.0)           # a per-channel operand
    with pytest.raises(RhoHipError, match="no other broadcast"):
        normal_kl(x, torch.zeros(3, 1), 0.0, 0.0)                 # another rank
    with pytest.raises(RhoHipError, match="no other broadcast"):
        discretized_gaussian_log_likelihood(x, means=torch.zeros(4, 5), log_scales=0.0)
    with pytest.raises(RhoHipError, match="at least one argument must be a Tensor"):
        normal_kl(0.0, 0.0, 0.0, 0.0)
    with pytest.raises(RhoHipError, match="must live on the GPU"):       # accepted shapes, but the HIP path has no CPU fallback
        normal_kl(x, torch.zeros(3, 1, 1, 1), 0.0, 0.0)


def test_reference_metrics_module_resolves_under_the_alias():
    import rho_diffusion_amd as RA
    import rho_diffusion_amd.diffusion.gaussian_diffusion as GDm
    RA.install_alias()
    try:
        from rho_diffusion.metrics.losses import approx_standard_normal_cdf, discretized_gaussian_log_likelihood, normal_kl
        from rho_diffusion.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType
        assert normal_kl is RA.metrics.losses.normal_kl
        assert discretized_gaussian_log_likelihood is RA.metrics.losses.discretized_gaussian_log_likelihood
        assert approx_standard_normal_cdf is RA.metrics.losses.approx_standard_normal_cdf
        assert (LossType, ModelMeanType, ModelVarType) == (GDm.LossType, GDm.ModelMeanType, GDm.ModelVarType)
    finally:
        for k in [k for k in sys.modules if k == "rho_diffusion" or k.startswith("rho_diffusion.")]:
            del sys.modules[k]
