"""GaussianDiffusionPipeline with a learned variance, host side (no GPU): the learned-range rows of the packed table against g19
(recorded from the reference, gaussian_diffusion.py:368-383), the refusals that remain, and the new C-ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rho_gd_posterior_step_lv", "rho_gd_vlb_terms_lv", "rho_gd_hybrid_loss", "rho_gd_hybrid_loss_bwd", "rho_gd_ddim_step_strided",
               "rho_abs_quantile_strided")


def _pipe(T=20, case="tiny3d", learned=True):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES[case]
    kw = dict(kw, out_channels=2 * kw["in_channels"]) if learned else dict(kw)
    return GaussianDiffusionPipeline(UNet, kw, LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T), xshape


@pytest.mark.parametrize("case,T", [("tiny2d", 50), ("tiny3d", 20)])
def test_learned_range_rows_bit_equal_to_reference(case, T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType, gd_table_rows, gd_table_rows_learned
    from rho_diffusion_amd.engine.ops import GD_ROW, GD_ROWS
    g = load_golden("g19_learned_variance.npz")
    pipe, _ = _pipe(T, case)
    tag = f"{case}_T{T}"
    assert len(GD_ROWS) == 15 and GD_ROW["log_beta"] == 14 and GD_ROW["post_logvar"] == 6
    rows = gd_table_rows_learned(pipe.tables)
    assert rows.dtype == np.float32 and rows.shape == (15, T)
    # min_log = posterior_log_variance_clipped, max_log = log(betas), each cast float64 -> float32 as _extract_into_tensor does
    assert np.array_equal(rows[GD_ROW["post_logvar"]], g[f"{tag}/tab/min_log"].astype(np.float32))
    assert np.array_equal(rows[GD_ROW["log_beta"]], g[f"{tag}/tab/max_log"].astype(np.float32))
    # the fixed tables carry the same row; their other rows are unchanged
    fixed = gd_table_rows(pipe.tables, ModelVarType.FIXED_SMALL)
    assert np.array_equal(fixed[GD_ROW["log_beta"]], rows[GD_ROW["log_beta"]])
    assert np.array_equal(fixed[:GD_ROW["model_var"]], rows[:GD_ROW["model_var"]])


def test_remaining_refusals():
    from rho_diffusion_amd.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType, model_variance_tables
    pipe, xshape = _pipe()
    B, C = xshape[0], xshape[1]
    x = torch.zeros(xshape)
    t = torch.zeros(B, dtype=torch.long)
    out2 = torch.zeros((B, 2 * C) + tuple(xshape[2:]))
    for vt in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
        pipe.model_var_type = vt
        # a learned variance has no per-t variance table: the fixed accessors keep refusing it
        with pytest.raises(NotImplementedError, match="368-383"):
            model_variance_tables(pipe.tables, vt)
        with pytest.raises(NotImplementedError, match="368-383"):
            pipe._gd_table("cpu")
        # a C-channel output under a learned variance (the reference asserts the 2C shape, :369)
        with pytest.raises(AssertionError, match="2C-channel"):
            pipe._check_output(x, x)
        pipe._check_output(out2, x)
        pipe.model_mean_type = ModelMeanType.PREVIOUS_X
        with pytest.raises(NotImplementedError, match="417-422"):
            pipe._mean_code()
        pipe.model_mean_type = ModelMeanType.START_X
        for lt in (LossType.KL, LossType.RESCALED_KL):
            pipe.loss_type = lt
            with pytest.raises(NotImplementedError, match="877-889"):
                pipe.training_losses(lambda *a, **k: out2, x, t)
        pipe.loss_type = LossType.MSE
    # a 2C output under a fixed variance
    for vt in (ModelVarType.FIXED_LARGE, ModelVarType.FIXED_SMALL):
        pipe.model_var_type = vt
        with pytest.raises(NotImplementedError, match="368-383"):
            pipe._check_output(out2, x)
        pipe._check_output(x, x)


def test_generate_template_takes_in_channels_with_a_learned_variance():
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType
    pipe, xshape = _pipe()
    pipe.model_var_type = ModelVarType.LEARNED_RANGE
    seen = {}

    def fake_reverse(x_T, conditions=None, t_checkpoints=None, eta=0.0):
        seen["shape"] = tuple(x_T.shape)
        return {"denoised": x_T, "buffer": None}
    pipe.reverse_process = fake_reverse
    pipe.make_image_grid = lambda x, filename=None: x
    pipe.generate()
    assert seen["shape"] == (pipe.sampling_batch_size, 1) + tuple(xshape[2:])


def test_new_symbols_in_header_and_library():
    from rho_diffusion_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rho_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", text).group(1)) == 10 == hip.ABI_VERSION
    assert int(re.search(r"#define\s+RHO_GD_ROWS\s+(\d+)", text).group(1)) == 15
    assert int(re.search(r"#define\s+RHO_GD_LOG_BETA\s+(\d+)", text).group(1)) == 14
    if not os.path.exists(hip.LIB_PATH):
        from rho_diffusion_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
