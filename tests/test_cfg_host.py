"""CPU: the surface of classifier-free guidance - the three C-ABI symbols (declared, bound, exported), the two DDPM keywords
with their defaults and the refusals that need no GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch
from torch import nn

from helpers import PARAM_SPACE, UNET_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_SYMBOLS = ["rho_p_sample_step_cfg", "rho_cond_drop", "rho_cond_keep_mask"]


def _ddpm(case="tiny2d_multi", backbone=None, backbone_kwargs=None, **kw):
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    cfg, xshape, ykind = UNET_CASES[case]
    ddpm = DDPM(backbone or UNet, dict(cfg) if backbone_kwargs is None else backbone_kwargs, LinearSchedule(20, 1e-3, 0.02),
                nn.MSELoss, timesteps=20, **kw)
    if backbone is None and ykind == "multi":
        ddpm.backbone.cond_fn = MultiEmbeddings(parameter_space=PARAM_SPACE, embedding_dim=4 * cfg["model_channels"])
    return ddpm, xshape


def test_symbols_declared_bound_and_exported():
    from rho_diffusion_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rho_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rho_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(hip.LIB_PATH):
        from rho_diffusion_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in CFG_SYMBOLS:
        assert name in declared, name
        assert name in hip.SIGNATURES, name
        assert hasattr(lib, name), name
    # the float `scale` / `p` arguments travel as c_float, sizes as int64
    assert hip.SIGNATURES["rho_p_sample_step_cfg"][1][5:7] == [ctypes.c_float, ctypes.c_int64]
    assert hip.SIGNATURES["rho_cond_keep_mask"][1][2] == ctypes.c_float
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == hip.ABI_VERSION


def test_keywords_trail_the_reference_arguments_with_neutral_defaults():
    from rho_diffusion_amd.diffusion import DDPM
    p = inspect.signature(DDPM.__init__).parameters
    assert list(p)[-2:] == ["guidance_scale", "cond_drop_prob"]
    assert p["guidance_scale"].default is None and p["cond_drop_prob"].default == 0.0
    assert inspect.signature(DDPM.reverse_process).parameters["guidance_scale"].default is None
    ddpm, _ = _ddpm()
    assert ddpm.guidance_scale is None and ddpm.cond_drop_prob == 0.0
    ddpm, _ = _ddpm(guidance_scale=2, cond_drop_prob=0.1)
    assert ddpm.guidance_scale == 2.0 and isinstance(ddpm.guidance_scale, float) and ddpm.cond_drop_prob == 0.1


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan")])
def test_cond_drop_prob_outside_the_half_open_unit_interval_is_refused(p):
    with pytest.raises(ValueError, match="cond_drop_prob"):
        _ddpm(cond_drop_prob=p)


def test_cond_drop_prob_just_inside_is_taken():
    assert _ddpm(cond_drop_prob=0.0)[0].cond_drop_prob == 0.0
    assert _ddpm(cond_drop_prob=0.999)[0].cond_drop_prob == 0.999


def test_guidance_without_conditions_is_refused():
    ddpm, xshape = _ddpm(guidance_scale=2.0)
    with pytest.raises(ValueError, match="conditions"):
        ddpm.reverse_process(torch.zeros(xshape))                       # the attribute
    ddpm, xshape = _ddpm()
    with pytest.raises(ValueError, match="conditions"):
        ddpm.reverse_process(torch.zeros(xshape), None, guidance_scale=0.0)       # the per-call value; 0 is a scale like any other


def test_guidance_on_an_unconditional_unet_is_refused():
    ddpm, xshape = _ddpm("tiny2d")
    assert ddpm.backbone.num_classes is None
    with pytest.raises(ValueError, match="num_classes"):
        ddpm.reverse_process(torch.zeros(xshape), torch.zeros(xshape[0], 2), guidance_scale=3.0)


def test_guidance_on_a_backbone_without_an_engine_is_refused():
    from rho_diffusion_amd.models.vit import VisionTransformer
    kw = dict(patch_size=4, input_shapes=[16, 16], num_channels=1, embedding_dim=64, hidden_dim=64, activation="GELU",
              transformer_depth=1, num_heads=2)
    ddpm, _ = _ddpm(backbone=VisionTransformer, backbone_kwargs=kw)
    assert not hasattr(ddpm.backbone, "engine")
    with pytest.raises(ValueError, match="unconditional"):
        ddpm.reverse_process(torch.zeros(2, 1, 16, 16), torch.zeros(2, 2), guidance_scale=3.0)


def test_unguided_call_on_the_cpu_still_fails_on_the_device_check():
    """guidance_scale=None changes nothing: the first thing reverse_process does is still to ask for GPU tensors."""
    from rho_diffusion_amd.hip import RhoHipError
    ddpm, xshape = _ddpm()
    with pytest.raises(RhoHipError):
        ddpm.reverse_process(torch.zeros(xshape), None)
