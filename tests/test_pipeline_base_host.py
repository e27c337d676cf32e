"""What the concrete pipelines share through AbstractDiffusionPipeline, host side (no GPU): the ``conditions`` parser of
reverse_process, and that the one inherited ``noise`` is still told apart from an override where DDPM's graph path asks."""
import pytest
import torch

from rho_diffusion_amd.diffusion.abstract_diffusion import AbstractDiffusionPipeline


def test_resolve_conditions():
    resolve, B = AbstractDiffusionPipeline._resolve_conditions, 5
    assert resolve(None, B, "cpu") is None
    got = resolve(7, B, "cpu")
    assert got.dtype == torch.long and torch.equal(got, torch.full((B,), 7))
    got = resolve([3, 1, 4, 1, 5], B, "cpu")
    assert got.dtype == torch.long and torch.equal(got, torch.tensor([3, 1, 4, 1, 5]))
    t = torch.arange(B)
    assert resolve(t, B, "cpu") is t
    torch.manual_seed(1234)
    got = resolve("auto", B, "cpu")
    torch.manual_seed(1234)
    assert got.dtype == torch.long and torch.equal(got, torch.randint(0, 10, (B,)))
    with pytest.raises(TypeError, match="float"):
        resolve(3.5, B, "cpu")
    with pytest.raises(TypeError, match="'automatic'"):
        resolve("automatic", B, "cpu")


def test_noise_is_inherited_and_overrides_are_detected():
    from rho_diffusion_amd.diffusion import DDPM, GaussianDiffusionPipeline
    from rho_diffusion_amd.diffusion.diffusers_ddpm import DiffusersDDPMPipeline

    class Taped(DDPM):
        def noise(self, data):
            return torch.zeros_like(data)
    for cls in (DDPM, GaussianDiffusionPipeline, DiffusersDDPMPipeline):
        assert cls.noise is AbstractDiffusionPipeline.noise
    assert Taped.noise is not AbstractDiffusionPipeline.noise
