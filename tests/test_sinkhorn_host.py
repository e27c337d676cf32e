"""CPU: the host side of the Sinkhorn divergence (metrics/geom.py:28-37) - the epsilon schedule, the float64 restatement the GPU
tests measure against (pinned here by exact transport), what the Python layer refuses, and the registry / alias names."""
import math
import sys

import numpy as np
import pytest
import torch

import sinkhorn_ref as SR


def test_epsilon_schedule_against_hand_written_lists():
    from rho_diffusion_amd.metrics.geom import epsilon_schedule
    assert epsilon_schedule(0.005, 1, 0.01, 0.5) == [0.005, 0.01]                   # blur >= diameter: the two ends
    assert epsilon_schedule(0.01, 1, 0.01, 0.5) == [0.01, 0.01]
    got = epsilon_schedule(4.0, 1, 0.01, 0.5)
    want = [4.0] + [4.0 * 0.5 ** k for k in range(9)] + [0.01]                      # 4, 4, 2, 1, ..., 0.015625, 0.01
    assert len(got) == 11
    assert got[0] == 4.0 and got[-1] == 0.01
    np.testing.assert_allclose(got, want, rtol=1e-14)
    got2 = epsilon_schedule(4.0, 2, 0.01, 0.5)
    want2 = [16.0] + [16.0 * 0.25 ** k for k in range(9)] + [0.01 ** 2]             # p = 2 squares the ends and the ratio
    assert got2[0] == 16.0 and got2[-1] == 0.01 ** 2 and len(got2) == 11
    np.testing.assert_allclose(got2, want2, rtol=1e-14)
    assert got == SR.epsilon_schedule(4.0, 1, 0.01, 0.5) and got2 == SR.epsilon_schedule(4.0, 2, 0.01, 0.5)


def _pair(n, m, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=torch.float64), torch.randn(m, d, generator=g, dtype=torch.float64) + 0.5


def test_restatement_against_exact_transport():
    """At blur 0.01 the divergence sits just below the optimal assignment cost (entropic bias; the self terms vanish: distinct points
    are ~90 apart)."""
    from scipy.optimize import linear_sum_assignment
    x, y = _pair(8, 8, 4099)
    r = SR.sinkhorn(x, y, p=1)
    C = r["costs"][0].numpy()
    rows, cols = linear_sum_assignment(C)
    exact = float(C[rows, cols].mean())
    loss = float(r["loss"])
    print(f"exact {exact:.9f} loss {loss:.9f} rel gap {(exact - loss) / exact:.3e}")
    assert 0.0 <= exact - loss <= 1e-3 * exact


@pytest.mark.parametrize("p", [1, 2])
def test_restatement_is_zero_on_identical_sets(p):
    x, _ = _pair(6, 6, 257)
    r = SR.sinkhorn(x, x.clone(), p=p)
    assert abs(float(r["loss"])) <= 1e-15 * r["c_max"]


@pytest.mark.parametrize("p", [1, 2])
def test_closed_form_gradient_equals_autograd(p):
    """The formula the kernels implement (P, Q of the last step, divided by the cost for p = 1) against autograd of the restatement."""
    x, y = _pair(5, 7, 9)
    r = SR.sinkhorn(x, y, p=p, want_grad=True, upstream=2.5)
    got = SR.closed_form_grad(x, y, p, r["eps_last"], r["h_b"], r["h_a"], upstream=2.5)
    assert float((got - r["grad"]).abs().max()) <= 1e-11 * float(r["grad"].abs().max())


def test_fp32_mode_accumulates_costs_left_to_right():
    x, y = _pair(3, 2, 1000)
    got = SR.sq_dists(x, y, fp32=True).numpy()
    xf, yf = x.float().numpy(), y.float().numpy()
    for i in range(3):
        for j in range(2):
            assert got[i, j] == np.cumsum((xf[i] - yf[j]) ** 2, dtype=np.float32)[-1]


def test_refusals():
    from rho_diffusion_amd.hip import RhoHipError
    from rho_diffusion_amd.metrics import SinkhornDivergence, WassersteinWrapper
    w = WassersteinWrapper()
    with pytest.raises(AssertionError):
        w(torch.zeros(4, 1, 8, 8), torch.zeros(4, 1, 8, 4))
    with pytest.raises(RhoHipError, match="128"):
        w(torch.zeros(129, 3), torch.zeros(129, 3))
    with pytest.raises(RhoHipError, match="p must be 1 or 2"):
        SinkhornDivergence(p=3)
    with pytest.raises(RhoHipError, match="first argument only"):
        w(torch.zeros(4, 3), torch.zeros(4, 3, requires_grad=True))
    with pytest.raises(RhoHipError, match="must live on the GPU"):
        w(torch.zeros(4, 3), torch.ones(4, 3))
    with pytest.raises(RhoHipError, match="scaling"):
        SinkhornDivergence(scaling=1.0)


def test_registry_and_alias_names():
    import rho_diffusion_amd as RA
    from rho_diffusion_amd.registry import registry
    cls = registry.get("layers", "WassersteinWrapper")
    assert cls is RA.metrics.geom.WassersteinWrapper
    m = cls()
    assert (m.p, m.blur, m.scaling, m.debias, m.diameter) == (1, 0.01, 0.5, True, None)
    RA.install_alias()
    try:
        from rho_diffusion.metrics.geom import WassersteinWrapper
        import rho_diffusion.metrics as RM
        assert WassersteinWrapper is cls and RM.PeakSignalNoiseRatio is RA.metrics.PeakSignalNoiseRatio
    finally:
        for k in [k for k in sys.modules if k == "rho_diffusion" or k.startswith("rho_diffusion.")]:
            del sys.modules[k]


def test_pipeline_metrics_stay_empty_by_default():
    from torch import nn
    from golden_cfg import UNET_CASES
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    kw, _, _ = UNET_CASES["tiny2d"] if "tiny2d" in UNET_CASES else next(iter(UNET_CASES.values()))
    ddpm = DDPM(UNet, dict(kw), LinearSchedule(10, 1e-3, 0.02), nn.MSELoss, timesteps=10)
    assert len(ddpm.metrics) == 0
