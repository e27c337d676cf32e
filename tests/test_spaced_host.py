"""CPU: the host side of few-step sampling on a spaced timestep sequence (rho_diffusion_amd/diffusion/spaced.py) - the sequence, the
coefficient rows of rho_p_sample_step_spaced against the float64 formulas written out here, the degenerate rows of the schedules,
the checkpoint rule - and the surface: the two C-ABI symbols (declared, bound, exported) and the new DDPM keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACED_SYMBOLS = ["rho_p_sample_step_spaced", "rho_spaced_advance"]


def _sp():
    from rho_diffusion_amd.diffusion import spaced
    return spaced


def _schedule(name):
    from rho_diffusion_amd.diffusion import CosineBetaSchedule, LinearSchedule
    return {"linear1000": lambda: LinearSchedule(1000), "cosine1000": lambda: CosineBetaSchedule(1000),
            "linear20": lambda: LinearSchedule(20, 1e-3, 0.01), "linear20_zero": lambda: LinearSchedule(20, 1e-3, 0.02)}[name]()


def _alpha_bar(name) -> torch.Tensor:
    ab = _schedule(name)["alpha_bar_t"]
    assert ab.dtype == torch.float32
    return ab


# ----------------------------------------------------------------------------- spaced_timesteps
@pytest.mark.parametrize("T", [2, 10, 20, 21, 1000, 1001])
def test_timesteps_endpoints_and_strictly_increasing(T):
    sp = _sp()
    sizes = range(1, T + 1) if T <= 21 else list(range(1, 65)) + [T]
    for S in sizes:
        taus = sp.spaced_timesteps(T, S)
        assert len(taus) == S and all(isinstance(t, int) for t in taus), (T, S)
        assert taus[-1] == T - 1, (T, S)
        if S > 1:
            assert taus[0] == 0, (T, S)
            assert all(b > a for a, b in zip(taus, taus[1:])), (T, S, taus)
            assert taus == [(2 * i * (T - 1) + (S - 1)) // (2 * (S - 1)) for i in range(S)]
    assert sp.spaced_timesteps(T, T) == list(range(T))
    assert sp.spaced_timesteps(T, 1) == [T - 1]


def test_timesteps_hand_cases():
    sp = _sp()
    assert sp.spaced_timesteps(20, 5) == [0, 5, 10, 14, 19]            # 4.75 -> 5, 9.5 -> 10 (halves up), 14.25 -> 14
    assert sp.spaced_timesteps(1000, 3) == [0, 500, 999]               # 499.5 -> 500
    assert sp.spaced_timesteps(1001, 50)[:3] == [0, 20, 41]


@pytest.mark.parametrize("T,S", [(20, 0), (20, -1), (20, 21), (1000, 1001), (2, 3)])
def test_timesteps_refusals(T, S):
    with pytest.raises(ValueError, match="num_steps"):
        _sp().spaced_timesteps(T, S)


def test_explicit_sequences():
    sp = _sp()
    assert sp.resolve_timesteps(20, 5) == sp.spaced_timesteps(20, 5)
    assert sp.resolve_timesteps(20, range(19)) == list(range(19))
    assert sp.resolve_timesteps(20, [3, 7, 19]) == [3, 7, 19]
    assert sp.resolve_timesteps(20, torch.tensor([0, 19])) == [0, 19]
    for bad in ([], [0, 0], [5, 3], [0, 20], [-1, 4], [0, 2, 2, 5], [0.5, 3]):
        with pytest.raises(ValueError):
            sp.resolve_timesteps(20, bad)
    with pytest.raises(ValueError):
        sp.resolve_timesteps(20, True)


# ----------------------------------------------------------------------------- spaced_coefficients
def _rows64(ab32: torch.Tensor, taus, eta):
    """The issue's formulas in float64 on the float32 table, vectorised in numpy: [S, 8] float64."""
    ab = ab32.double().numpy()[np.asarray(taus)]
    abp = np.concatenate([[1.0], ab[:-1]])
    one_m = 1.0 - ab
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(one_m == 0.0, 0.0, 1.0 / np.sqrt(one_m))
        sigma = np.where(one_m == 0.0, 0.0, eta * np.sqrt((1.0 - abp) / one_m) * np.sqrt(1.0 - ab / abp))
    coef_eps = np.sqrt(np.maximum(1.0 - abp - sigma ** 2, 0.0))
    return np.stack([np.sqrt(1.0 / ab), np.sqrt(1.0 / ab - 1.0), np.sqrt(ab), inv, np.sqrt(abp), sigma, coef_eps, np.zeros_like(ab)], 1)


@pytest.mark.parametrize("name", ["linear1000", "cosine1000", "linear20"])
@pytest.mark.parametrize("S", [1, 2, 5, 50])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_coefficients_are_the_float64_formulas_rounded_once(name, S, eta):
    sp = _sp()
    ab = _alpha_bar(name)
    if S > len(ab):
        S = len(ab)                                                  # linear20 at "50": every timestep
    taus = sp.spaced_timesteps(len(ab), S)
    rows = sp.spaced_coefficients(ab, taus, eta)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (S, 8) and rows.is_contiguous()
    want = torch.from_numpy(_rows64(ab, taus, eta)).to(torch.float32)
    assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), (name, S, eta, (rows - want).abs().max())
    assert torch.isfinite(rows).all()
    # row 0: the walk ends at alpha_bar = 1 - the last step returns the x0 estimate
    assert float(rows[0, 5]) == 0.0 and float(rows[0, 6]) == 0.0 and float(rows[0, 4]) == 1.0 and (rows[:, 7] == 0).all()
    if eta == 0.0:
        assert (rows[:, 5] == 0).all()
    else:                                                            # noise wherever the step starts and ends below alpha_bar = 1
        abp = torch.cat([torch.ones(1), ab[torch.tensor(taus)][:-1]])
        assert torch.equal(rows[:, 5] > 0, abp < 1), (name, S, eta)  # (the cosine's t = 0 has alpha_bar = 1: its row 1 is noiseless)


@pytest.mark.parametrize("name", ["linear1000", "linear20"])
def test_eta_one_on_every_timestep_is_the_posterior_variance(name):
    """At S == T, eta == 1: sigma_t^2 = (1 - ab_{t-1}) / (1 - ab_t) * (1 - ab_t / ab_{t-1}), the DDPM posterior variance."""
    sp = _sp()
    ab32 = _alpha_bar(name)
    T = len(ab32)
    ab = ab32.double().numpy()
    # float64 rows: rebuild sigma the way spaced_coefficients does before its one rounding
    sig = _rows64(ab32, list(range(T)), 1.0)[:, 5]
    abp = np.concatenate([[1.0], ab[:-1]])
    want = (1.0 - abp) / (1.0 - ab) * (1.0 - ab / abp)
    np.testing.assert_allclose(sig[1:] ** 2, want[1:], rtol=1e-12, atol=0.0)
    assert sig[0] == 0.0 and want[0] == 0.0
    # and the float32 rows are that, rounded once
    rows = sp.spaced_coefficients(ab32, list(range(T)), 1.0)
    got, s64 = rows[:, 5].double().numpy(), np.sqrt(want)
    assert np.all(np.abs(got - s64) <= (2.0 ** -24 + 1e-12) * s64)


def test_cosine_degenerate_rows():
    sp = _sp()
    ab = _alpha_bar("cosine1000")
    T = len(ab)
    assert T == 1001 and float(ab[0]) == 1.0 and 0.0 < float(ab[-1]) < 1e-30
    for eta in (0.0, 0.5, 1.0):
        rows = sp.spaced_coefficients(ab, sp.spaced_timesteps(T, 50), eta)
        assert torch.isfinite(rows).all()
        assert float(rows[-1, 0]) > 1e15 and float(rows[-1, 1]) > 1e15               # 1 / sqrt(3.75e-33): large, finite in float32
        assert float(rows[0, 3]) == 0.0 and float(rows[0, 0]) == 1.0 and float(rows[0, 1]) == 0.0     # t = 0: 1 - alpha_bar == 0
        assert float(rows[0, 5]) == 0.0 and float(rows[0, 6]) == 0.0
    one = sp.spaced_coefficients(ab, [T - 1], 1.0)
    assert torch.isfinite(one).all() and float(one[0, 4]) == 1.0


def test_zero_alpha_bar_is_refused_by_name():
    sp = _sp()
    ab = _alpha_bar("linear20_zero")
    assert float(ab[19]) == 0.0 and float(ab[18]) > 0.0
    for S in (1, 2, 5, 20):
        with pytest.raises(ValueError, match=r"timestep 19\b.*no x0 estimate.*explicit"):
            sp.spaced_coefficients(ab, sp.spaced_timesteps(20, S), 0.0)
    with pytest.raises(ValueError, match="timestep 19"):
        sp.spaced_coefficients(ab, [0, 7, 19], 1.0)
    rows = sp.spaced_coefficients(ab, range(19), 0.5)
    assert tuple(rows.shape) == (19, 8) and torch.isfinite(rows).all()


@pytest.mark.parametrize("eta", [-0.1, -1.0, float("nan")])
def test_negative_eta_is_refused(eta):
    with pytest.raises(ValueError, match="eta"):
        _sp().spaced_coefficients(_alpha_bar("linear20"), [0, 19], eta)


# ----------------------------------------------------------------------------- spaced_checkpoints
@pytest.mark.parametrize("T", [10, 20, 21, 1000, 1001])
def test_checkpoints_on_every_timestep_are_the_full_loop_rule(T):
    spc = T // 10
    assert _sp().spaced_checkpoints(T, list(range(T))) == {t for t in range(T) if t % spc == 0}


def test_checkpoints_hand_case():
    sp = _sp()
    # T = 20: multiples of 2; taus = [0, 5, 10, 14, 19]: 0 -> 0; 2, 4 -> 5; 6, 8, 10 -> 10; 12, 14 -> 14; 16, 18 -> 19
    assert sp.spaced_checkpoints(20, [0, 5, 10, 14, 19]) == {0, 5, 10, 14, 19}
    # T = 1000: multiples of 100; a walk that stops at 450 serves 0 .. 400 only
    assert sp.spaced_checkpoints(1000, [0, 30, 250, 450]) == {0, 250, 450}
    assert sp.spaced_checkpoints(20, [7]) == {7}
    assert sp.spaced_checkpoints(20, [3, 4, 5]) == {3, 4}              # 0, 2 -> 3; 4 -> 4; nothing at or above 6


# ----------------------------------------------------------------------------- surface
def test_symbols_declared_bound_and_exported():
    from rho_diffusion_amd import hip
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    declared = set(re.findall(r"\b(rho_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    if not os.path.exists(hip.LIB_PATH):
        from rho_diffusion_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in SPACED_SYMBOLS:
        assert name in declared, name
        assert name in hip.SIGNATURES, name
        assert hasattr(lib, name), name
    args = hip.SIGNATURES["rho_p_sample_step_spaced"][1]
    assert len(args) == 11 and args[5:10] == [ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_int]
    assert hip.SIGNATURES["rho_spaced_advance"][1][4] == ctypes.c_uint64 and len(hip.SIGNATURES["rho_spaced_advance"][1]) == 6
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == hip.ABI_VERSION


def _ddpm(schedule="linear20", **kw):
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.models import UNet
    cfg, xshape, _ = UNET_CASES["tiny2d"]
    return DDPM(UNet, dict(cfg), _schedule(schedule), nn.MSELoss, timesteps=20, **kw), xshape


def test_keywords_and_defaults():
    from rho_diffusion_amd.diffusion import DDPM
    p = inspect.signature(DDPM.__init__).parameters
    assert p["sampling_steps"].default is None and p["sampling_eta"].default == 0.0
    r = inspect.signature(DDPM.reverse_process).parameters
    assert list(r)[1:] == ["x_T", "conditions", "t_checkpoints", "guidance_scale", "num_steps", "eta", "clip_denoised"]
    assert r["num_steps"].default is None and r["eta"].default is None and r["clip_denoised"].default is True
    ddpm, _ = _ddpm()
    assert ddpm.sampling_steps is None and ddpm.sampling_eta == 0.0
    ddpm, _ = _ddpm(sampling_steps=5, sampling_eta=1)
    assert ddpm.sampling_steps == 5 and ddpm.sampling_eta == 1.0 and isinstance(ddpm.sampling_eta, float)


def test_host_refusals_come_before_the_device_check():
    """A CPU tensor reaches the ValueError of a bad sequence, not the RhoHipError of the device check: nothing was drawn."""
    from rho_diffusion_amd.hip import RhoHipError
    ddpm, xshape = _ddpm()
    x = torch.zeros(xshape)
    for kw in (dict(num_steps=21), dict(num_steps=0), dict(num_steps=[5, 3]), dict(num_steps=[0, 20]), dict(num_steps=5, eta=-0.5)):
        with pytest.raises(ValueError):
            ddpm.reverse_process(x, **kw)
    with pytest.raises(ValueError, match="clip_denoised"):
        ddpm.reverse_process(x, clip_denoised=False)
    assert ddpm._noise_offset == 0
    with pytest.raises(RhoHipError):
        ddpm.reverse_process(x, num_steps=5)                         # a good sequence: on to the device check
    zero, _ = _ddpm("linear20_zero", sampling_steps=5)
    with pytest.raises(ValueError, match="timestep 19"):
        zero.reverse_process(x)                                      # the attribute is the default
    with pytest.raises(RhoHipError):
        zero.reverse_process(x, num_steps=range(0, 19, 3))


def test_rows_are_cached_per_sequence_and_eta():
    ddpm, _ = _ddpm()
    a = ddpm._spaced_host(5, 0.5)
    assert ddpm._spaced_host(5, 0.5) is a and ddpm._spaced_host([0, 5, 10, 14, 19], 0.5) is a
    assert ddpm._spaced_host(5, 0.0) is not a and ddpm._spaced_host(4, 0.5) is not a
    assert a["taus"] == (0, 5, 10, 14, 19) and tuple(a["rows"].shape) == (5, 8)
