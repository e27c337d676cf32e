"""CPU: the host side of DDPM(sampler="dpmpp_2m") / DDPM.reverse_process_with(sampler="dpmpp_2m", spacing="logsnr") - the log-SNR timestep selection and the
coefficient rows of rho_dpmpp_2m_step (diffusion/multistep.py), the accuracy the second-order rows buy, and the argument handling
that needs no GPU.

The restatements below are written independently of the code under test: the timestep rule as vectorised torch float64 on the
schedule's float32 alpha_bar, the rows in the paper's log-SNR form (sigma'/sigma, -alpha' (e^{-h} - 1) with exp, r = h_prev / h).  The
two float64 forms of a row entry agree to about 1e-12 relative, so after the single rounding to float32 they differ by at most one
unit in the last place: that is the tolerance, per finite entry, and cells that are defined (0, 1, a square root) are compared
exactly."""
import ctypes
import inspect
import math
import os

import pytest
import torch
from torch import nn

from helpers import UNET_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["epsilon", "v", "sample"]


def _ab(name: str) -> torch.Tensor:
    from rho_diffusion_amd.diffusion import CosineBetaSchedule, LinearSchedule
    if name == "linear":
        return LinearSchedule(1000)["alpha_bar_t"].float()
    if name == "cosine":
        return CosineBetaSchedule(1000)["alpha_bar_t"].float()
    return LinearSchedule(20, 1e-3, 0.02)["alpha_bar_t"].float()


def _lam64(ab32: torch.Tensor) -> torch.Tensor:
    ab = ab32.double()
    return torch.log(ab.sqrt() / (1.0 - ab).sqrt())


def _logsnr_restated(ab32: torch.Tensor, S: int):
    """The rule of the issue: finite lam only, S values evenly spaced from lam(lo) down to lam(hi), nearest timestep (the lower on a
    tie), ends pinned, bumped to strictly increasing."""
    lam = _lam64(ab32)
    idx = torch.nonzero(torch.isfinite(lam)).flatten()
    lo, hi = int(idx[0]), int(idx[-1])
    if S == 1:
        return [hi], lo, hi
    grid = lam[lo] + torch.arange(S, dtype=torch.float64) * (lam[hi] - lam[lo]) / (S - 1)
    d = (lam[idx][None, :] - grid[:, None]).abs()
    pick = idx[torch.argmin(d, dim=1)].tolist()                  # argmin: the first (lowest) index among equal minima
    pick[0], pick[-1] = lo, hi
    for i in range(1, S):
        pick[i] = max(pick[i], pick[i - 1] + 1)
    return (pick if pick[-1] <= hi else None), lo, hi            # None: the bump ran past hi, the rule refuses


@pytest.mark.parametrize("name,S", [("linear", s) for s in (1, 2, 5, 10, 50)] + [("cosine", s) for s in (1, 2, 3, 5, 10, 50)]
                         + [("linear20", s) for s in (1, 2, 5, 10, 19)])
def test_logsnr_timesteps(name, S):
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    ab = _ab(name)
    want, lo, hi = _logsnr_restated(ab, S)
    if want is None:
        # the cosine table ends in alpha_bar = 3.7e-33, lam = -37 after -6.5: every value below the middle of that gap snaps to the
        # last timestep, and the rule refuses rather than pick other timesteps than it states
        assert name != "linear" and S >= 4
        with pytest.raises(ValueError, match=f"num_steps={S}"):
            logsnr_timesteps(ab, S)
        return
    got = logsnr_timesteps(ab, S)
    assert got == want and all(isinstance(t, int) for t in got), (got, want)
    assert len(got) == S and all(b > a for a, b in zip(got, got[1:]))
    assert got[-1] == hi and (S == 1 or got[0] == lo)
    if name == "linear":
        assert (lo, hi) == (0, 999)
    if name == "cosine":                                         # alpha_bar[0] == 1 in float32: lam = +inf, never selected
        assert float(ab[0]) == 1.0 and lo >= 1 and 0 not in got
    if name == "linear20":                                       # alpha_bar[19] == 0: lam = -inf, never selected
        assert float(ab[19]) == 0.0 and (lo, hi) == (0, 18) and 19 not in got


def test_logsnr_timesteps_are_even_in_lam_and_not_in_t():
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    from rho_diffusion_amd.diffusion.spaced import spaced_timesteps
    ab = _ab("linear")
    lam = _lam64(ab)
    S = 10
    taus = logsnr_timesteps(ab, S)
    grid = lam[0] + torch.arange(S, dtype=torch.float64) * (lam[999] - lam[0]) / (S - 1)
    for i in range(1, S - 1):                                    # the nearest timestep: off its value by at most half the gap to a neighbour
        t = taus[i]
        assert abs(float(lam[t] - grid[i])) <= 0.5 * max(float(lam[t - 1] - lam[t]), float(lam[t] - lam[t + 1])), (i, t)
    h = -(lam[taus][1:] - lam[taus][:-1])
    uni = spaced_timesteps(1000, S)
    hu = -(lam[uni][1:] - lam[uni][:-1])
    assert taus != uni and float(hu.max() / hu.min()) > float(h.max() / h.min())     # uniform in t is the less even in lam


def test_logsnr_refusals():
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    ab = _ab("linear20")                                         # finite lam on 0..18
    for bad in (0, -1, 20, 21, 1000):
        with pytest.raises(ValueError, match=str(bad)):
            logsnr_timesteps(ab, bad)
    for bad in (2.5, True, None, [1, 2]):
        with pytest.raises(ValueError):
            logsnr_timesteps(ab, bad)
    with pytest.raises(ValueError):
        logsnr_timesteps(torch.tensor([1.0, 0.0]), 1)            # no timestep with a finite lam
    # lam = 2.0, 1.9, 1.8, 1.7, -2.0 and S = 4: the values 2, 2/3, -2/3, -2 snap to 0, 3, 4, 4; the bump would need timestep 5
    crowded = torch.sigmoid(2.0 * torch.tensor([2.0, 1.9, 1.8, 1.7, -2.0], dtype=torch.float64)).float()
    with pytest.raises(ValueError, match="num_steps=4"):
        logsnr_timesteps(crowded, 4)
    assert logsnr_timesteps(crowded, 3) == [0, 3, 4]


def _ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in float32 units in the last place between finite values of the same sign (0 against 0: 0)."""
    assert a.dtype == b.dtype == torch.float32
    return (a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs()


def _rows_restated(ab32: torch.Tensor, taus, kind: str) -> torch.Tensor:
    """float64 rows in the paper's log-SNR form; the edge rules of the issue applied as written there."""
    ab = ab32.double().tolist()
    S = len(taus)
    lam = [math.inf if ab[t] == 1.0 else -math.inf if ab[t] == 0.0 else math.log(math.sqrt(ab[t]) / math.sqrt(1.0 - ab[t])) for t in taus]
    hs, out = [], []
    for k in range(S):
        lam_p = math.inf if k == 0 else lam[k - 1]
        hs.append(lam_p - lam[k] if math.isfinite(lam_p) or math.isfinite(lam[k]) else math.nan)
    for k in range(S):
        a, ap = ab[taus[k]], (1.0 if k == 0 else ab[taus[k - 1]])
        if kind == "epsilon":
            conv = [math.sqrt(1.0 / a), math.sqrt(1.0 / a - 1.0)]
        elif kind == "v":
            conv = [math.sqrt(a), math.sqrt(1.0 - a)]
        else:
            conv = [0.0, 0.0]
        h = hs[k]
        if k == 0:
            step = [0.0, 1.0, 0.0]
        else:
            if math.sqrt(1.0 - ap) == 0.0:
                c_x, c_0 = 0.0, math.sqrt(ap)
            elif math.isfinite(h):
                c_x, c_0 = math.sqrt(1.0 - ap) / math.sqrt(1.0 - a), -math.sqrt(ap) * (math.exp(-h) - 1.0)
            else:
                c_x = math.sqrt(1.0 - ap) / math.sqrt(1.0 - a)
                c_0 = math.sqrt(ap) - c_x * math.sqrt(a)
            if k == S - 1 or not math.isfinite(h) or not math.isfinite(hs[k + 1]):
                step = [c_x, c_0, 0.0]
            else:
                r = hs[k + 1] / h
                step = [c_x, c_0 * (1.0 + 1.0 / (2.0 * r)), -c_0 / (2.0 * r)]
        out.append(conv + step + [0.0, 0.0, 0.0])
    return torch.tensor(out, dtype=torch.float64)


def _sequences():
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    from rho_diffusion_amd.diffusion.spaced import spaced_timesteps
    lin, cos = _ab("linear"), _ab("cosine")
    return [("linear", lin, logsnr_timesteps(lin, S)) for S in (1, 2, 5, 10, 50)] + \
           [("linear-uniform", lin, spaced_timesteps(1000, S)) for S in (5, 50)] + \
           [("cosine", cos, logsnr_timesteps(cos, S)) for S in (2, 3)] + [("cosine-explicit", cos, list(range(1, 1001, 111)))] + \
           [("cosine-from-0", cos, list(range(0, 1001, 100))), ("linear20", _ab("linear20"), list(range(19)))]


@pytest.mark.parametrize("kind", TYPES)
def test_rows_against_the_log_snr_form(kind):
    from rho_diffusion_amd.diffusion.multistep import ROW_WIDTH, dpmpp_2m_coefficients
    assert ROW_WIDTH == 8
    for name, ab, taus in _sequences():
        got = dpmpp_2m_coefficients(ab, taus, kind)
        want = _rows_restated(ab, taus, kind).to(torch.float32)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(taus), 8) and torch.isfinite(got).all(), name
        worst = int(_ulps(got, want).max())
        assert worst <= 1, (name, kind, len(taus), worst)
        assert torch.equal(got[:, 5:], torch.zeros(len(taus), 3)), name
        if len(taus) >= 5:                                       # the interior is second order: c_d1 < 0 < c_0 < c_d0, c_d0 + c_d1 = c_0
            mid = got[2:-1].double()
            assert (mid[:, 4] < 0).all() and (mid[:, 3] > 0).all(), name
            c0 = _rows_restated(ab, taus, kind)[2:-1]
            slack = 1.001 * 2.0 ** -24 * (mid[:, 3].abs() + mid[:, 4].abs())      # the two roundings to float32
            assert ((mid[:, 3] + mid[:, 4] - (c0[:, 3] + c0[:, 4])).abs() <= slack).all(), name


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


@pytest.mark.parametrize("kind", TYPES)
def test_edge_rows_cell_by_cell(kind):
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients, logsnr_timesteps
    lin = _ab("linear")
    ab = lin.double().tolist()

    def conv(a):
        return {"epsilon": [_f32(math.sqrt(1.0 / a)), _f32(math.sqrt(1.0 / a - 1.0))], "v": [_f32(math.sqrt(a)), _f32(math.sqrt(1.0 - a))],
                "sample": [0.0, 0.0]}[kind]

    taus = logsnr_timesteps(lin, 10)
    rows = dpmpp_2m_coefficients(lin, taus, kind)
    # row 0: the x0 estimate itself
    assert rows[0].tolist() == conv(ab[taus[0]]) + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    # row S-1: no history, first order: c_d0 = c_0 = alpha' - c_x alpha to one ulp, c_d1 = 0
    a, ap = ab[taus[-1]], ab[taus[-2]]
    c_x = math.sqrt(1.0 - ap) / math.sqrt(1.0 - a)
    last = rows[-1].tolist()
    assert last[:2] == conv(a) and last[2] == _f32(c_x) and last[4:] == [0.0, 0.0, 0.0, 0.0]
    assert int(_ulps(rows[-1, 3:4], torch.tensor([math.sqrt(ap) - c_x * math.sqrt(a)], dtype=torch.float64).float())) <= 1
    # S = 1
    one = dpmpp_2m_coefficients(lin, [999], kind)
    assert one.tolist() == [conv(ab[999]) + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]]
    # S = 2: both rows first order
    two = dpmpp_2m_coefficients(lin, [100, 999], kind)
    assert two[0].tolist() == conv(ab[100]) + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert float(two[1, 4]) == 0.0 and float(two[1, 3]) > 0.0 and float(two[1, 2]) == _f32(math.sqrt(1.0 - ab[100]) / math.sqrt(1.0 - ab[999]))
    # an alpha_bar_prev == 1 target at k = 1 (the cosine schedule's t = 0): c_x = 0, c_0 = alpha' = 1, first order; row 2 is second order
    cos = _ab("cosine")
    assert float(cos[0]) == 1.0
    ctaus = list(range(0, 1000, 100))
    crows = dpmpp_2m_coefficients(cos, ctaus, kind)
    a1 = cos.double().tolist()[ctaus[1]]
    assert crows[1].tolist() == conv(a1) + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert crows[0].tolist() == ([1.0, 0.0] if kind != "sample" else [0.0, 0.0]) + [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assert float(crows[2, 4]) < 0.0 and float(crows[3, 4]) < 0.0


@pytest.mark.parametrize("kind", ["v", "sample"])
def test_source_without_signal(kind):
    """LinearSchedule(20, 1e-3, 0.02): alpha_bar[19] == 0, lam = -inf, h = +inf.  Row 19 is first order with c_x = sigma', c_0 = alpha';
    row 18, whose h_prev is that h, is first order too; row 17 is second order again."""
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients
    ab32 = _ab("linear20")
    ab = ab32.double().tolist()
    assert ab[19] == 0.0 and ab[18] > 0.0
    rows = dpmpp_2m_coefficients(ab32, range(20), kind)
    assert torch.isfinite(rows).all()
    head = [0.0, 1.0] if kind == "v" else [0.0, 0.0]
    assert rows[19].tolist() == head + [_f32(math.sqrt(1.0 - ab[18])), _f32(math.sqrt(ab[18])), 0.0, 0.0, 0.0, 0.0]
    h18 = math.log(math.sqrt(ab[17] / (1.0 - ab[17]))) - math.log(math.sqrt(ab[18] / (1.0 - ab[18])))
    assert float(rows[18, 4]) == 0.0 and float(rows[18, 2]) == _f32(math.sqrt(1.0 - ab[17]) / math.sqrt(1.0 - ab[18]))
    assert int(_ulps(rows[18, 3:4], torch.tensor([-math.sqrt(ab[17]) * (math.exp(-h18) - 1.0)], dtype=torch.float64).float())) <= 1
    assert float(rows[17, 4]) < 0.0
    assert int(_ulps(rows, _rows_restated(ab32, list(range(20)), kind).float()).max()) <= 1


def test_epsilon_refuses_a_source_without_signal():
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients
    ab = _ab("linear20")
    with pytest.raises(ValueError) as a:
        dpmpp_2m_coefficients(ab, range(20), "epsilon")
    with pytest.raises(ValueError) as b:
        spaced_coefficients(ab, range(20), 0.0)
    assert str(a.value) == str(b.value) and "timestep 19" in str(a.value)
    assert torch.isfinite(dpmpp_2m_coefficients(ab, range(19), "epsilon")).all()
    with pytest.raises(ValueError, match="prediction_type"):
        dpmpp_2m_coefficients(ab, range(19), "x0")
    with pytest.raises(ValueError, match="strictly increasing"):
        dpmpp_2m_coefficients(ab, [3, 3, 5], "v")
    for bad_ab in (torch.tensor([0.9, 1.5]), torch.tensor([0.9, -0.1])):
        with pytest.raises(ValueError, match="timestep 1"):
            dpmpp_2m_coefficients(bad_ab, [0, 1], "v")


def _walk64(rows: torch.Tensor, ab, taus, s: float, second: bool) -> float:
    """x before row 0, float64 on the float32 rows, from x = 1 at taus[-1] under the analytic epsilon model of iid N(0, s^2) data:
    eps = sqrt(1 - ab) x / D, D = ab s^2 + 1 - ab.  ``second`` False folds c_d1 into c_d0 (c_d0 + c_d1 = c_0): the first-order walk
    on the same timesteps."""
    x, hist = 1.0, 0.0
    for k in range(len(taus) - 1, 0, -1):
        a_x, a_p, c_x, c_d0, c_d1 = rows[k][:5].tolist()
        a = ab[taus[k]]
        x0 = a_x * x - a_p * (math.sqrt(1.0 - a) * x / (a * s * s + 1.0 - a))
        if not second:
            c_d0, c_d1 = c_d0 + c_d1, 0.0
        x, hist = c_x * x + c_d0 * x0 + c_d1 * hist, x0
    return x


@pytest.mark.parametrize("s", [0.5, 2.0])
@pytest.mark.parametrize("S", [10, 20, 50])
def test_second_order_rows_are_at_least_four_times_as_accurate(S, s):
    """The probability-flow ODE of iid N(0, s^2) data has the closed form x_t = x_T sqrt(D_t / D_T).  On log-SNR spaced timesteps of
    LinearSchedule(1000) the 2M walk's relative error at taus[0] is at most a quarter of the first-order walk's."""
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients, logsnr_timesteps
    ab32 = _ab("linear")
    ab = ab32.double().tolist()
    taus = logsnr_timesteps(ab32, S)
    rows = dpmpp_2m_coefficients(ab32, taus, "epsilon").double()
    D = lambda t: ab[t] * s * s + 1.0 - ab[t]                    # noqa: E731
    exact = math.sqrt(D(taus[0]) / D(taus[-1]))
    e2 = abs(_walk64(rows, ab, taus, s, True) - exact) / exact
    e1 = abs(_walk64(rows, ab, taus, s, False) - exact) / exact
    print(f"S={S} s={s}: first order {e1:.3e}, 2M {e2:.3e}, ratio {e1 / e2:.2f}")
    assert e1 > 1e-2 and e2 <= 0.25 * e1, (S, s, e1, e2)


# ----------------------------------------------------------------------------- DDPM(sampler=, sampling_spacing=) without a GPU
def _ddpm(**kw):
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    cfg, xshape, _ = UNET_CASES["tiny2d"]
    return DDPM(UNet, dict(cfg), LinearSchedule(20, 1e-3, 0.02), nn.MSELoss, timesteps=20, **kw), xshape


def test_constructor_and_signature():
    from rho_diffusion_amd.diffusion import DDPM
    p = inspect.signature(DDPM.__init__).parameters
    assert p["sampler"].default == "ddim" and p["sampling_spacing"].default is None
    names = ["self", "x_T", "conditions", "t_checkpoints", "guidance_scale", "num_steps", "eta", "clip_denoised"]
    assert list(inspect.signature(DDPM.reverse_process).parameters) == names          # the reference's method keeps its keywords
    q = inspect.signature(DDPM.reverse_process_with).parameters
    assert list(q) == names + ["sampler", "spacing"] and q["sampler"].default is None and q["spacing"].default is None
    ddpm, _ = _ddpm()
    assert ddpm.sampler == "ddim" and ddpm.sampling_spacing is None
    ddpm, _ = _ddpm(sampler="dpmpp_2m", sampling_spacing="logsnr")
    assert ddpm.sampler == "dpmpp_2m" and ddpm.sampling_spacing == "logsnr"
    for kw in (dict(sampler="euler"), dict(sampler=None), dict(sampler=2), dict(sampling_spacing="karras"), dict(sampling_spacing=1)):
        with pytest.raises(ValueError, match="sampler|spacing"):
            _ddpm(**kw)


def test_spaced_host_by_sampler_and_spacing():
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients, logsnr_timesteps
    from rho_diffusion_amd.diffusion.prediction import spaced_pred_coefficients
    from rho_diffusion_amd.diffusion.spaced import spaced_timesteps
    ddpm, _ = _ddpm()
    ab = ddpm.schedule["alpha_bar_t"].float()
    log5, uni5 = tuple(logsnr_timesteps(ab, 5)), tuple(spaced_timesteps(20, 5))
    assert log5 != uni5 and log5[-1] == 18 and uni5[-1] == 19
    a = ddpm._spaced_host(5, 0.0, "dpmpp_2m")                    # spacing None: logsnr for dpmpp_2m
    assert a["taus"] == log5 and a["sampler"] == "dpmpp_2m" and torch.equal(a["rows"], dpmpp_2m_coefficients(ab, log5, "epsilon"))
    assert ddpm._spaced_host(5, 0.0, "dpmpp_2m", "logsnr") is a and ddpm._spaced_host(list(log5), 0.0, "dpmpp_2m") is a
    b = ddpm._spaced_host(5, 0.0, "ddim", "logsnr")              # the same timesteps under the first-order update: another entry
    assert b is not a and b["taus"] == log5 and b["sampler"] == "ddim"
    assert torch.equal(b["rows"], spaced_pred_coefficients(ab, log5, 0.0, "epsilon"))
    with pytest.raises(ValueError, match="timestep 19"):         # uniform spacing ends at t = 19, alpha_bar == 0: epsilon refuses
        ddpm._spaced_host(5, 0.0, "dpmpp_2m", "uniform")
    assert sorted(k[3] for k in ddpm._spaced_cache) == ["ddim", "dpmpp_2m"] and all(k[2] == "epsilon" for k in ddpm._spaced_cache)
    ddpm.prediction_type = "v"
    e = ddpm._spaced_host(5, 0.0, "dpmpp_2m", "uniform")
    assert e["taus"] == uni5 and torch.equal(e["rows"], dpmpp_2m_coefficients(ab, uni5, "v"))
    d = ddpm._spaced_host(5, 0.5)                                # the defaults are those of before: ddim on spaced_timesteps
    assert d["taus"] == uni5 and d["sampler"] == "ddim" and torch.equal(d["rows"], spaced_pred_coefficients(ab, uni5, 0.5, "v"))
    assert ddpm._spaced_host(5, 0.5, "ddim", "uniform") is d


def test_sampling_refusals_come_before_any_gpu_work():
    from rho_diffusion_amd.hip import RhoHipError
    eps, xshape = _ddpm()
    x = torch.zeros(xshape)
    with pytest.raises(ValueError, match="eta"):
        eps.reverse_process_with(x, num_steps=5, sampler="dpmpp_2m", eta=0.3)
    with pytest.raises(ValueError, match="num_steps"):
        eps.reverse_process_with(x, sampler="dpmpp_2m")
    with pytest.raises(ValueError, match="spacing"):
        eps.reverse_process_with(x, num_steps=[0, 5, 10], sampler="dpmpp_2m", spacing="logsnr")
    with pytest.raises(ValueError, match="spacing"):
        eps.reverse_process_with(x, num_steps=[0, 5, 10], spacing="uniform")
    with pytest.raises(ValueError, match="sampler"):
        eps.reverse_process_with(x, num_steps=5, sampler="heun")
    with pytest.raises(ValueError, match="spacing"):
        eps.reverse_process_with(x, num_steps=5, spacing="cosine")
    noisy, _ = _ddpm(sampler="dpmpp_2m", sampling_eta=0.5, sampling_steps=5)
    with pytest.raises(ValueError, match="eta"):                 # the attribute's eta is refused like the argument's
        noisy.reverse_process(x)
    assert eps._noise_offset == 0 and noisy._noise_offset == 0
    v, _ = _ddpm(prediction_type="v", sampler="dpmpp_2m")
    for kw in (dict(), dict(num_steps=5), dict(num_steps=range(20)), dict(num_steps=5, spacing="uniform"), dict(num_steps=5, eta=0.0)):
        with pytest.raises(RhoHipError):                         # all host checks pass: the first GPU requirement refuses
            v.reverse_process_with(x, **kw)
    for kw in (dict(num_steps=5, sampler="dpmpp_2m"), dict(num_steps=5, spacing="logsnr"), dict(num_steps=[0, 5, 18], sampler="dpmpp_2m")):
        with pytest.raises(RhoHipError):
            eps.reverse_process_with(x, **kw)
    attr, _ = _ddpm(sampling_spacing="logsnr")                   # a sequence given with the call outranks the attribute's spacing
    with pytest.raises(RhoHipError):
        attr.reverse_process(x, num_steps=[0, 5, 18])
    both, _ = _ddpm(sampling_spacing="logsnr", sampling_steps=[0, 5, 18])
    with pytest.raises(ValueError, match="spacing"):
        both.reverse_process(x)


def test_library_exports_and_binding():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    if not os.path.exists(hip.LIB_PATH):
        from rho_diffusion_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(lib, "rho_dpmpp_2m_step") and len(hip.SIGNATURES["rho_dpmpp_2m_step"][1]) == 12
    assert callable(ops.dpmpp_2m_step)
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    assert "int rho_dpmpp_2m_step(float* x, const float* pred, float* hist, const float* rows, const int32_t* k_dev, int32_t S" in header
    assert hip.ABI_VERSION == 10
