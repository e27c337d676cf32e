"""Few-step sampling on a spaced timestep sequence (DDIM, Song et al. 2021, with ``eta``): the host side of
``DDPM.reverse_process(num_steps=, eta=)``.  Pure functions, no GPU: the timestep sequence, the per-step coefficient rows read by
rho_p_sample_step_spaced, and the checkpoint rule.  The reference has no few-step sampler for its DDPM class.

The walk visits ``taus`` (strictly increasing) from the top: step k goes from t = taus[k] to taus[k-1]; step 0 goes to "t = -1",
alpha_bar = 1, and so returns the (clipped) x0 estimate.  With ab = alpha_bar[taus[k]] and abp = alpha_bar[taus[k-1]] (1 for k = 0)

    x0    = sqrt(1/ab) * x - sqrt(1/ab - 1) * eps_hat                      (clamped to [-1, 1] under clip_denoised)
    eps   = (x - sqrt(ab) * x0) / sqrt(1 - ab)                             (eps_hat itself without the clamp)
    sigma = eta * sqrt((1 - abp) / (1 - ab)) * sqrt(1 - ab / abp)
    x'    = sqrt(abp) * x0 + sqrt(1 - abp - sigma^2) * eps + sigma * z

Degenerate rows are defined here, not met in the kernel: 1 - ab == 0 (the cosine schedule's t = 0) writes 1/sqrt(1 - ab) and
sigma as 0; ab == 0 (LinearSchedule(20, 1e-3, 0.02) at t = 19) has no x0 estimate and is refused."""
from __future__ import annotations

import math
import numbers
from typing import Iterable, List, Sequence, Set, Union

import torch

__all__ = ["spaced_timesteps", "resolve_timesteps", "spaced_coefficients", "spaced_checkpoints", "ROW_WIDTH"]

ROW_WIDTH = 8       # c_recip, c_recipm1, sqrt_ab, inv_sqrt_1mab, sqrt_abp, sigma, coef_eps, pad: two 16-byte pieces per row


def spaced_timesteps(T: int, S: int) -> List[int]:
    """``S`` timesteps of a ``T``-entry schedule, evenly spaced with both ends kept: tau_i = round(i * (T-1) / (S-1)) in integer
    arithmetic (halves round up).  Strictly increasing because the spacing (T-1)/(S-1) is at least 1."""
    T, S = int(T), int(S)
    if S < 1 or S > T:
        raise ValueError(f"num_steps must lie in [1, {T}] for a schedule of {T} timesteps: got {S}")
    if S == 1:
        return [T - 1]
    return [(2 * i * (T - 1) + (S - 1)) // (2 * (S - 1)) for i in range(S)]


def resolve_timesteps(T: int, num_steps: Union[int, Iterable[int]]) -> List[int]:
    """``num_steps`` as the sampler takes it: a count (-> spaced_timesteps) or an explicit strictly increasing sequence in [0, T)."""
    if isinstance(num_steps, bool):
        raise ValueError("num_steps must be a step count or a sequence of timesteps, not a bool")
    if isinstance(num_steps, numbers.Integral):
        return spaced_timesteps(T, num_steps)
    if torch.is_tensor(num_steps):
        num_steps = num_steps.tolist()
    taus = list(num_steps)
    if not taus or any(int(t) != t for t in taus):
        raise ValueError(f"an explicit timestep sequence holds at least one integer timestep: got {taus}")
    taus = [int(t) for t in taus]
    if taus[0] < 0 or taus[-1] >= T or any(b <= a for a, b in zip(taus, taus[1:])):
        raise ValueError(f"an explicit timestep sequence must be strictly increasing and lie within [0, {T}): got {taus}")
    return taus


def spaced_coefficients(alpha_bar, taus: Sequence[int], eta: float) -> torch.Tensor:
    """float32 [S, 8] rows of rho_p_sample_step_spaced, row k for t = taus[k]: evaluated in float64 on the schedule's float32
    ``alpha_bar`` and rounded once."""
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0: got {eta}")
    ab_all = torch.as_tensor(alpha_bar).detach().to("cpu", torch.float32).double().tolist()
    taus = resolve_timesteps(len(ab_all), list(taus))
    rows = []
    ab_prev = 1.0
    for tau in taus:
        ab = ab_all[tau]
        if not ab > 0.0:
            raise ValueError(f"alpha_bar is {ab} at timestep {tau}: x_t holds no signal there and no x0 estimate exists; pass an "
                             f"explicit timestep sequence that stops below {tau} (num_steps=range(0, {tau}, stride))")
        one_m = 1.0 - ab
        if one_m == 0.0:
            inv, sigma = 0.0, 0.0
        else:
            inv = 1.0 / math.sqrt(one_m)
            sigma = eta * math.sqrt((1.0 - ab_prev) / one_m) * math.sqrt(max(1.0 - ab / ab_prev, 0.0))
        coef_eps = math.sqrt(max(1.0 - ab_prev - sigma * sigma, 0.0))
        rows.append([math.sqrt(1.0 / ab), math.sqrt(max(1.0 / ab - 1.0, 0.0)), math.sqrt(ab), inv, math.sqrt(ab_prev), sigma,
                     coef_eps, 0.0])
        ab_prev = ab
    out = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    if not torch.isfinite(out).all():
        bad = [taus[k] for k in range(len(taus)) if not torch.isfinite(out[k]).all()]
        raise ValueError(f"the coefficient rows of timesteps {bad} do not fit float32 (alpha_bar too small); stop the sequence below them")
    return out


def spaced_checkpoints(T: int, taus: Sequence[int]) -> Set[int]:
    """The timesteps after whose step reverse_process writes the next ``buffer`` slot: the full loop's rule is t % (T // 10) == 0;
    a spaced walk takes, for every such multiple m, the first visited timestep at or above it.  Equal to the full rule at S == T."""
    spc = int(T) // 10
    if spc < 1:
        raise ValueError(f"checkpoints are spaced T // 10 apart: a schedule of {T} timesteps has none")
    taus = list(taus)
    out = set()
    for m in range(0, int(T), spc):
        hit = [t for t in taus if t >= m]
        if hit:
            out.add(min(hit))
    return out
