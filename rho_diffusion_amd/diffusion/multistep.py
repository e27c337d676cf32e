"""DPM-Solver++(2M) (Lu et al. 2022) on a spaced timestep sequence and the log-SNR timestep selection it needs: the host side of
``DDPM(sampler="dpmpp_2m", sampling_spacing="logsnr")`` and ``reverse_process_with(sampler=, spacing=)``.  Pure functions, no GPU, in
the manner of spaced.py and prediction.py: the timestep sequence and the per-step coefficient rows read by rho_dpmpp_2m_step.  The
reference has no few-step sampler.

With ab = alpha_bar[t], alpha = sqrt(ab), sigma = sqrt(1 - ab) and the half log-SNR lam = log(alpha / sigma), the walk of spaced.py
(step k from t = taus[k] to taus[k-1], primes for the target, ab' = 1 for k = 0) takes the data-prediction multistep update

    h  = lam' - lam                         r = h_prev / h     (h_prev: the h of the step before, row k + 1)
    D  = (1 + 1/(2r)) x0_k - 1/(2r) x0_{k+1}
    x' = (sigma'/sigma) x + alpha' (1 - e^{-h}) D

where x0_k is the x0 estimate at taus[k] and x0_{k+1} the one the step before left behind.  It is second order in h only where the
steps are of similar size in lam: on timesteps uniform in t the ratio r runs away near t = 0 and the extrapolation can be worse than
the first-order update, hence logsnr_timesteps.

Degenerate rows are defined here, not met in the kernel: a step whose h or h_prev is not finite (an alpha_bar == 0 source, an
alpha_bar == 1 target) or whose r is not a finite positive number is first order, sigma' == 0 writes c_x = 0, and row 0 returns the
x0 estimate as on the DDIM walk."""
from __future__ import annotations

import math
import numbers
from typing import List, Sequence

import torch

from .prediction import resolve_prediction_type
from .spaced import resolve_timesteps

__all__ = ["logsnr_timesteps", "dpmpp_2m_coefficients", "ROW_WIDTH", "SAMPLERS", "SPACINGS"]

ROW_WIDTH = 8       # a_x, a_p, c_x, c_d0, c_d1, 0, 0, 0: two 16-byte pieces per row
SAMPLERS = ("ddim", "dpmpp_2m")
SPACINGS = ("uniform", "logsnr")


def _alpha_bar64(alpha_bar) -> List[float]:
    return torch.as_tensor(alpha_bar).detach().to("cpu", torch.float32).double().flatten().tolist()


def _lam(ab: float) -> float:
    """log(sqrt(ab) / sqrt(1 - ab)); +inf at ab == 1, -inf at ab == 0."""
    if ab >= 1.0:
        return math.inf
    if ab <= 0.0:
        return -math.inf
    return math.log(math.sqrt(ab) / math.sqrt(1.0 - ab))


def logsnr_timesteps(alpha_bar, S: int) -> List[int]:
    """``S`` strictly increasing timesteps, evenly spaced in lam(t) = log(sqrt(ab) / sqrt(1 - ab)) (float64 on the float32 table).

    Only timesteps with a finite lam (0 < ab < 1) are considered; lo and hi are the first and the last of them.  Take S values evenly
    spaced from lam(lo) down to lam(hi), v_i = lam(lo) + i (lam(hi) - lam(lo)) / (S - 1); for each the timestep whose lam is nearest,
    the lower timestep on a tie; pin the first entry to lo and the last to hi; walk upwards and raise an entry to its predecessor plus
    one where it does not exceed it.  S == 1 gives [hi].  ValueError if S lies outside [1, hi - lo + 1] or the walk pushes an entry
    past hi."""
    ab_all = _alpha_bar64(alpha_bar)
    if isinstance(S, bool) or not isinstance(S, numbers.Integral):
        raise ValueError(f"num_steps must be a step count for log-SNR spacing: got {S!r}")
    S = int(S)
    finite = [t for t, ab in enumerate(ab_all) if 0.0 < ab < 1.0]
    if not finite:
        raise ValueError("log-SNR spacing needs a timestep with 0 < alpha_bar < 1: the schedule has none")
    lo, hi = finite[0], finite[-1]
    if S < 1 or S > hi - lo + 1:
        raise ValueError(f"num_steps must lie in [1, {hi - lo + 1}] for log-SNR spacing over the timesteps {lo}..{hi}: got {S}")
    if S == 1:
        return [hi]
    lam = {t: _lam(ab_all[t]) for t in finite}
    top, bottom = lam[lo], lam[hi]
    taus = []
    for i in range(S):
        v = top + i * (bottom - top) / (S - 1)
        best, best_d = lo, math.inf
        for t in finite:                                         # ascending: a tie keeps the lower timestep
            d = abs(lam[t] - v)
            if d < best_d:
                best, best_d = t, d
        taus.append(best)
    taus[0], taus[-1] = lo, hi
    for i in range(1, S):
        if taus[i] <= taus[i - 1]:
            taus[i] = taus[i - 1] + 1
    if taus[-1] > hi or any(b <= a for a, b in zip(taus, taus[1:])):
        raise ValueError(f"num_steps={S} log-SNR spaced timesteps do not fit below timestep {hi} as a strictly increasing sequence "
                         "(a gap in log-SNR at the end of the schedule draws several of them to its last timestep); pass an explicit "
                         "timestep sequence")
    return taus


def dpmpp_2m_coefficients(alpha_bar, taus: Sequence[int], prediction_type) -> torch.Tensor:
    """float32 [S, 8] rows of rho_dpmpp_2m_step, row k for the step from t = taus[k] to taus[k-1] (ab_prev = 1 for k = 0):
    {a_x, a_p, c_x, c_d0, c_d1, 0, 0, 0}, evaluated in float64 on the schedule's float32 ``alpha_bar`` and rounded once.

    x0 = fma(a_x, x, -(a_p p)): "epsilon" a_x = sqrt(1/ab), a_p = sqrt(1/ab - 1), ab == 0 refused as spaced_coefficients refuses it;
    "v" a_x = sqrt(ab), a_p = sqrt(1 - ab), ab == 0 a row like any other; "sample" x0 = p, a_x = a_p = 0.
    c_x = sigma'/sigma, c_0 = alpha' (1 - e^{-h}) (= alpha' - c_x alpha where h is not finite), c_d0 = c_0 (1 + 1/(2r)),
    c_d1 = -c_0 / (2r).  First order (c_d0 = c_0, c_d1 = 0): row S-1, row 0, and any row whose h or h_prev is not finite or whose
    r = h_prev / h is not a finite positive number (two equal alpha_bar).  sigma' == 0: c_x = 0, c_0 = alpha'.  Row 0 is always
    {a_x, a_p, 0, 1, 0}: the last step returns the x0 estimate."""
    kind = resolve_prediction_type(prediction_type)
    ab_all = _alpha_bar64(alpha_bar)
    taus = resolve_timesteps(len(ab_all), list(taus))
    S = len(taus)
    base = []                                                    # per row: a_x, a_p, c_x, c_0, h
    ab_prev = 1.0
    for tau in taus:
        ab = ab_all[tau]
        if not 0.0 <= ab <= 1.0:
            raise ValueError(f"alpha_bar is {ab} at timestep {tau}: it must lie in [0, 1]")
        if kind == "epsilon":
            if not ab > 0.0:
                raise ValueError(f"alpha_bar is {ab} at timestep {tau}: x_t holds no signal there and no x0 estimate exists; pass an "
                                 f"explicit timestep sequence that stops below {tau} (num_steps=range(0, {tau}, stride))")
            a_x, a_p = math.sqrt(1.0 / ab), math.sqrt(max(1.0 / ab - 1.0, 0.0))
        elif kind == "v":
            a_x, a_p = math.sqrt(ab), math.sqrt(max(1.0 - ab, 0.0))
        else:
            a_x, a_p = 0.0, 0.0
        alpha, sigma = math.sqrt(ab), math.sqrt(1.0 - ab)
        alpha_p, sigma_p = math.sqrt(ab_prev), math.sqrt(1.0 - ab_prev)
        h = _lam(ab_prev) - _lam(ab)                             # nan for inf - inf: not finite either way
        if sigma_p == 0.0:
            c_x, c_0 = 0.0, alpha_p
        else:
            c_x = sigma_p / sigma
            c_0 = -alpha_p * math.expm1(-h) if math.isfinite(h) else alpha_p - c_x * alpha
        base.append((a_x, a_p, c_x, c_0, h))
        ab_prev = ab
    rows = []
    for k, (a_x, a_p, c_x, c_0, h) in enumerate(base):
        c_d0, c_d1 = c_0, 0.0
        if k == 0:
            c_x, c_d0 = 0.0, 1.0
        elif k < S - 1:
            h_prev = base[k + 1][4]
            if math.isfinite(h) and math.isfinite(h_prev) and h > 0.0 and h_prev > 0.0:
                r = h_prev / h
                if math.isfinite(r) and r > 0.0:
                    c_d0, c_d1 = c_0 * (1.0 + 1.0 / (2.0 * r)), -c_0 / (2.0 * r)
        rows.append([a_x, a_p, c_x, c_d0, c_d1, 0.0, 0.0, 0.0])
    out = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    if not torch.isfinite(out).all():
        bad = [taus[k] for k in range(S) if not torch.isfinite(out[k]).all()]
        raise ValueError(f"the coefficient rows of timesteps {bad} do not fit float32 (alpha_bar too small); stop the sequence below them")
    return out
