"""What the backbone predicts and how the timesteps are weighted: the host side of ``DDPM(prediction_type=, snr_gamma=)``.  Pure
functions, no GPU, in the manner of spaced.py: the names of the objectives, the min-SNR-gamma weight table read by rho_pred_loss_ws
and the per-step coefficient rows read by rho_p_sample_step_spaced_pred.  The reference's DDPM predicts the noise and weights every
timestep alike.

With ab = alpha_bar[t], x_t = sqrt(ab) x0 + sqrt(1 - ab) eps, the three objectives regress the backbone onto

    epsilon   eps                                     (Ho et al. 2020, the reference)
    v         sqrt(ab) eps - sqrt(1 - ab) x0          (Salimans & Ho 2022)
    sample    x0

and min-SNR-gamma (Hang et al. 2023) scales the squared error of timestep t by a weight that caps the x0-space weight snr(t) at
gamma, snr = ab / (1 - ab): in the units of each objective

    epsilon   min(snr, gamma) / snr          v   min(snr, gamma) / (snr + 1)          sample   min(snr, gamma)

The ends of the table are defined here: 1 - ab == 0 (snr = inf) gives 0, 0, gamma; ab == 0 (snr = 0) gives 1 (the limit), 0, 0.

The v and sample walks need no division by sqrt(ab): x0 = sqrt(ab) x - sqrt(1 - ab) v, or the prediction itself.  Their rows are
therefore defined at ab == 0 as well, where the epsilon walk has no x0 estimate and refuses (spaced.py)."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .spaced import resolve_timesteps, spaced_coefficients

__all__ = ["PREDICTION_TYPES", "PRED_EPSILON", "PRED_V", "PRED_SAMPLE", "resolve_prediction_type", "check_snr_gamma",
           "min_snr_weights", "spaced_pred_coefficients"]

PRED_EPSILON, PRED_V, PRED_SAMPLE = 0, 1, 2                      # RHO_PRED_* of include/rho_hip.h
PREDICTION_TYPES = {"epsilon": PRED_EPSILON, "v": PRED_V, "sample": PRED_SAMPLE}
_ALIASES = {"v_prediction": "v"}


def resolve_prediction_type(name) -> str:
    """The canonical name of an objective: "epsilon", "v" (alias "v_prediction") or "sample"."""
    if isinstance(name, str):
        name = _ALIASES.get(name, name)
        if name in PREDICTION_TYPES:
            return name
    raise ValueError(f"prediction_type must be one of 'epsilon', 'v' (or 'v_prediction'), 'sample': got {name!r}")


def check_snr_gamma(gamma) -> Optional[float]:
    """``gamma`` as a float, None kept: a finite number greater than 0, else ValueError."""
    if gamma is None:
        return None
    if isinstance(gamma, bool):
        raise ValueError("snr_gamma must be a finite number greater than 0 or None, not a bool")
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"snr_gamma must be a finite number greater than 0 or None: got {gamma!r}") from None
    if not (math.isfinite(g) and g > 0.0):
        raise ValueError(f"snr_gamma must be a finite number greater than 0 or None: got {gamma!r}")
    return g


def min_snr_weights(alpha_bar, prediction_type, gamma) -> Optional[torch.Tensor]:
    """float32 [T] loss weights of min-SNR-gamma for ``prediction_type``, evaluated in float64 on the schedule's float32
    ``alpha_bar`` and rounded once.  ``gamma`` None: no table (None), every timestep weighs 1."""
    kind = resolve_prediction_type(prediction_type)
    gamma = check_snr_gamma(gamma)
    if gamma is None:
        return None
    ab_all = torch.as_tensor(alpha_bar).detach().to("cpu", torch.float32).double().flatten().tolist()
    out = []
    for ab in ab_all:
        one_m = 1.0 - ab
        if one_m == 0.0:                                         # snr = inf
            w = gamma if kind == "sample" else 0.0
        elif ab == 0.0:                                          # snr = 0: min(snr, gamma) / snr -> 1
            w = 1.0 if kind == "epsilon" else 0.0
        else:
            snr = ab / one_m
            capped = min(snr, gamma)
            w = capped / snr if kind == "epsilon" else capped / (snr + 1.0) if kind == "v" else capped
        out.append(w)
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def spaced_pred_coefficients(alpha_bar, taus: Sequence[int], eta: float, prediction_type) -> torch.Tensor:
    """float32 [S, 8] rows of a spaced walk for ``prediction_type``.  "epsilon": spaced_coefficients(alpha_bar, taus, eta) unchanged
    (rho_p_sample_step_spaced).  "v" / "sample": the rows of rho_p_sample_step_spaced_pred, row k for t = taus[k],
    {sqrt_ab, sqrt_1mab, inv_sqrt_1mab, sqrt_abp, sigma, coef_eps, 0, 0} with sigma and coef_eps by the rules of spaced_coefficients,
    inv_sqrt_1mab and sigma 0 where 1 - ab == 0; ab == 0 is a row like any other.  Evaluated in float64 on the schedule's float32
    ``alpha_bar`` and rounded once."""
    kind = resolve_prediction_type(prediction_type)
    if kind == "epsilon":
        return spaced_coefficients(alpha_bar, taus, eta)
    eta = float(eta)
    if not eta >= 0.0:
        raise ValueError(f"eta must be >= 0: got {eta}")
    ab_all = torch.as_tensor(alpha_bar).detach().to("cpu", torch.float32).double().tolist()
    taus = resolve_timesteps(len(ab_all), list(taus))
    rows = []
    ab_prev = 1.0
    for tau in taus:
        ab = ab_all[tau]
        if not 0.0 <= ab <= 1.0:
            raise ValueError(f"alpha_bar is {ab} at timestep {tau}: it must lie in [0, 1]")
        one_m = 1.0 - ab
        if one_m == 0.0:
            inv, sigma = 0.0, 0.0
        else:
            inv = 1.0 / math.sqrt(one_m)
            ratio = ab / ab_prev if ab_prev > 0.0 else 1.0       # two timesteps without signal: no step between them, sigma = 0
            sigma = eta * math.sqrt((1.0 - ab_prev) / one_m) * math.sqrt(max(1.0 - ratio, 0.0))
        coef_eps = math.sqrt(max(1.0 - ab_prev - sigma * sigma, 0.0))
        rows.append([math.sqrt(ab), math.sqrt(one_m), inv, math.sqrt(ab_prev), sigma, coef_eps, 0.0, 0.0])
        ab_prev = ab
    out = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
    if not torch.isfinite(out).all():
        bad = [taus[k] for k in range(len(taus)) if not torch.isfinite(out[k]).all()]
        raise ValueError(f"the coefficient rows of timesteps {bad} do not fit float32; stop the sequence below them")
    return out
