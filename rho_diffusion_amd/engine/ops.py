"""Tensor-level wrappers over the C ABI (include/rho_hip.h): shape/dtype checks on the host,
raw device pointers into the kernels.  All functions enqueue on the current torch stream and
return torch tensors that own the device memory.  No arithmetic happens in PyTorch here."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence, Tuple

import torch

from .. import hip
from ..hip import ConvDesc, RhoHipError, check, dtype_code, ptr, stream

Tensor = torch.Tensor


def _f32c(t: Tensor, name: str) -> Tensor:
    hip.require_gpu(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RhoHipError(f"{name} must be contiguous float32, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def spatial5(shape: Sequence[int]) -> Tuple[int, int, int]:
    """(D, H, W) of a 1/2/3-D spatial shape (missing leading axes are 1)."""
    s = list(shape)
    while len(s) < 3:
        s.insert(0, 1)
    return int(s[0]), int(s[1]), int(s[2])


def elem_chunk(dtype: torch.dtype) -> int:
    """channels per 64-byte chunk: the conv kernel's channel granularity."""
    return 32 if dtype == torch.bfloat16 else 16


# ----------------------------------------------------------------------------- diffusion loops
def q_sample(x0: Tensor, eps: Tensor, t: Tensor, alpha_bar: Tensor, out: Optional[Tensor] = None,
             nan_flag: Optional[Tensor] = None) -> Tensor:
    x0, eps, alpha_bar = _f32c(x0, "x0"), _f32c(eps, "eps"), _f32c(alpha_bar, "alpha_bar")
    if t.dtype != torch.int64 or not t.is_cuda:
        raise RhoHipError("t must be an int64 GPU tensor")
    out = torch.empty_like(x0) if out is None else out
    B = x0.shape[0]
    check(hip.lib().rho_q_sample(ptr(x0), ptr(eps), ptr(out), ptr(alpha_bar), ptr(t), B, x0.numel() // B, alpha_bar.numel(),
                                 ptr(nan_flag), stream()), "rho_q_sample")
    return out


def _step_operands(x: Tensor, pred: Tensor, side: Optional[Tensor], rows: Tensor, idx_dev: Tensor, scale: Optional[float],
                   names: Sequence[str] = ("x", "pred", "z", "rows", "k_dev"), width: int = 8) -> Tuple[int, bool]:
    """The operand checks of the five reverse-process updates, (n, guided): ``x`` / ``pred`` contiguous float32 holding one row of n
    elements (``scale`` None) or the two rows of the doubled batch (guided), the optional side operand (z or hist) one row of n,
    ``rows`` float32 [S, ``width``], ``idx_dev`` the int32[1] device scalar that picks the row.  ``names``: theirs in the caller."""
    xn, pn, sn, rn, kn = names
    _f32c(x, xn), _f32c(pred, pn), _f32c(rows, rn)
    if side is not None:
        _f32c(side, sn)
    if rows.dim() != 2 or rows.shape[1] != width or rows.shape[0] < 1:
        raise RhoHipError(f"{rn} must be float32 [S, {width}], got {tuple(rows.shape)}")
    guided = scale is not None
    n = x.numel() // 2 if guided else x.numel()
    if n < 1 or x.numel() != (2 * n if guided else n) or pred.numel() != x.numel() or (side is not None and side.numel() != n):
        raise RhoHipError(f"{xn} / {pn} hold {'two rows' if guided else 'one row'} of n elements and {sn} one: got {x.numel()}, "
                          f"{pred.numel()}, {None if side is None else side.numel()}")
    if idx_dev.dtype != torch.int32 or not idx_dev.is_cuda or idx_dev.numel() != 1:
        raise RhoHipError(f"{kn} must be int32[1] on the GPU")
    return n, guided


def p_sample_step(x: Tensor, eps_hat: Tensor, z: Optional[Tensor], coef_table: Tensor, t_dev: Tensor) -> Tensor:
    n, _ = _step_operands(x, eps_hat, z, coef_table, t_dev, None, ("x", "eps_hat", "z", "coef_table", "t_dev"), 3)
    check(hip.lib().rho_p_sample_step(ptr(x), ptr(eps_hat), ptr(z), ptr(coef_table), ptr(t_dev), n, stream()), "rho_p_sample_step")
    return x


def p_sample_step_cfg(x2: Tensor, eps2: Tensor, z: Optional[Tensor], coef_table: Tensor, t_dev: Tensor, scale: float) -> Tensor:
    """One guided reverse update (rho_p_sample_step_cfg).  ``x2`` [2B, ...]: x_t and its copy; ``eps2`` [2B, ...]: the conditional
    and the null-condition prediction; ``z`` [B, ...] or None.  Both halves of ``x2`` receive the update."""
    n, _ = _step_operands(x2, eps2, z, coef_table, t_dev, float(scale), ("x2", "eps2", "z", "coef_table", "t_dev"), 3)
    check(hip.lib().rho_p_sample_step_cfg(ptr(x2), ptr(eps2), ptr(z), ptr(coef_table), ptr(t_dev), float(scale), n, stream()),
          "rho_p_sample_step_cfg")
    return x2


def p_sample_step_spaced(x: Tensor, eps_hat: Tensor, z: Optional[Tensor], rows: Tensor, k_dev: Tensor, scale: Optional[float] = None,
                         clip: bool = True) -> Tensor:
    """One reverse update of the spaced walk (rho_p_sample_step_spaced): row ``*k_dev`` of ``rows`` [S, 8].  ``scale`` None: ``x`` and
    ``eps_hat`` hold the sample and its prediction; a float: the guided form, both hold the doubled batch [2B, ...] and both halves
    of ``x`` receive the update.  ``z`` [B, ...] or None."""
    n, guided = _step_operands(x, eps_hat, z, rows, k_dev, scale, ("x", "eps_hat", "z", "rows", "k_dev"))
    check(hip.lib().rho_p_sample_step_spaced(ptr(x), ptr(eps_hat), ptr(z), ptr(rows), ptr(k_dev), rows.shape[0], n, int(guided),
                                             float(scale) if guided else 0.0, int(bool(clip)), stream()), "rho_p_sample_step_spaced")
    return x


def p_sample_step_spaced_pred(x: Tensor, pred: Tensor, z: Optional[Tensor], rows: Tensor, k_dev: Tensor, pred_type: int,
                              scale: Optional[float] = None, clip: bool = True) -> Tensor:
    """One reverse update of the spaced walk of a v- or x0-predicting backbone (rho_p_sample_step_spaced_pred): row ``*k_dev`` of
    ``rows`` [S, 8] as spaced_pred_coefficients writes them, ``pred_type`` 1 (v) or 2 (sample).  ``scale`` / ``z`` / ``clip`` as in
    p_sample_step_spaced."""
    if pred_type not in (1, 2):
        raise RhoHipError(f"pred_type must be 1 (v) or 2 (sample), got {pred_type}: epsilon takes p_sample_step_spaced")
    n, guided = _step_operands(x, pred, z, rows, k_dev, scale)
    check(hip.lib().rho_p_sample_step_spaced_pred(ptr(x), ptr(pred), ptr(z), ptr(rows), ptr(k_dev), rows.shape[0], n, int(guided),
                                                  float(scale) if guided else 0.0, int(bool(clip)), int(pred_type), stream()),
          "rho_p_sample_step_spaced_pred")
    return x


def dpmpp_2m_step(x: Tensor, pred: Tensor, hist: Tensor, rows: Tensor, k_dev: Tensor, pred_type: int, scale: Optional[float] = None,
                  clip: bool = True) -> Tensor:
    """One step of DPM-Solver++(2M) on the spaced walk (rho_dpmpp_2m_step): row ``*k_dev`` of ``rows`` [S, 8] as
    dpmpp_2m_coefficients writes them, ``pred_type`` 0 (epsilon), 1 (v) or 2 (sample).  ``hist`` [B, ...] holds the x0 estimate of the
    step before - one row also under guidance, read only by a second-order row - and receives this step's.  ``scale`` / ``clip`` as in
    p_sample_step_spaced."""
    if pred_type not in (0, 1, 2):
        raise RhoHipError(f"pred_type must be 0 (epsilon), 1 (v) or 2 (sample), got {pred_type}")
    n, guided = _step_operands(x, pred, _f32c(hist, "hist"), rows, k_dev, scale, ("x", "pred", "hist", "rows", "k_dev"))
    check(hip.lib().rho_dpmpp_2m_step(ptr(x), ptr(pred), ptr(hist), ptr(rows), ptr(k_dev), rows.shape[0], n, int(guided),
                                      float(scale) if guided else 0.0, int(bool(clip)), int(pred_type), stream()),
          "rho_dpmpp_2m_step")
    return x


def spaced_advance(k_dev: Tensor, t_dev: Tensor, taus: Tensor, offset_dev: Optional[Tensor], delta: int) -> None:
    """k <- k - 1, t <- taus[k] while k >= 0, offset += delta (rho_spaced_advance): the loop state of the spaced walk."""
    for name, t in (("k_dev", k_dev), ("t_dev", t_dev)):
        if t.dtype != torch.int32 or not t.is_cuda or t.numel() != 1:
            raise RhoHipError(f"{name} must be int32[1] on the GPU")
    if taus.dtype != torch.int32 or not taus.is_cuda or taus.dim() != 1 or not taus.is_contiguous() or taus.numel() < 1:
        raise RhoHipError("taus must be a contiguous int32 [S] GPU tensor")
    if offset_dev is not None and (offset_dev.dtype != torch.int64 or not offset_dev.is_cuda or offset_dev.numel() != 1):
        raise RhoHipError("offset_dev must be int64[1] on the GPU or None")
    check(hip.lib().rho_spaced_advance(ptr(k_dev), ptr(t_dev), ptr(taus), ptr(offset_dev), delta, stream()), "rho_spaced_advance")


def q_sample_coef(x0: Tensor, eps: Tensor, t: Tensor, coef_a: Tensor, coef_b: Tensor, out: Optional[Tensor] = None,
                  err_flag: Optional[Tensor] = None) -> Tensor:
    """x_t = a[t] * x0 + b[t] * eps with explicit float32 tables (GaussianDiffusionPipeline.q_sample)."""
    x0, eps, coef_a, coef_b = _f32c(x0, "x0"), _f32c(eps, "eps"), _f32c(coef_a, "coef_a"), _f32c(coef_b, "coef_b")
    if t.dtype != torch.int64 or not t.is_cuda:
        raise RhoHipError("t must be an int64 GPU tensor")
    out = torch.empty_like(x0) if out is None else out
    B = x0.shape[0]
    check(hip.lib().rho_q_sample_coef(ptr(x0), ptr(eps), ptr(out), ptr(coef_a), ptr(coef_b), ptr(t), B, x0.numel() // B,
                                      min(coef_a.numel(), coef_b.numel()), ptr(err_flag), stream()), "rho_q_sample_coef")
    return out


def quantile_workspace(batch: int, device, ws: Optional[Tensor] = None) -> Tensor:
    need = hip.lib().rho_abs_quantile_workspace_bytes(batch)
    if ws is None or ws.device != torch.device(device) or ws.numel() * ws.element_size() < need:
        ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=device)
    return ws


def _sample_rows(v: Tensor, name: str, batch: int, n: int) -> int:
    """Per-sample stride of ``v``: a float32 GPU tensor whose sample b is the contiguous block of n elements at v[b] (a contiguous
    tensor, or one half of a contiguous [B, 2C, ...] learned-variance output sliced along dim 1).  n for a contiguous tensor."""
    hip.require_gpu(v, name)
    if v.dtype != torch.float32 or v.dim() < 1 or v.shape[0] != batch or v.numel() != batch * n or not (v.is_contiguous() or v[0].is_contiguous()):
        raise RhoHipError(f"{name} must be float32 [{batch}, ...] with {n} contiguous elements per sample, got {v.dtype} {tuple(v.shape)} "
                          f"strides {v.stride()}")
    return n if batch == 1 or v.is_contiguous() else v.stride(0)


def abs_quantile(x: Tensor, q: float, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """Per-sample torch.quantile(|x|.flatten(1), q) (float32, linear interpolation), exact radix select on the device.  ``x`` is any
    per-sample view (``_sample_rows``), read in place: e.g. the mean half of a learned-variance output.  Any storage offset: the 16-byte
    loads are taken only where the base is 16-byte aligned (the same bits either way)."""
    B = x.shape[0]
    n = x.numel() // B
    stride = _sample_rows(x, "x", B, n)
    workspace = quantile_workspace(B, x.device, workspace)
    out = torch.empty(B, dtype=torch.float32, device=x.device) if out is None else out
    if stride == n:
        check(hip.lib().rho_abs_quantile(ptr(x), B, n, float(q), ptr(workspace), ptr(out), stream()), "rho_abs_quantile")
    else:
        check(hip.lib().rho_abs_quantile_strided(ptr(x), B, n, stride, float(q), ptr(workspace), ptr(out), stream()), "rho_abs_quantile_strided")
    return out


def ddim_step(x_t: Tensor, model_out: Tensor, quantile: Tensor, noise: Optional[Tensor], x_prev: Tensor, pred_xstart: Optional[Tensor],
              c_recip: float, c_recipm1: float, sqrt_abar_prev: float, coef_eps: float, sigma_masked: float) -> Tensor:
    _f32c(x_t, "x_t"), _f32c(model_out, "model_out"), _f32c(quantile, "quantile"), _f32c(x_prev, "x_prev")
    B = x_t.shape[0]
    check(hip.lib().rho_ddim_step(ptr(x_t), ptr(model_out), ptr(quantile), ptr(noise), ptr(x_prev), ptr(pred_xstart), B,
                                  x_t.numel() // B, c_recip, c_recipm1, sqrt_abar_prev, coef_eps, sigma_masked, stream()),
          "rho_ddim_step")
    return x_prev


# GaussianDiffusionPipeline API (csrc/gaussian.hip): rows of the packed per-timestep table (include/rho_hip.h RHO_GD_*)
GD_ROWS = ("sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "model_var", "model_logvar", "post_logvar", "abar", "abar_prev", "abar_next",
           "sqrt_abar", "log_1m_abar", "1m_abar", "post_var", "log_beta")
GD_ROW = {k: i for i, k in enumerate(GD_ROWS)}
GD_START_X, GD_EPSILON = 0, 1
GD_LEARNED, GD_LEARNED_RANGE = 0, 1         # var_type of the learned-variance entry points
GD_AFFINE_OPS = {"ax": 0, "ax+by": 1, "ax-by": 2, "(ax-y)/b": 3}


def _gd_t(t: Tensor, batch: int) -> Tensor:
    if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 1 or t.numel() != batch:
        raise RhoHipError(f"t must be a contiguous int64 [{batch}] GPU tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _gd_tab(tab: Tensor) -> int:
    _f32c(tab, "tab")
    if tab.dim() != 2 or tab.shape[0] != len(GD_ROWS):
        raise RhoHipError(f"tab must be float32 [{len(GD_ROWS)}, T], got {tuple(tab.shape)}")
    return tab.shape[1]


def _same(x: Tensor, *others) -> None:
    for name, o in others:
        if o is not None:
            _f32c(o, name)
            if o.shape != x.shape:
                raise RhoHipError(f"{name} has shape {tuple(o.shape)}, expected {tuple(x.shape)}")


def gd_affine(x: Tensor, y: Optional[Tensor], t: Tensor, tab: Tensor, row_a: str, row_b: Optional[str], op: str,
              out: Optional[Tensor] = None, err_flag: Optional[Tensor] = None) -> Tensor:
    """out = a[t]*x | a[t]*x + b[t]*y | a[t]*x - b[t]*y | (a[t]*x - y)/b[t] with a, b rows of the packed table (rho_gd_affine)."""
    _f32c(x, "x")
    _same(x, ("y", y))
    B = x.shape[0]
    T = _gd_tab(tab)
    out = torch.empty_like(x) if out is None else out
    _same(x, ("out", out))
    check(hip.lib().rho_gd_affine(ptr(x), ptr(y), ptr(out), ptr(_gd_t(t, B)), ptr(tab), T, GD_ROW[row_a], GD_ROW[row_b] if row_b else 0,
                                  GD_AFFINE_OPS[op], B, x.numel() // B, ptr(err_flag), stream()), "rho_gd_affine")
    return out


def _gd_quantile(quantile: Optional[Tensor], batch: int) -> None:
    if quantile is not None and _f32c(quantile, "quantile").numel() != batch:
        raise RhoHipError("quantile must be float32 [B]")


def _gd_variance(var_values: Optional[Tensor], var_type: Optional[int], *lv_only) -> bool:
    """Whether the call has a learned variance: ``var_values`` and ``var_type`` come together, and what only a learned variance has
    (``lv_only``) comes with them."""
    if (var_values is None) != (var_type is None) or (var_values is None and any(o is not None for o in lv_only)):
        raise RhoHipError("a learned variance takes var_values and var_type together; variance / log_variance outputs need them")
    return var_values is not None


def gd_posterior_step(x_t: Tensor, model_out: Tensor, t: Tensor, tab: Tensor, mean_type: int, quantile: Optional[Tensor],
                      grad: Optional[Tensor], noise: Optional[Tensor], out: Optional[Tensor], pred_xstart: Optional[Tensor],
                      err_flag: Optional[Tensor] = None, var_values: Optional[Tensor] = None, var_type: Optional[int] = None,
                      variance: Optional[Tensor] = None, log_variance: Optional[Tensor] = None) -> Optional[Tensor]:
    """p_mean_variance / condition_mean / p_sample in one pass.  With a fixed variance (rho_gd_posterior_step) it comes from ``tab``
    and ``out`` is required.  With a learned one (rho_gd_posterior_step_lv: ``var_values`` and ``var_type`` GD_LEARNED /
    GD_LEARNED_RANGE) ``model_out`` (the mean half or an x0) and ``var_values`` are per-sample views read in place, every output is
    optional and the per-element ``variance`` / ``log_variance`` can be written too."""
    _f32c(x_t, "x_t")
    _same(x_t, ("grad", grad), ("noise", noise), ("out", out), ("pred_xstart", pred_xstart), ("variance", variance),
          ("log_variance", log_variance))
    B, n = x_t.shape[0], x_t.numel() // x_t.shape[0]
    _gd_quantile(quantile, B)
    if _gd_variance(var_values, var_type, variance, log_variance):
        ms, vs = _sample_rows(model_out, "model_out", B, n), _sample_rows(var_values, "var_values", B, n)
        check(hip.lib().rho_gd_posterior_step_lv(ptr(x_t), ptr(model_out), ms, ptr(var_values), vs, ptr(_gd_t(t, B)), ptr(tab), _gd_tab(tab),
                                                 mean_type, var_type, ptr(quantile), ptr(grad), ptr(noise), ptr(out), ptr(pred_xstart),
                                                 ptr(variance), ptr(log_variance), B, n, ptr(err_flag), stream()), "rho_gd_posterior_step_lv")
    else:
        _same(x_t, ("model_out", model_out))
        check(hip.lib().rho_gd_posterior_step(ptr(x_t), ptr(model_out), ptr(_gd_t(t, B)), ptr(tab), _gd_tab(tab), mean_type, ptr(quantile),
                                              ptr(grad), ptr(noise), ptr(out), ptr(pred_xstart), B, n, ptr(err_flag), stream()),
              "rho_gd_posterior_step")
    return out


def gd_ddim_step(x_t: Tensor, model_out: Tensor, t: Tensor, tab: Tensor, mean_type: int, quantile: Optional[Tensor],
                 grad: Optional[Tensor], noise: Optional[Tensor], eta: float, reverse: bool, sample: Tensor, pred_xstart: Optional[Tensor],
                 err_flag: Optional[Tensor] = None) -> Tensor:
    """ddim_sample (eta, condition_score) or ddim_reverse_sample with per-sample t (rho_gd_ddim_step; rho_gd_ddim_step_strided where
    ``model_out`` is a non-contiguous per-sample view of x_t's per-sample size, read in place)."""
    _f32c(x_t, "x_t")
    _same(x_t, ("grad", grad), ("noise", noise), ("sample", sample), ("pred_xstart", pred_xstart))
    B, n = x_t.shape[0], x_t.numel() // x_t.shape[0]
    stride = _sample_rows(model_out, "model_out", B, n)
    _gd_quantile(quantile, B)
    tail = (ptr(_gd_t(t, B)), ptr(tab), _gd_tab(tab), mean_type, ptr(quantile), ptr(grad), ptr(noise), float(eta), 1 if reverse else 0,
            ptr(sample), ptr(pred_xstart), B, n, ptr(err_flag), stream())
    if stride == n:
        check(hip.lib().rho_gd_ddim_step(ptr(x_t), ptr(model_out), *tail), "rho_gd_ddim_step")
    else:
        check(hip.lib().rho_gd_ddim_step_strided(ptr(x_t), ptr(model_out), stride, *tail), "rho_gd_ddim_step_strided")
    return sample


def gd_workspace(batch: int, per_sample: int, device, ws: Optional[Tensor] = None) -> Tensor:
    need = hip.lib().rho_gd_reduce_workspace_bytes(batch, per_sample)
    if ws is None or ws.device != torch.device(device) or ws.numel() * ws.element_size() < need:
        ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=device)
    return ws


def gd_vlb_terms(x_start: Tensor, x_t: Optional[Tensor], model_out: Optional[Tensor], t: Optional[Tensor], tab: Tensor, mean_type: int,
                 quantile: Optional[Tensor], noise: Optional[Tensor], vb: Tensor, xstart_mse: Optional[Tensor] = None,
                 mse: Optional[Tensor] = None, raw_kl: Optional[Tensor] = None, raw_nll: Optional[Tensor] = None,
                 pred_xstart: Optional[Tensor] = None, prior: bool = False, workspace: Optional[Tensor] = None,
                 err_flag: Optional[Tensor] = None, var_values: Optional[Tensor] = None, var_type: Optional[int] = None) -> Tensor:
    """_vb_terms_bpd + calc_bpd_loop statistics (or _prior_bpd) per sample (rho_gd_vlb_terms).  vb / xstart_mse / mse: float32 with
    B elements at a common stride (e.g. column j of an [N, T] tensor).  With a learned variance (rho_gd_vlb_terms_lv: ``var_values``
    and ``var_type``) ``model_out`` and ``var_values`` are per-sample views read in place."""
    _f32c(x_start, "x_start")
    _same(x_start, ("x_t", x_t), ("noise", noise), ("pred_xstart", pred_xstart))
    B, n = x_start.shape[0], x_start.numel() // x_start.shape[0]
    stride = vb.stride(0) if vb.dim() == 1 else 1
    for name, o in (("vb", vb), ("xstart_mse", xstart_mse), ("mse", mse)):
        if o is not None and (o.dtype != torch.float32 or not o.is_cuda or o.dim() != 1 or o.numel() != B or (B > 1 and o.stride(0) != stride)):
            raise RhoHipError(f"{name} must be float32 [B] on the GPU with vb's stride")
    for name, o in (("raw_kl", raw_kl), ("raw_nll", raw_nll)):
        if o is not None and (_f32c(o, name).numel() != B):
            raise RhoHipError(f"{name} must be float32 [B]")
    _gd_quantile(quantile, B)
    ws = gd_workspace(B, n, x_start.device, workspace)
    outs = (ptr(vb), ptr(xstart_mse), ptr(mse), max(stride, 1), ptr(raw_kl), ptr(raw_nll), ptr(pred_xstart), ptr(ws), B, n, ptr(err_flag), stream())
    if _gd_variance(var_values, var_type):
        if prior:
            raise RhoHipError("the prior term has no model variance: var_values does not go with prior=True")
        ms, vs = _sample_rows(model_out, "model_out", B, n), _sample_rows(var_values, "var_values", B, n)
        check(hip.lib().rho_gd_vlb_terms_lv(ptr(x_start), ptr(x_t), ptr(model_out), ms, ptr(var_values), vs, ptr(_gd_t(t, B)), ptr(tab),
                                            _gd_tab(tab), mean_type, var_type, ptr(quantile), ptr(noise), *outs), "rho_gd_vlb_terms_lv")
    else:
        _same(x_start, ("model_out", model_out))
        check(hip.lib().rho_gd_vlb_terms(ptr(x_start), ptr(x_t), ptr(model_out), ptr(_gd_t(t, B)) if t is not None else None, ptr(tab),
                                         _gd_tab(tab), mean_type, ptr(quantile), ptr(noise), 1 if prior else 0, *outs), "rho_gd_vlb_terms")
    return vb


def gd_mse_per_sample(target: Tensor, out: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
    """mean_flat((target - out)^2) -> float32 [B], fixed-order reduction (rho_gd_mse_per_sample)."""
    _f32c(target, "target")
    _same(target, ("out", out))
    B, n = target.shape[0], target.numel() // target.shape[0]
    loss = torch.empty(B, dtype=torch.float32, device=target.device)
    ws = gd_workspace(B, n, target.device, workspace)
    check(hip.lib().rho_gd_mse_per_sample(ptr(target), ptr(out), ptr(loss), ptr(ws), B, n, stream()), "rho_gd_mse_per_sample")
    return loss


def gd_mse_per_sample_bwd(target: Tensor, out: Tensor, g: Tensor) -> Tensor:
    _f32c(target, "target")
    _same(target, ("out", out))
    B, n = target.shape[0], target.numel() // target.shape[0]
    if _f32c(g, "g").numel() != B:
        raise RhoHipError("g must be float32 [B]")
    grad = torch.empty_like(out)
    check(hip.lib().rho_gd_mse_per_sample_bwd(ptr(target), ptr(out), ptr(g), ptr(grad), B, n, stream()), "rho_gd_mse_per_sample_bwd")
    return grad


def _gd_hybrid_args(x_start: Tensor, x_t: Tensor, target: Tensor, model_out: Tensor):
    _f32c(x_start, "x_start")
    _same(x_start, ("x_t", x_t), ("target", target))
    _f32c(model_out, "model_out")
    B, n = x_start.shape[0], x_start.numel() // x_start.shape[0]
    if model_out.shape[0] != B or model_out.numel() != 2 * B * n:
        raise RhoHipError(f"model_out must be float32 [B, 2C, ...] for x_start {tuple(x_start.shape)}, got {tuple(model_out.shape)}")
    return B, n


def gd_hybrid_loss(x_start: Tensor, x_t: Tensor, target: Tensor, model_out: Tensor, t: Tensor, tab: Tensor, mean_type: int, var_type: int,
                   vb_scale: Optional[float], workspace: Optional[Tensor] = None, err_flag: Optional[Tensor] = None):
    """training_losses' hybrid objective with a learned variance (rho_gd_hybrid_loss): (loss, mse, vb), float32 [B] each.
    ``vb_scale``: T/1000 for RESCALED_MSE, None for MSE."""
    B, n = _gd_hybrid_args(x_start, x_t, target, model_out)
    loss, mse, vb = (torch.empty(B, dtype=torch.float32, device=x_start.device) for _ in range(3))
    ws = gd_workspace(B, n, x_start.device, workspace)
    check(hip.lib().rho_gd_hybrid_loss(ptr(x_start), ptr(x_t), ptr(target), ptr(model_out), ptr(_gd_t(t, B)), ptr(tab), _gd_tab(tab),
                                       mean_type, var_type, 0 if vb_scale is None else 1, float(vb_scale or 0.0), ptr(loss), ptr(mse),
                                       ptr(vb), ptr(ws), B, n, ptr(err_flag), stream()), "rho_gd_hybrid_loss")
    return loss, mse, vb


def gd_hybrid_loss_bwd(x_start: Tensor, x_t: Tensor, target: Tensor, model_out: Tensor, t: Tensor, tab: Tensor, mean_type: int,
                       var_type: int, vb_scale: Optional[float], g_loss: Optional[Tensor], g_mse: Optional[Tensor], g_vb: Optional[Tensor],
                       err_flag: Optional[Tensor] = None) -> Tensor:
    """d(loss, mse, vb) / d model_out [B, 2C, ...] (rho_gd_hybrid_loss_bwd); an upstream gradient of None counts as 0."""
    B, n = _gd_hybrid_args(x_start, x_t, target, model_out)
    for name, o in (("g_loss", g_loss), ("g_mse", g_mse), ("g_vb", g_vb)):
        if o is not None and _f32c(o, name).numel() != B:
            raise RhoHipError(f"{name} must be float32 [B]")
    grad = torch.empty_like(model_out)
    check(hip.lib().rho_gd_hybrid_loss_bwd(ptr(x_start), ptr(x_t), ptr(target), ptr(model_out), ptr(_gd_t(t, B)), ptr(tab), _gd_tab(tab),
                                           mean_type, var_type, 0 if vb_scale is None else 1, float(vb_scale or 0.0), ptr(g_loss),
                                           ptr(g_mse), ptr(g_vb), ptr(grad), B, n, ptr(err_flag), stream()), "rho_gd_hybrid_loss_bwd")
    return grad


def normal_kl(operands, out: Tensor, batch: int, per_sample: int) -> Tensor:
    """operands: 4 x (tensor or None, mode, scalar) as rho_normal_kl takes them (mode 0 full, 1 per-sample, 2 scalar)."""
    ps = [ptr(o[0]) for o in operands]
    modes = sum(o[1] << (2 * k) for k, o in enumerate(operands))
    check(hip.lib().rho_normal_kl(*ps, *[float(o[2]) for o in operands], modes, ptr(out), batch, per_sample, stream()), "rho_normal_kl")
    return out


def discretized_gaussian_ll(operands, out: Tensor, batch: int, per_sample: int) -> Tensor:
    ps = [ptr(o[0]) for o in operands]
    modes = sum(o[1] << (2 * k) for k, o in enumerate(operands))
    check(hip.lib().rho_discretized_gaussian_ll(*ps, *[float(o[2]) for o in operands], modes, ptr(out), batch, per_sample, stream()),
          "rho_discretized_gaussian_ll")
    return out


def approx_normal_cdf(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    _f32c(x, "x")
    out = torch.empty_like(x) if out is None else out
    check(hip.lib().rho_approx_normal_cdf(ptr(x), ptr(out), x.numel(), stream()), "rho_approx_normal_cdf")
    return out


def step_advance(t_dev: Optional[Tensor], offset_dev: Optional[Tensor], delta: int) -> None:
    check(hip.lib().rho_step_advance(ptr(t_dev), ptr(offset_dev), delta, stream()), "rho_step_advance")


def philox_normal(out: Tensor, seed: int, offset: int = 0, offset_dev: Optional[Tensor] = None) -> Tensor:
    _f32c(out, "out")
    check(hip.lib().rho_philox_normal(ptr(out), out.numel(), seed & (2 ** 64 - 1), offset, ptr(offset_dev), stream()),
          "rho_philox_normal")
    return out


def mse(a: Tensor, b: Tensor, want_grad: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    _f32c(a, "a"), _f32c(b, "b")
    buf = torch.empty(1 + 1024, dtype=torch.float32, device=a.device)        # loss + the ordered reduction's block partials
    loss = buf[:1]
    grad = torch.empty_like(a) if want_grad else None
    check(hip.lib().rho_mse_ws(ptr(a), ptr(b), ptr(loss), ptr(grad), a.numel(), buf.data_ptr() + 4, 1024, stream()), "rho_mse_ws")
    return loss, grad


def pred_loss(pred: Tensor, x0: Tensor, eps: Tensor, t: Tensor, alpha_bar: Tensor, w: Optional[Tensor], pred_type: int,
              want_grad: bool = False, err_flag: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """The weighted training loss of an eps- (0), v- (1) or x0-predicting (2) backbone and optionally its gradient w.r.t. ``pred``
    (rho_pred_loss_ws).  ``pred`` / ``x0`` / ``eps`` [B, ...] float32, ``t`` int64 [B] on the device, ``alpha_bar`` [T] and ``w`` [T]
    or None (weight 1)."""
    _f32c(pred, "pred"), _f32c(x0, "x0"), _f32c(eps, "eps"), _f32c(alpha_bar, "alpha_bar")
    if x0.shape != pred.shape or eps.shape != pred.shape or pred.dim() < 1 or pred.numel() < 1:
        raise RhoHipError(f"pred, x0 and eps must have one non-empty shape: got {tuple(pred.shape)}, {tuple(x0.shape)}, {tuple(eps.shape)}")
    B = pred.shape[0]
    if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.numel() != B:
        raise RhoHipError(f"t must be a contiguous int64 [{B}] GPU tensor")
    if w is not None and (_f32c(w, "w").numel() != alpha_bar.numel()):
        raise RhoHipError(f"w must have the {alpha_bar.numel()} entries of alpha_bar, got {w.numel()}")
    if pred_type not in (0, 1, 2):
        raise RhoHipError(f"pred_type must be 0 (epsilon), 1 (v) or 2 (sample), got {pred_type}")
    if err_flag is not None and (err_flag.dtype != torch.int32 or not err_flag.is_cuda or err_flag.numel() != 1):
        raise RhoHipError("err_flag must be int32[1] on the GPU or None")
    buf = torch.empty(1 + 1024, dtype=torch.float32, device=pred.device)     # loss + the ordered reduction's block partials
    loss = buf[:1]
    grad = torch.empty_like(pred) if want_grad else None
    check(hip.lib().rho_pred_loss_ws(ptr(pred), ptr(x0), ptr(eps), ptr(alpha_bar), ptr(w), ptr(t), B, pred.numel() // B,
                                     alpha_bar.numel(), int(pred_type), ptr(loss), ptr(grad), buf.data_ptr() + 4, 1024, ptr(err_flag),
                                     stream()), "rho_pred_loss_ws")
    return loss, grad


def mean_flat(x: Tensor) -> Tensor:
    """Mean over all non-batch axes (layers.py:105-110) on the device, float32, fixed summation order."""
    x = _f32c(x, "x")
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    check(hip.lib().rho_mean_flat(ptr(x), ptr(out), x.shape[0], x.numel() // x.shape[0], stream()), "rho_mean_flat")
    return out


def deterministic() -> bool:
    """The library's reproducibility switch (RHO_DETERMINISTIC=1 / rho_set_deterministic)."""
    return bool(hip.lib().rho_get_deterministic())


def set_deterministic(on: bool) -> bool:
    return bool(hip.lib().rho_set_deterministic(1 if on else 0))


def adamw(p: Tensor, g: Tensor, m: Tensor, v: Tensor, lr: float, beta1: float, beta2: float, eps: float,
          weight_decay: float, step: int) -> None:
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _f32c(t, name)
    check(hip.lib().rho_adamw(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step, stream()),
          "rho_adamw")


# kind codes and flag bits of rho_optim_step (include/rho_hip.h)
OPT_KINDS = {"Adam": 0, "AdamW": 1, "SGD": 2, "RMSprop": 3, "Adagrad": 4, "Adamax": 5, "NAdam": 6, "RAdam": 7, "Adadelta": 8}
OPT_MAXIMIZE, OPT_AMSGRAD, OPT_DECOUPLED_WD, OPT_NESTEROV, OPT_CENTERED = 1, 2, 4, 8, 16


def optim_step(kind: str, p: Tensor, g: Tensor, states, hp, step: int, flags: int = 0, gscale: Optional[Tensor] = None) -> None:
    """One fused update of the flat arena ``p`` by ``g`` (rho_optim_step).  ``states``: up to three state arenas in the kind's slot
    order, None for a slot it does not use; ``hp``: (lr, weight_decay, eps, then the kind's own hyperparameters), rounded to float32
    as the ABI receives them; ``gscale``: 1-element device tensor that scales the gradient as it is loaded."""
    if kind not in OPT_KINDS:
        raise RhoHipError(f"no fused update for optimizer kind {kind!r}")
    _f32c(p, "p")
    _f32c(g, "g")
    s = list(states) + [None] * (3 - len(states))
    for i, t in enumerate(s):
        if t is not None and (_f32c(t, f"s{i}").numel() != p.numel()):
            raise RhoHipError(f"state arena s{i} has {t.numel()} elements, the parameters {p.numel()}")
    if g.numel() != p.numel():
        raise RhoHipError(f"gradient arena has {g.numel()} elements, the parameters {p.numel()}")
    if gscale is not None:
        _f32c(gscale, "gscale")
    vals = [float(v) for v in hp] + [0.0] * (8 - len(hp))
    hp_arr = (C.c_float * 8)(*vals)
    check(hip.lib().rho_optim_step(OPT_KINDS[kind], flags, ptr(p), ptr(g), *(ptr(t) if t is not None else None for t in s), p.numel(),
                                   C.addressof(hp_arr), step, ptr(gscale) if gscale is not None else None, stream()),
          "rho_optim_step")


def sumsq_blocks(n: int) -> int:
    """Number of per-workgroup partials rho_sumsq_partial writes for an n-element arena."""
    k = hip.lib().rho_sumsq_blocks(n)
    check(min(k, 0), "rho_sumsq_blocks")
    return k


def sumsq_partial(x: Tensor, partials: Tensor) -> None:
    """Per-workgroup sums of x^2 into ``partials`` (>= sumsq_blocks(x.numel()) float32), fixed order, no atomics."""
    _f32c(x, "x")
    _f32c(partials, "partials")
    if partials.numel() < sumsq_blocks(x.numel()):
        raise RhoHipError("partials buffer too small")
    check(hip.lib().rho_sumsq_partial(ptr(x), x.numel(), ptr(partials), stream()), "rho_sumsq_partial")


def clip_coef(partials: Tensor, max_norm: float, out: Tensor) -> None:
    """out[0] = sqrt(sum partials), out[1] = min(1, max_norm / (out[0] + 1e-6)) (torch.nn.utils.clip_grad_norm_), one workgroup."""
    _f32c(partials, "partials")
    if _f32c(out, "out").numel() < 2:
        raise RhoHipError("out needs 2 floats")
    check(hip.lib().rho_clip_coef(ptr(partials), partials.numel(), max_norm, ptr(out), stream()), "rho_clip_coef")


# ----------------------------------------------------------------------------- embeddings
# activation codes of the C ABI (include/rho_hip.h, rho_timestep_embed): the elementwise, parameter-free entries of the reference's
# activation registry (rho_diffusion/registry.py:162-170)
ACT_CODES = {"Identity": 0, "SiLU": 1, "ReLU": 2, "GELU": 3, "Tanh": 4, "Sigmoid": 5, "ELU": 6}


def sinusoid_frequencies(dim: int, wavelength: int = 10000, device=None) -> Tensor:
    """omega_i = wavelength^(2i / dim), i = 0 .. dim/2 - 1, float32: the denominators of the timestep sinusoid
    (models/common.py:38 evaluates this very expression; the kernel divides t by it)."""
    if dim % 2:
        raise RhoHipError("`dim` should be dividable by 2.")
    i = torch.arange(dim // 2)
    return torch.pow(wavelength, 2 * i / dim).to(device=device, dtype=torch.float32).contiguous()


def timestep_embed(omega: Tensor, t: Optional[Tensor], batch: int, *, t_scalar_dev: Optional[Tensor] = None,
                   w0: Optional[Tensor] = None, b0: Optional[Tensor] = None, w2: Optional[Tensor] = None,
                   b2: Optional[Tensor] = None, cond: Optional[Tensor] = None, pe_out: Optional[Tensor] = None,
                   h_out: Optional[Tensor] = None, emb_out: Optional[Tensor] = None, act: int = 1):
    """Sinusoid of any integer t (+ the time_embed MLP and the label-embedding add when w0 is given): rho_timestep_embed.
    ``act``: activation code between the two linears (1 = SiLU, see ACT_CODES)."""
    _f32c(omega, "omega")
    dim = 2 * omega.numel()
    if t is not None and (t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous()):
        raise RhoHipError("t must be a contiguous int64 GPU tensor")
    edim = w0.shape[0] if w0 is not None else 0
    if pe_out is None:
        pe_out = torch.empty(batch, dim, dtype=torch.float32, device=omega.device)
    if w0 is not None and emb_out is None:
        emb_out = torch.empty(batch, edim, dtype=torch.float32, device=omega.device)
    check(hip.lib().rho_timestep_embed(ptr(omega), ptr(t), ptr(t_scalar_dev), ptr(w0), ptr(b0), ptr(w2), ptr(b2), ptr(cond),
                                       ptr(pe_out), ptr(h_out), ptr(emb_out), batch, dim, edim, int(act), stream()), "rho_timestep_embed")
    return pe_out if w0 is None else emb_out


def randint(n: int, high: int, seed: int, offset: int = 0, offset_dev: Optional[Tensor] = None, out: Optional[Tensor] = None,
            device=None) -> Tensor:
    """Uniform int64 on [0, high) from the Philox stream (seed, offset): random_timesteps on the device."""
    out = torch.empty(n, dtype=torch.int64, device=device) if out is None else out
    hip.require_gpu(out, "out")
    check(hip.lib().rho_randint(ptr(out), n, high, seed & (2 ** 64 - 1), offset, ptr(offset_dev), stream()), "rho_randint")
    return out


def cond_keep_mask(n: int, p: float, seed: int, offset: int = 0, offset_dev: Optional[Tensor] = None, out: Optional[Tensor] = None,
                   device=None) -> Tensor:
    """uint8 [n] keep mask of label dropout: keep[b] = (u_b >= p), one Philox uniform per sample from the stream (seed, offset)."""
    out = torch.empty(n, dtype=torch.uint8, device=device) if out is None else out
    hip.require_gpu(out, "out")
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < n:
        raise RhoHipError("out must be a contiguous uint8 tensor of at least n elements")
    check(hip.lib().rho_cond_keep_mask(ptr(out), n, float(p), seed & (2 ** 64 - 1), offset, ptr(offset_dev), stream()),
          "rho_cond_keep_mask")
    return out


def cond_drop(cond: Tensor, cond_idx: Optional[Tensor], keep: Tensor, nkeys: int = 0) -> Tensor:
    """Zero the rows of ``cond`` [B, dim] whose ``keep`` [B] (uint8) is 0 and set their ``cond_idx`` [B, nkeys] entries to -1."""
    _f32c(cond, "cond")
    hip.require_gpu(keep, "keep")
    B = cond.shape[0]
    if cond.dim() != 2 or keep.dtype != torch.uint8 or not keep.is_contiguous() or keep.numel() != B:
        raise RhoHipError(f"cond must be [B, dim] and keep uint8 [B]: got {tuple(cond.shape)}, {keep.dtype} {tuple(keep.shape)}")
    if cond_idx is not None and (cond_idx.dtype != torch.int32 or not cond_idx.is_contiguous() or cond_idx.numel() < B * nkeys):
        raise RhoHipError("cond_idx must be a contiguous int32 tensor of at least B * nkeys elements")
    check(hip.lib().rho_cond_drop(ptr(cond), ptr(cond_idx), ptr(keep), B, cond.shape[1], nkeys, stream()), "rho_cond_drop")
    return cond


def sph_harm_fields(lm: Tensor, grid: int, out: Optional[Tensor] = None, minmax_in: Optional[Tensor] = None,
                    minmax_out: Optional[Tensor] = None) -> Tensor:
    """Spherical-harmonic density fields float32 [B, G, G, G] for (l, m) = lm[b] (int32 [B, 2] on the GPU)."""
    hip.require_gpu(lm, "lm")
    if lm.dtype != torch.int32 or lm.dim() != 2 or lm.shape[1] != 2 or not lm.is_contiguous():
        raise RhoHipError("lm must be a contiguous int32 [B, 2] tensor")
    B = lm.shape[0]
    out = torch.empty(B, grid, grid, grid, dtype=torch.float32, device=lm.device) if out is None else out
    ws = torch.empty(int(hip.lib().rho_sph_harm_workspace_bytes(B, grid)) // 8, dtype=torch.float64, device=lm.device)
    for name, mm in (("minmax_in", minmax_in), ("minmax_out", minmax_out)):
        if mm is not None and (mm.dtype != torch.float64 or tuple(mm.shape) != (B, 4) or not mm.is_cuda or not mm.is_contiguous()):
            raise RhoHipError(f"{name} must be a contiguous float64 [B, 4] GPU tensor")
    check(hip.lib().rho_sph_harm_fields(ptr(lm), B, grid, ptr(out), ptr(ws), ptr(minmax_in), ptr(minmax_out), stream()),
          "rho_sph_harm_fields")
    return out


# ----------------------------------------------------------------------------- image datasets
RAW_DTYPES = {torch.float32: 0, torch.uint8: 2, torch.float64: 3}          # RHO_F32 / RHO_U8 / RHO_F64 of include/rho_hip.h


def _pair(v) -> Tuple[int, int]:
    return (int(v), int(v)) if isinstance(v, (int,)) else (int(v[0]), int(v[1]))


def crop_resize_axis_taps(in_size: int, crop: int, out_size: int, antialias: bool):
    """(start int32 [out_size], weight float32 [out_size, k]) of one axis: CenterCrop + bilinear resize (rho_crop_resize_taps, host)."""
    import numpy as np
    L = hip.lib()
    k = int(L.rho_crop_resize_taps(int(in_size), int(crop), int(out_size), int(bool(antialias)), None, None))
    if k <= 0:
        raise RhoHipError(f"rho_crop_resize_taps(in={in_size}, crop={crop}, out={out_size}) failed: {k}")
    start = np.empty(int(out_size), dtype=np.int32)
    weight = np.empty((int(out_size), k), dtype=np.float32)
    L.rho_crop_resize_taps(int(in_size), int(crop), int(out_size), int(bool(antialias)), start.ctypes.data, weight.ctypes.data)
    return torch.from_numpy(start), torch.from_numpy(weight)


def crop_resize_taps(h: int, w: int, crop, size, antialias: bool = True, device=None) -> dict:
    """Device tap tables of CenterCrop(crop) + Resize(size) for raw images [N, h, w, C] (image rows = the w axis after
    swapaxes(1, 3)): build once per geometry and pass to ``crop_resize``."""
    (ch, cw), (oh, ow) = _pair(crop), _pair(size)
    ys, wy = crop_resize_axis_taps(w, ch, oh, antialias)
    xs, wx = crop_resize_axis_taps(h, cw, ow, antialias)
    return dict(hw=(int(h), int(w)), crop=(ch, cw), size=(oh, ow), antialias=bool(antialias),
                y=(ys.to(device), wy.to(device), wy.shape[1]), x=(xs.to(device), wx.to(device), wx.shape[1]))


def crop_resize_check(flag: Tensor) -> None:
    """Host poll of rho_crop_resize's error flag (one synchronisation)."""
    v = int(flag.item())
    if v:
        flag.zero_()
        if v & 4:
            raise RhoHipError("crop_resize: an index lies outside [0, N) (rho_crop_resize err_flag bit 2)")
        raise RhoHipError(f"crop_resize: the tap tables do not match the launch geometry (err_flag {v})")


def crop_resize(raw: Tensor, rowmax: Tensor, index: Tensor, crop, size, antialias: bool = True, taps: Optional[dict] = None,
                out: Optional[Tensor] = None, err_flag: Optional[Tensor] = None) -> Tensor:
    """Rows ``index`` of the resident raw images [N, H, W, C] (uint8 / float32 / float64) -> float32 [B, C, size[0], size[1]]:
    rows / rowmax in numpy's promotion, swapaxes to [C, W, H], CenterCrop(crop), bilinear Resize(size) (antialias: torch's
    triangle filter), 2 t - 1 - one launch (rho_crop_resize).  ``rowmax``: float64 [N] on the device.  Without ``err_flag`` the
    call polls its own flag and raises on an index outside [0, N); with one, the caller polls (``crop_resize_check``)."""
    hip.require_gpu(raw, "raw")
    if raw.dtype not in RAW_DTYPES or raw.dim() != 4 or not raw.is_contiguous():
        raise RhoHipError(f"raw must be a contiguous uint8 / float32 / float64 [N, H, W, C] tensor, got {raw.dtype} {tuple(raw.shape)}")
    N, H, W, Cc = raw.shape
    if rowmax.dtype != torch.float64 or tuple(rowmax.shape) != (N,) or not rowmax.is_cuda or not rowmax.is_contiguous():
        raise RhoHipError(f"rowmax must be a contiguous float64 [{N}] GPU tensor")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda or not index.is_contiguous():
        raise RhoHipError("index must be a contiguous int64 [B] GPU tensor")
    (ch, cw), (oh, ow) = _pair(crop), _pair(size)
    if taps is None:
        taps = crop_resize_taps(H, W, (ch, cw), (oh, ow), antialias, raw.device)
    elif taps["hw"] != (H, W) or taps["crop"] != (ch, cw) or taps["size"] != (oh, ow) or taps["antialias"] != bool(antialias):
        raise RhoHipError(f"crop_resize: taps were built for {taps['hw']} crop {taps['crop']} size {taps['size']} antialias "
                          f"{taps['antialias']}, the call asks for {(H, W)} crop {(ch, cw)} size {(oh, ow)} antialias {bool(antialias)}")
    B = index.numel()
    if out is None:
        out = torch.empty(B, Cc, oh, ow, dtype=torch.float32, device=raw.device)
    elif _f32c(out, "out").shape != (B, Cc, oh, ow):
        raise RhoHipError(f"out must be float32 [{B}, {Cc}, {oh}, {ow}], got {tuple(out.shape)}")
    if B == 0:
        return out
    (ys, wy, ky), (xs, wx, kx) = taps["y"], taps["x"]
    flag = torch.zeros(1, dtype=torch.int32, device=raw.device) if err_flag is None else err_flag
    check(hip.lib().rho_crop_resize(ptr(raw), RAW_DTYPES[raw.dtype], N, H, W, Cc, ptr(index), B, ptr(rowmax), ptr(ys), ptr(wy), ky,
                                    ptr(xs), ptr(wx), kx, ch, cw, oh, ow, ptr(out), ptr(flag), stream()), "rho_crop_resize")
    if err_flag is None:
        crop_resize_check(flag)
    return out


def pil_resize_taps(in_size: int, out_size: int):
    """(start int32 [out_size], count int32 [out_size], coef int32 [out_size, ksize]) of one axis of PIL.Image.resize(BILINEAR) on
    an 8-bit image: Pillow's fixed-point tap table (rho_pil_resize_taps, host)."""
    import numpy as np
    L = hip.lib()
    k = int(L.rho_pil_resize_taps(int(in_size), int(out_size), None, None, None))
    if k <= 0:
        raise RhoHipError(f"rho_pil_resize_taps(in={in_size}, out={out_size}) failed: {k}")
    start = np.empty(int(out_size), dtype=np.int32)
    count = np.empty(int(out_size), dtype=np.int32)
    coef = np.empty((int(out_size), k), dtype=np.int32)
    L.rho_pil_resize_taps(int(in_size), int(out_size), start.ctypes.data, count.ctypes.data, coef.ctypes.data)
    return torch.from_numpy(start), torch.from_numpy(count), torch.from_numpy(coef)


def u8_image_lut(device=None) -> Tensor:
    """float32 [256]: ToTensor() then 2 t - 1 for every uint8 value, in torch's own arithmetic (byte -> float32, / 255, * 2, - 1)."""
    return ((torch.arange(256, dtype=torch.float32) / 255) * 2 - 1).to(device)


def u8_image_taps(h: int, w: int, size, device=None) -> dict:
    """Device tap tables of Image.resize((size[1], size[0]), BILINEAR) for raw images [N, h, w, C]; an axis that keeps its size has
    none (Pillow skips that pass).  Build once per geometry and pass to ``u8_image_batch``."""
    oh, ow = _pair(size)

    def axis(n_in, n_out):
        if n_in == n_out:
            return None
        s, n, k = pil_resize_taps(n_in, n_out)
        return s.to(device), n.to(device), k.to(device), k.shape[1]

    return dict(hw=(int(h), int(w)), size=(oh, ow), y=axis(int(h), oh), x=axis(int(w), ow))


def u8_image_check(flag: Tensor) -> None:
    """Host poll of rho_u8_image_batch's error flag (one synchronisation)."""
    v = int(flag.item())
    if v:
        flag.zero_()
        if v & 4:
            raise RhoHipError("u8_image_batch: an index lies outside [0, N) (rho_u8_image_batch err_flag bit 2)")
        raise RhoHipError(f"u8_image_batch: the tap tables do not match the launch geometry (err_flag {v})")


def u8_image_batch(raw: Tensor, index: Tensor, size=None, lut: Optional[Tensor] = None, taps: Optional[dict] = None,
                   out: Optional[Tensor] = None, err_flag: Optional[Tensor] = None) -> Tensor:
    """Rows ``index`` of the resident uint8 images [N, H, W, C] -> float32 [B, C, size[0], size[1]] as torchvision makes them from a
    PIL.Image: Image.resize(BILINEAR) in Pillow's integer arithmetic (``size`` None: no resize), ToTensor and 2 t - 1 through ``lut``
    (default ``u8_image_lut``) - one launch (rho_u8_image_batch), bit-equal to the host path.  Without ``err_flag`` the call polls its
    own flag and raises on an index outside [0, N); with one, the caller polls (``u8_image_check``)."""
    hip.require_gpu(raw, "raw")
    if raw.dtype != torch.uint8 or raw.dim() != 4 or not raw.is_contiguous():
        raise RhoHipError(f"raw must be a contiguous uint8 [N, H, W, C] tensor, got {raw.dtype} {tuple(raw.shape)}")
    N, H, W, Cc = raw.shape
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda or not index.is_contiguous():
        raise RhoHipError("index must be a contiguous int64 [B] GPU tensor")
    oh, ow = (H, W) if size is None else _pair(size)
    if taps is None:
        taps = u8_image_taps(H, W, (oh, ow), raw.device)
    elif taps["hw"] != (H, W) or taps["size"] != (oh, ow):
        raise RhoHipError(f"u8_image_batch: taps were built for {taps['hw']} -> {taps['size']}, the call asks for {(H, W)} -> {(oh, ow)}")
    if lut is None:
        lut = u8_image_lut(raw.device)
    elif lut.dtype != torch.float32 or tuple(lut.shape) != (256,) or not lut.is_cuda or not lut.is_contiguous():
        raise RhoHipError("lut must be a contiguous float32 [256] GPU tensor")
    B = index.numel()
    if out is None:
        out = torch.empty(B, Cc, oh, ow, dtype=torch.float32, device=raw.device)
    elif _f32c(out, "out").shape != (B, Cc, oh, ow):
        raise RhoHipError(f"out must be float32 [{B}, {Cc}, {oh}, {ow}], got {tuple(out.shape)}")
    if B == 0:
        return out
    ys, yn, ky, ksy = taps["y"] or (None, None, None, 0)
    xs, xn, kx, ksx = taps["x"] or (None, None, None, 0)
    flag = torch.zeros(1, dtype=torch.int32, device=raw.device) if err_flag is None else err_flag
    check(hip.lib().rho_u8_image_batch(ptr(raw), N, H, W, Cc, ptr(index), B, ptr(ys), ptr(yn), ptr(ky), ksy, ptr(xs), ptr(xn), ptr(kx),
                                       ksx, oh, ow, ptr(lut), ptr(out), ptr(flag), stream()), "rho_u8_image_batch")
    if err_flag is None:
        u8_image_check(flag)
    return out


# ----------------------------------------------------------------------------- spectra
def line_profile_check(flag: Tensor) -> None:
    """Host poll of rho_line_profile's error flag (one synchronisation)."""
    v = int(flag.item())
    if v:
        flag.zero_()
        if v & 4:
            raise RhoHipError("line_profile: an index lies outside [0, N) (rho_line_profile err_flag bit 2)")
        raise RhoHipError(f"line_profile: offsets do not describe lines inside [0, total] (err_flag {v})")


def line_profile(grid: Tensor, centers: Tensor, intensity: Tensor, offsets: Tensor, index: Tensor, widths: Tensor,
                 line_width: Optional[Tensor] = None, out: Optional[Tensor] = None, err_flag: Optional[Tensor] = None,
                 normalise: bool = True) -> Tensor:
    """Gaussian line profiles float32 [B, G] of items ``index`` (int64 [B]) on the monotone float32 ``grid`` [G] (rho_line_profile):
    the lines of all N items packed in CSR form (``centers`` / ``intensity`` float32 [total], ``offsets`` int64 [N + 1]), sorted by
    centre inside an item; ``widths`` float32 [B], or one width per line in ``line_width`` float32 [total].  Lines outside
    [grid.min(), grid.max()] are masked; ``normalise`` divides every row by its maximum (a row without a line in range is NaN, as
    in the reference), else the plain sums are returned.  Without ``err_flag`` the call polls its own flag and raises on an index
    outside [0, N); with one, the caller polls (``line_profile_check``)."""
    hip.require_gpu(grid, "grid")
    _f32c(grid, "grid")
    if grid.dim() != 1 or grid.numel() == 0:
        raise RhoHipError(f"grid must be a non-empty float32 [G] tensor, got {tuple(grid.shape)}")
    G = grid.numel()
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_cuda or not offsets.is_contiguous():
        raise RhoHipError("offsets must be a contiguous int64 [N + 1] GPU tensor")
    N = offsets.numel() - 1
    total = centers.numel()
    for name, t in (("centers", centers), ("intensity", intensity), ("line_width", line_width)):
        if t is None:
            continue
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != total or not t.is_cuda or not t.is_contiguous():
            raise RhoHipError(f"{name} must be a contiguous float32 [{total}] GPU tensor")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda or not index.is_contiguous():
        raise RhoHipError("index must be a contiguous int64 [B] GPU tensor")
    B = index.numel()
    if widths.dtype != torch.float32 or tuple(widths.shape) != (B,) or not widths.is_cuda or not widths.is_contiguous():
        raise RhoHipError(f"widths must be a contiguous float32 [{B}] GPU tensor")
    if out is None:
        out = torch.empty(B, G, dtype=torch.float32, device=grid.device)
    elif _f32c(out, "out").shape != (B, G):
        raise RhoHipError(f"out must be float32 [{B}, {G}], got {tuple(out.shape)}")
    if B == 0:
        return out
    rowmax = torch.empty(B, dtype=torch.float32, device=grid.device) if normalise else None
    flag = torch.zeros(1, dtype=torch.int32, device=grid.device) if err_flag is None else err_flag
    check(hip.lib().rho_line_profile(ptr(grid), G, ptr(centers), ptr(intensity), ptr(line_width), total, ptr(offsets), N, ptr(index),
                                     ptr(widths), B, ptr(out), ptr(rowmax), ptr(flag), stream()), "rho_line_profile")
    if err_flag is None:
        line_profile_check(flag)
    return out


def linear(x: Tensor, w: Tensor, bias: Optional[Tensor], add: Optional[Tensor] = None, act_in: int = 0,
           act_out: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """out = act_out(w act_in(x) + bias (+ add)): rho_linear.  ``act_in`` / ``act_out``: activation codes (see ACT_CODES; True is SiLU)."""
    _f32c(x, "x"), _f32c(w, "w")
    B, K = x.shape
    O = w.shape[0]
    if w.shape[1] != K:
        raise RhoHipError(f"linear: weight {tuple(w.shape)} does not match input {tuple(x.shape)}")
    out = torch.empty(B, O, dtype=torch.float32, device=x.device) if out is None else out
    check(hip.lib().rho_linear(ptr(x), ptr(w), ptr(bias), ptr(add), ptr(out), B, K, O, int(act_in), int(act_out), stream()),
          "rho_linear")
    return out


# ----------------------------------------------------------------------------- layout
def pack_input(x: Tensor, dtype: torch.dtype, cpad: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """[N, C, *S] float32 -> channels-last [N, D, H, W, Cpad] in the engine dtype."""
    _f32c(x, "x")
    N, Cc = x.shape[0], x.shape[1]
    D, H, W = spatial5(x.shape[2:])
    ck = elem_chunk(dtype)
    cpad = cpad or ((Cc + ck - 1) // ck) * ck
    out = torch.empty(N, D, H, W, cpad, dtype=dtype, device=x.device) if out is None else out
    check(hip.lib().rho_pack_input(ptr(x), ptr(out), dtype_code(dtype), N, Cc, D * H * W, cpad, stream()), "rho_pack_input")
    return out


# Prepared layouts of a conv weight [Cout, Cin, *k] float32 (rho_prep_op, include/rho_hip.h): one set of shape rules (prepared_shape),
# one record builder with the extent checks (prep_op), two sinks with the same add_* methods (PrepTable: one launch; EagerPrep: at once)
def kernel3(w) -> Tuple[int, int, int]:
    """(kd, kh, kw) of a conv weight [Cout, Cin, *k] (a tensor or its shape; missing leading axes are 1)."""
    k = [int(v) for v in getattr(w, "shape", w)[2:]]
    return tuple([1] * (3 - len(k)) + k)


def sel_code(taps) -> int:
    """A tap selection as rho_prep_conv_weight_sel reads it: new tap r of the axis is source tap (code >> 4r) & 15."""
    return sum(int(v) << (4 * i) for i, v in enumerate(taps))


def _sel_taps(sel_hw, k) -> Tuple[tuple, tuple]:
    return tuple(tuple(range(k[1 + a])) if sel_hw[a] is None else tuple(sel_hw[a]) for a in (0, 1))


def prepared_shape(kind: int, w, dtype: torch.dtype, dgrad: bool = False, *, k=None, phase_hw=(0, 0), sel_hw=(None, None)):
    """(taps', d1, d2) of the layout ``kind`` (hip.PREP_FWD / DGRAD / PHASE / SEL) of a weight [Cout, Cin, *k] (tensor or shape; ``k``
    overrides the kernel extents): forward [taps', ceil32(Cout), ceilCK(Cin)], data gradient (PREP_DGRAD, or ``dgrad``) [taps',
    ceil32(Cin), ceilCK(Cout)]; a phased axis has 2 taps, a selected axis as many as it selects."""
    shape = getattr(w, "shape", w)
    cout, cin = int(shape[0]), int(shape[1])
    kd, kh, kw = kernel3(shape) if k is None else k
    if kind == hip.PREP_PHASE:
        kh, kw = (2 if phase_hw[0] else kh), (2 if phase_hw[1] else kw)
    elif kind == hip.PREP_SEL:
        kh, kw = (len(s) for s in _sel_taps(sel_hw, (kd, kh, kw)))
    rows, cols = (cin, cout) if (dgrad or kind == hip.PREP_DGRAD) else (cout, cin)
    ck = elem_chunk(dtype)
    return int(kd * kh * kw), -(-rows // 32) * 32, -(-cols // ck) * ck


def prep_op(kind: int, w: Tensor, out: Tensor, *, perm: Optional[Tensor] = None, cout=None, cin=None, k=None, phase_hw=(0, 0),
            sel_hw=(None, None), flip_d: bool = False, dgrad: bool = False, n: Optional[int] = None) -> "hip.PrepOp":
    """The rho_prep_op record (blk0 / nblk left 0) that writes layout ``kind`` of ``w`` into ``out`` - a pure function of its
    arguments (any device).  ``cout`` / ``cin`` / ``k`` default to ``w``'s own shape; a caller that re-reads a parameter under
    another geometry passes them, and every extent the device will index is checked here against what the tensors hold.
    PREP_VEC: out.flat[i] = w.flat[perm[i] if perm else i] for i < n (default: all of w), zero beyond; ``cin`` = source length."""
    def bad(why):
        return RhoHipError(f"prep_op kind {kind}: {why} (w {tuple(w.shape)}, out {tuple(out.shape)} {out.dtype})")
    if w.dtype != torch.float32 or not w.is_contiguous():
        raise bad(f"the source must be contiguous float32, got {w.dtype} contiguous={w.is_contiguous()}")
    if not out.is_contiguous():
        raise bad("out is not contiguous")
    if perm is not None and (perm.dtype != torch.int32 or not perm.is_contiguous()):
        raise bad("the index table must be contiguous int32")
    op = hip.PrepOp()
    op.w, op.out, op.perm = w.data_ptr(), out.data_ptr(), (perm.data_ptr() if perm is not None else None)
    op.kind, op.dtype, op.total = kind, dtype_code(out.dtype), out.numel()
    op.kd = op.kh = op.kw = 1
    if kind == hip.PREP_VEC:
        op.cout, op.cin = (w.numel() if n is None else int(n)), (w.numel() if cin is None else int(cin))
        op.d1, op.d2 = out.numel(), 1
        if w.numel() < op.cin:
            raise bad(f"a source of {op.cin} elements is read, it holds {w.numel()}")
        if op.cout > out.numel() or (perm is not None and perm.numel() < op.cout):
            raise bad(f"n = {op.cout} elements are written, out holds {out.numel()}, the index table {perm.numel() if perm is not None else '-'}")
        return op
    if out.dim() != 3:
        raise bad("out must be [taps, d1, d2]")
    op.cout, op.cin = int(w.shape[0] if cout is None else cout), int(w.shape[1] if cin is None else cin)
    op.kd, op.kh, op.kw = kd, kh, kw = tuple(int(v) for v in (kernel3(w) if k is None else k))
    op.d1, op.d2 = int(out.shape[1]), int(out.shape[2])
    taps2 = kd * kh * kw
    if kind == hip.PREP_PHASE:
        op.ph_h, op.ph_w, op.dgrad = int(phase_hw[0]), int(phase_hw[1]), int(dgrad)
        taps2 = kd * (2 if op.ph_h else kh) * (2 if op.ph_w else kw)
    elif kind == hip.PREP_SEL:
        sh, sw = _sel_taps(sel_hw, (kd, kh, kw))
        op.kh2, op.kw2, op.sel_h, op.sel_w, op.flip_d, op.dgrad = len(sh), len(sw), sel_code(sh), sel_code(sw), int(flip_d), int(dgrad)
        taps2 = kd * len(sh) * len(sw)
    if op.cout <= 0 or op.cin <= 0 or op.cout * op.cin * kd * kh * kw > w.numel():
        raise bad(f"read as {op.cout} x {op.cin} x {kd}x{kh}x{kw} = {op.cout * op.cin * kd * kh * kw} elements, the source holds {w.numel()}")
    if taps2 * op.d1 * op.d2 != out.numel():
        raise bad(f"the layout has {taps2} taps: {taps2 * op.d1 * op.d2} elements, out holds {out.numel()}")
    real1, real2 = (op.cin, op.cout) if (kind == hip.PREP_DGRAD or op.dgrad) else (op.cout, op.cin)
    if op.d2 < real2 or (op.d1 < real1 and not (kind == hip.PREP_FWD and perm is not None)):
        raise bad(f"out does not hold [{taps2}, >={real1}, >={real2}]")
    if perm is not None and perm.numel() < (op.d1 if kind == hip.PREP_FWD else op.cout):
        raise bad(f"the index table has {perm.numel()} entries")
    return op


class PrepSink:
    """``add_*``: one method per layout kind, shared by PrepTable and EagerPrep (which say in ``_push`` what becomes of a record).
    ``geo`` = cout / cin / k of prep_op: the geometry under which the parameter is read, when it is not its own shape."""

    def add_fwd(self, w: Tensor, out: Tensor, row_src: Optional[Tensor] = None, **geo):
        self._push(prep_op(hip.PREP_FWD, w, out, perm=row_src, **geo), w, out, row_src)

    def add_dgrad(self, w: Tensor, out: Tensor, col_src: Optional[Tensor] = None, **geo):
        self._push(prep_op(hip.PREP_DGRAD, w, out, perm=col_src, **geo), w, out, col_src)

    def add_phase(self, w: Tensor, out: Tensor, phase_hw, dgrad: bool = False, **geo):
        self._push(prep_op(hip.PREP_PHASE, w, out, phase_hw=phase_hw, dgrad=dgrad, **geo), w, out, None)

    def add_sel(self, w: Tensor, out: Tensor, sel_hw, flip_d: bool = False, dgrad: bool = False, **geo):
        self._push(prep_op(hip.PREP_SEL, w, out, sel_hw=sel_hw, flip_d=flip_d, dgrad=dgrad, **geo), w, out, None)

    def add_vec(self, src: Tensor, out: Tensor, perm: Optional[Tensor] = None, n: Optional[int] = None):
        """out.flat[i] = src.flat[perm[i] if perm else i] for i < n (default: all of src; perm[i] < 0: zero), zeros up to out.numel();
        src float32, out float32 or bf16 - a general gather (padded biases, plain copies, layouts no other kind describes)."""
        self._push(prep_op(hip.PREP_VEC, src, out, perm=perm, n=n), src, out, perm)


class EagerPrep(PrepSink):
    """Every layout at once through the per-tensor entry point of its kind (parameters the table cannot read in place, and the
    stand-alone ops.prep_conv_weight* calls)."""

    def _push(self, op, w: Tensor, out: Tensor, perm: Optional[Tensor]):
        hip.require_gpu(w, "w")
        hip.require_gpu(out, "out")
        k, pads = (op.kd, op.kh, op.kw), ((op.d2, op.d1) if op.dgrad else (op.d1, op.d2)) + (op.dgrad,)      # (coutp, cinp, dgrad)
        name, args = {hip.PREP_FWD: ("", (k[0] * k[1] * k[2], op.d1, op.d2, op.perm)),
                      hip.PREP_DGRAD: ("_dgrad", (k[0] * k[1] * k[2], op.d1, op.d2, op.perm)),
                      hip.PREP_PHASE: ("_phase", k + (op.ph_h, op.ph_w) + pads),
                      hip.PREP_SEL: ("_sel", k + (op.kh2, op.kw2, op.sel_h, op.sel_w, op.flip_d) + pads)}[op.kind]
        fn = getattr(hip.lib(), "rho_prep_conv_weight" + name)
        check(fn(op.w, op.out, op.dtype, op.cout, op.cin, *args, stream()), "rho_prep_conv_weight" + name)

    def add_vec(self, src: Tensor, out: Tensor, perm: Optional[Tensor] = None, n: Optional[int] = None):
        """The gather in torch (data movement only: it has no per-tensor entry point)."""
        op = prep_op(hip.PREP_VEC, src, out, perm=perm, n=n)
        src, flat = src.reshape(-1), out.view(-1)
        idx = perm[:op.cout].long() if perm is not None else torch.arange(op.cout, device=src.device)
        got = torch.where((idx >= 0) & (idx < op.cin), src[idx.clamp(0, op.cin - 1)], torch.zeros((), device=src.device))
        flat[:op.cout].copy_(got)
        flat[op.cout:].zero_()


def prep_conv_weight(w: Tensor, dtype: torch.dtype, coutp: Optional[int] = None, cinp: Optional[int] = None,
                     row_src: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """PyTorch conv weight [Cout, Cin, *k] float32 -> [taps, CoutP, CinP] in the engine dtype."""
    taps, d1, d2 = prepared_shape(hip.PREP_FWD, w, dtype)
    out = torch.empty(taps, coutp or d1, cinp or d2, dtype=dtype, device=w.device) if out is None else out
    if row_src is not None and (row_src.dtype != torch.int32 or row_src.numel() != out.shape[1]):
        raise RhoHipError("row_src must be int32[coutp]")
    EagerPrep().add_fwd(w, out, row_src)
    return out


def prep_conv_weight_dgrad(w: Tensor, dtype: torch.dtype, col_src: Optional[Tensor] = None,
                           out: Optional[Tensor] = None) -> Tensor:
    """PyTorch conv weight [Cout, Cin, *k] -> dgrad weights [taps, ceil32(Cin), ceilCK(Cout)] (flipped, transposed); a given
    ``out`` [taps, rows, cols] sets the padded extents."""
    out = torch.empty(prepared_shape(hip.PREP_DGRAD, w, dtype), dtype=dtype, device=w.device) if out is None else out
    EagerPrep().add_dgrad(w, out, col_src)
    return out


def prep_conv_weight_phase(w: Tensor, dtype: torch.dtype, phase_hw: Tuple[int, int], out: Optional[Tensor] = None,
                           dgrad: bool = False) -> Tensor:
    """Weights of one sub-pixel phase of a conv behind a nearest x2 upsample (rho_conv_desc.ph_h / ph_w): parameter
    [Cout, Cin, *k] (k = 3 on a phased axis) -> [kd * kh' * kw', CoutP, CinP] with kh' / kw' = 2 on the phased axes; dgrad: the
    data-gradient layout [taps, ceil32(Cin), ceilCK(Cout)] (flipped, transposed) for a launch with phd_h / phd_w."""
    out = torch.empty(prepared_shape(hip.PREP_PHASE, w, dtype, dgrad, phase_hw=phase_hw), dtype=dtype, device=w.device) if out is None else out
    EagerPrep().add_phase(w, out, phase_hw, dgrad=dgrad)
    return out


def prep_conv_weight_sel(w: Tensor, dtype: torch.dtype, sel_hw, *, flip_d: bool = False, dgrad: bool = False,
                         out: Optional[Tensor] = None) -> Tensor:
    """Tap selection of a 3-tap parameter for the parity splits of a stride-2 conv (rho_prep_conv_weight_sel): sel_hw = (taps of H,
    taps of W), each a tuple of source tap indices (None keeps the axis)."""
    out = torch.empty(prepared_shape(hip.PREP_SEL, w, dtype, dgrad, sel_hw=sel_hw), dtype=dtype, device=w.device) if out is None else out
    EagerPrep().add_sel(w, out, sel_hw, flip_d=flip_d, dgrad=dgrad)
    return out


class PrepTable(PrepSink):
    """Device table of rho_prep_op for rho_prep_batch: every prepared weight layout / padded bias / fp32 copy of a model in one
    launch.  ``add_*`` mirror the per-tensor prep calls (same arguments, same results); ``launch()`` uploads the table once."""

    def __init__(self, device):
        self.device = device
        self.ops: list = []
        self.keep: list = []
        self._dev = None
        self._blocks = 0

    def _push(self, op, w: Tensor, out: Tensor, perm: Optional[Tensor]):
        hip.require_gpu(w, "w")
        op.blk0, op.nblk = self._blocks, max(1, min((op.total + 1023) // 1024, int(os.environ.get("RHO_PREP_MAX_BLOCKS", "2048"))))
        self._blocks += op.nblk
        self.ops.append(op)
        self.keep.append((w, out, perm))
        self._dev = None

    def launch(self) -> None:
        if not self.ops:
            return
        if self._dev is None:
            raw = b"".join(bytes(op) for op in self.ops)
            self._dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        check(hip.lib().rho_prep_batch(self._dev.data_ptr(), len(self.ops), self._blocks, stream()), "rho_prep_batch")


class WfinTable:
    """Device table of rho_wfin_op for rho_wgrad_finalize_batch: the accumulation regions of one arena into parameter gradients in
    one launch.  ``add`` records one region (offsets in floats from the arena's base), ``build`` resolves the pointers - the arena
    and the gradients may move between launches - and uploads the table, ``launch`` runs it."""

    def __init__(self, device):
        self.device = device
        self.entries: list = []
        self._dev = None
        self._blocks = 0

    def add(self, *, kind, off, cout, cin, coutp, cinb, k, rs=None, up_h=0, up_w=0, stride=0, nblk=None, **extra):
        """kind 0: [taps][coutp][cinb] -> grad[row_src(r)][ci][tap] (``rs``: pointer of an int32 row table or None);  kind 1: all
        sub-pixel phases (``stride`` floats apart) into the 3-tap gradient;  kind 2: the one-channel head's [tap][ci] rows with
        mirrored taps.  ``nblk`` overrides the op's share of the launch; other keywords (the owning parameter) are kept with the
        entry and not read here."""
        self.entries.append(dict(extra, kind=kind, off=off, rs=rs, cout=cout, cin=cin, coutp=coutp, cinb=cinb, k=tuple(k), up_h=up_h,
                                 up_w=up_w, stride=stride, nblk=nblk))
        self._dev = None

    def records(self, arena_ptr: int, grad_ptrs) -> list:
        """The host-side rho_wfin_op records (blk0 ascending and contiguous, op 0 at 0) and, as a side effect, the launch's blocks."""
        if len(grad_ptrs) != len(self.entries):
            raise RhoHipError(f"WfinTable: {len(grad_ptrs)} gradient pointers for {len(self.entries)} entries")
        recs, blk = [], 0
        for e, g in zip(self.entries, grad_ptrs):
            op = hip.WfinOp()
            op.dw, op.grad, op.row_src = arena_ptr + 4 * e["off"], g, e["rs"]
            op.cout, op.cin, op.coutp, op.cinb = e["cout"], e["cin"], e["coutp"], e["cinb"]
            op.kd, op.kh, op.kw = e["k"]
            op.total = e["cout"] * e["cin"] * e["k"][0] * e["k"][1] * e["k"][2]
            op.kind, op.up_h, op.up_w, op.phase_stride = e["kind"], e["up_h"], e["up_w"], e["stride"]
            op.nblk = max(1, min((op.total + 255) // 256, 512)) if e["nblk"] is None else int(e["nblk"])
            op.blk0 = blk
            blk += op.nblk
            recs.append(op)
        self._blocks = blk
        return recs

    def build(self, arena_ptr: int, grad_ptrs) -> None:
        raw = b"".join(bytes(op) for op in self.records(arena_ptr, grad_ptrs))
        self._dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)

    def launch(self, s=None) -> int:
        """Enqueue the launch on stream ``s`` (default: the current one) and return the library's status code."""
        if self._dev is None:
            raise RhoHipError("WfinTable.launch before build")
        return hip.lib().rho_wgrad_finalize_batch(self._dev.data_ptr(), len(self.entries), self._blocks, stream() if s is None else s)


# ----------------------------------------------------------------------------- GroupNorm
def gn_nblk(s: int) -> int:
    return int(hip.lib().rho_gn_nblk(s))


def gn_coeffs(x1: Tensor, x2: Optional[Tensor], gamma: Tensor, beta: Tensor, scale: Optional[Tensor] = None,
              shift: Optional[Tensor] = None, film_stride: int = 0, partials: Optional[Tensor] = None,
              a: Optional[Tensor] = None, b: Optional[Tensor] = None, stats: Optional[Tensor] = None):
    """GroupNorm(32) statistics of the (virtually concatenated) channels-last input and the folded
    per-(sample, channel) affine (a, b) consumed by the conv prologue."""
    N = x1.shape[0]
    c1 = x1.shape[-1]
    c2 = x2.shape[-1] if x2 is not None else 0
    S = x1.numel() // (N * c1)
    Cc = c1 + c2
    nblk = gn_nblk(S)
    dev = x1.device
    partials = torch.empty(N * nblk * (Cc // 8) * 16, dtype=torch.float32, device=dev) if partials is None else partials
    a = torch.empty(N, Cc, dtype=torch.float32, device=dev) if a is None else a
    b = torch.empty(N, Cc, dtype=torch.float32, device=dev) if b is None else b
    stats = torch.empty(N, 32, 2, dtype=torch.float32, device=dev) if stats is None else stats
    L = hip.lib()
    check(L.rho_gn_partial(ptr(x1), c1, ptr(x2), c2, dtype_code(x1.dtype), N, S, ptr(partials), stream()), "rho_gn_partial")
    check(L.rho_gn_finalize(ptr(partials), N, Cc, S, nblk, ptr(gamma), ptr(beta), ptr(scale), ptr(shift), film_stride,
                            ptr(stats), ptr(a), ptr(b), stream()), "rho_gn_finalize")
    return a, b, stats


def gn_apply_launch(x1: Tensor, x2: Optional[Tensor], pre: dict, act: int, out: Tensor, drop=None, drop_ctr: Optional[Tensor] = None):
    """Launch closure (stream -> rc) of out = act(a * concat(x1, x2) + b) with the folded affine of ``pre`` (rho_gn_apply), or,
    with ``drop`` = (p, seed, ...), the same pass under the Philox mask keyed by (seed, drop_ctr) (rho_gn_apply_drop)."""
    c1 = x1.shape[-1]
    c2 = x2.shape[-1] if x2 is not None else 0
    a = (ptr(x1), c1, ptr(x2), c2, dtype_code(x1.dtype), x1.shape[0], x1.shape[1] * x1.shape[2] * x1.shape[3], ptr(pre["a"]),
         ptr(pre["b"]), int(act), ptr(out))
    L = hip.lib()
    if drop is None:
        return lambda s: L.rho_gn_apply(*a, s)
    ad = a + (float(drop[0]), int(drop[1]), ptr(drop_ctr))
    return lambda s: L.rho_gn_apply_drop(*ad, s)


# ----------------------------------------------------------------------------- convolution
def make_conv_desc(x1: Tensor, x2: Optional[Tensor], w: Tensor, bias: Tensor, *, kernel: Tuple[int, int, int],
                   cout: int, split: int, y: Optional[Tensor], y2: Optional[Tensor], stride_hw=(1, 1), up_hw=(0, 0),
                   pre_a: Optional[Tensor] = None, pre_b: Optional[Tensor] = None, pre_silu: bool = False,
                   res: Optional[Tensor] = None, res_add: Optional[Tensor] = None, res_add_stride: int = 0,
                   y2_cl: bool = False, res2: Optional[Tensor] = None, zs_hw=(0, 0), out_hw=(0, 0), phase_hw=(0, 0),
                   phase_dgrad_hw=(0, 0), skip: Optional[tuple] = None) -> ConvDesc:
    N, D, H, W, c1 = x1.shape
    d = ConvDesc()
    d.x1, d.x2 = ptr(x1), ptr(x2)
    d.pre_a, d.pre_b = ptr(pre_a), ptr(pre_b)
    d.w, d.bias = ptr(w), ptr(bias)
    d.res, d.res_add = ptr(res), ptr(res_add)
    d.y, d.y2 = ptr(y), ptr(y2)
    d.dtype = dtype_code(x1.dtype)
    d.y2_f32 = int(y2 is not None and y2.dtype == torch.float32)
    d.c1 = c1
    d.c2 = x2.shape[-1] if x2 is not None else 0
    d.cout, d.coutp, d.split = cout, w.shape[1], split
    d.n, d.d, d.h, d.w_ = N, D, H, W
    d.kd, d.kh, d.kw = kernel
    d.sh, d.sw = stride_hw
    d.up_h, d.up_w = up_hw
    d.pre_silu = int(pre_silu)
    d.res_add_stride = res_add_stride
    d.y2_cl = int(y2_cl)
    d.res2 = ptr(res2)
    d.zs_h, d.zs_w = int(zs_hw[0]), int(zs_hw[1])
    d.out_h, d.out_w = int(out_hw[0]), int(out_hw[1])
    d.ph_h, d.ph_w = int(phase_hw[0]), int(phase_hw[1])
    d.phd_h, d.phd_w = int(phase_dgrad_hw[0]), int(phase_dgrad_hw[1])
    if d.phd_h:                                        # x1 is the full-resolution dY: the launch's grid is the source resolution
        d.h = H // 2
    if d.phd_w:
        d.w_ = W // 2
    if w.shape[2] != d.c1 + d.c2:
        raise RhoHipError(f"conv: prepared weight has {w.shape[2]} input channels, inputs provide {d.c1 + d.c2}")
    if skip is not None:
        # (sx1, sx2, prepared 1x1x1 weights [1, coutp, c], bias): out += W_skip . cat(sx1, sx2) + b_skip inside this launch (rho_conv_desc.sk_*)
        sx1, sx2, sw, sb = skip
        d.sk_x1, d.sk_x2, d.sk_w, d.sk_bias = ptr(sx1), ptr(sx2), ptr(sw), ptr(sb)
        d.sk_c1 = sx1.shape[-1]
        d.sk_c2 = sx2.shape[-1] if sx2 is not None else 0
        if sw.shape[0] != 1 or sw.shape[1] != w.shape[1] or sw.shape[2] != d.sk_c1 + d.sk_c2:
            raise RhoHipError(f"conv: folded skip weights {tuple(sw.shape)} do not match coutp {w.shape[1]} / {d.sk_c1 + d.sk_c2} input channels")
    return d


def conv_out_shape(x_shape, kernel, stride_hw, up_hw):
    N, D, H, W, _ = x_shape
    kd, kh, kw = kernel
    ho = H * 2 if up_hw[0] else (H + 2 * (kh // 2) - kh) // stride_hw[0] + 1
    wo = W * 2 if up_hw[1] else (W + 2 * (kw // 2) - kw) // stride_hw[1] + 1
    return N, D, ho, wo


def conv_stats_tiles(desc: ConvDesc) -> int:
    """Tiles per sample of the fused output statistics of ``desc`` (0: not available for this geometry)."""
    return int(hip.lib().rho_conv_stats_tiles(C.byref(desc)))


def stem_conv3d_tiles(d: int, h: int, w: int) -> int:
    return int(hip.lib().rho_stem_conv3d_tiles(d, h, w))


def stem_conv3d(x: Tensor, w: Tensor, bias: Tensor, y: Tensor, stats: Optional[Tensor] = None) -> None:
    """rho_stem_conv3d: x float32 [N, 1, D, H, W] -> y bf16 channels-last [N, D, H, W, cout]; w = prepared im2col-form weights
    [1, coutp, 32]; stats (optional) float32 [N, stem_conv3d_tiles(D, H, W), 2, cout]."""
    hip.require_gpu(x, "x")
    N, _, D, H, W = x.shape
    check(hip.lib().rho_stem_conv3d(ptr(x), ptr(w), ptr(bias), ptr(y), ptr(stats), N, D, H, W, y.shape[-1], stream()), "rho_stem_conv3d")


def head_conv3d(x: Tensor, pre_a: Optional[Tensor], pre_b: Optional[Tensor], pre_silu: bool, w: Tensor, bias: Optional[Tensor],
                out: Tensor) -> None:
    """rho_head_conv3d: x bf16 channels-last [N, D, H, W, C] -> out float32 [N, 1, D, H, W]; w = prepared taps-as-rows weights [1, 32, C]."""
    hip.require_gpu(x, "x")
    N, D, H, W, Cc = x.shape
    check(hip.lib().rho_head_conv3d(ptr(x), ptr(pre_a), ptr(pre_b), int(pre_silu), ptr(w), ptr(bias), ptr(out), N, D, H, W, Cc, stream()),
          "rho_head_conv3d")


def conv_workspace_bytes(desc: ConvDesc) -> int:
    """Bytes of workspace the k-split of ``desc`` wants (rho_conv_desc.ws); 0: the launch is not split."""
    return int(hip.lib().rho_conv_workspace_bytes(C.byref(desc)))


def attach_conv_workspace(descs, device) -> Optional[Tensor]:
    """One workspace for all of ``descs`` (stream-ordered launches share it): the largest any of them wants, or None."""
    want = [conv_workspace_bytes(d) for d in descs]
    if not want or max(want) == 0:
        return None
    ws = torch.empty(max(want), dtype=torch.uint8, device=device)
    for d, b in zip(descs, want):
        if b:
            d.ws, d.ws_bytes = ptr(ws), ws.numel()
    return ws


def conv_variant(desc: ConvDesc) -> str:
    """Name of the k_conv instantiation rho_conv_nd_fwd launches for ``desc`` (nothing is launched)."""
    buf = C.create_string_buffer(128)
    check(hip.lib().rho_conv_variant(C.byref(desc), buf, 128), "rho_conv_variant")
    return buf.value.decode()


def conv_variant_detail(desc: ConvDesc) -> str:
    """The string rho_conv_variant leaves behind the variant name's terminating NUL: ``"geo=1"`` where the launch runs the
    compile-time 4 x 8 x 8 tile form of its instantiation, ``"geo=0"`` otherwise."""
    buf = C.create_string_buffer(128)
    check(hip.lib().rho_conv_variant(C.byref(desc), buf, 128), "rho_conv_variant")
    return buf.raw[len(buf.value) + 1:].split(b"\0", 1)[0].decode()


def conv_wgrad_variant(desc: ConvDesc, dy_width: int) -> str:
    buf = C.create_string_buffer(128)
    check(hip.lib().rho_conv_wgrad_variant(C.byref(desc), dy_width, buf, 128), "rho_conv_wgrad_variant")
    return buf.value.decode()


def conv_launch(desc: ConvDesc) -> None:
    check(hip.lib().rho_conv_nd_fwd(C.byref(desc), stream()), "rho_conv_nd_fwd")


def conv(x1: Tensor, x2: Optional[Tensor], w: Tensor, bias: Tensor, *, kernel, cout: int, split: Optional[int] = None,
         stride_hw=(1, 1), up_hw=(0, 0), pre_a=None, pre_b=None, pre_silu=False, res=None, res_add=None,
         res_add_stride: int = 0, y2_dtype: Optional[torch.dtype] = None):
    """Allocate outputs and run one convolution. Returns (y channels-last or None, y2 channel-major or None)."""
    split = cout if split is None else split
    N, Do, Ho, Wo = conv_out_shape(x1.shape, kernel, stride_hw, up_hw)
    y = torch.empty(N, Do, Ho, Wo, split, dtype=x1.dtype, device=x1.device) if split > 0 else None
    y2 = None
    if split < cout:
        y2 = torch.empty(N, cout - split, Do * Ho * Wo, dtype=y2_dtype or x1.dtype, device=x1.device)
    d = make_conv_desc(x1, x2, w, bias, kernel=kernel, cout=cout, split=split, y=y, y2=y2, stride_hw=stride_hw, up_hw=up_hw,
                       pre_a=pre_a, pre_b=pre_b, pre_silu=pre_silu, res=res, res_add=res_add, res_add_stride=res_add_stride)
    ws = attach_conv_workspace([d], x1.device)      # (freed to the caching allocator on return: reuse is ordered on this stream)
    conv_launch(d)
    return y, y2


# ----------------------------------------------------------------------------- attention
def attention(qk: Tensor, vt: Tensor, heads: int, out: Optional[Tensor] = None, lse: Optional[Tensor] = None) -> Tensor:
    """qk channels-last [B, T, 2C], vt channel-major [B, C, T] -> channels-last [B, T, C].
    lse (optional float32 [B, heads, T]) receives the per-query log-sum-exp for the backward."""
    B, T, C2 = qk.shape
    Cc = C2 // 2
    ch = Cc // heads
    out = torch.empty(B, T, Cc, dtype=qk.dtype, device=qk.device) if out is None else out
    check(hip.lib().rho_attention_fwd(ptr(qk), ptr(vt), ptr(out), ptr(lse), dtype_code(qk.dtype), B, T, heads, ch, stream()),
          "rho_attention_fwd")
    return out


def attention_variant(dtype: torch.dtype, ch: int, backward: bool = False) -> str:
    """Names of the kernels ``attention`` (``attention_bwd`` with ``backward``) launches for this dtype and head width, joined
    with ``+`` in launch order (nothing is launched, no GPU is needed)."""
    buf = C.create_string_buffer(128)
    check(hip.lib().rho_attention_variant(dtype_code(dtype), int(ch), int(bool(backward)), buf, 128), "rho_attention_variant")
    return buf.value.decode()


# ============================================================================= backward ops
def conv_wgrad(desc: ConvDesc, dy: Tensor, dw: Tensor, dbias: Optional[Tensor] = None) -> None:
    """Accumulate the weight gradient of the forward conv `desc` into the fp32 buffer dw [taps, coutp, cin] (and, when given,
    the channel sums of dy = the bias gradient into dbias [coutp])."""
    if deterministic():
        need = int(hip.lib().rho_conv_wgrad_workspace_bytes(C.byref(desc), dy.shape[-1]))
        ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dy.device)
        check(hip.lib().rho_conv_nd_wgrad_ws(C.byref(desc), ptr(dy), dy.shape[-1], ptr(dw), ptr(dbias), ptr(ws), need, stream()),
              "rho_conv_nd_wgrad_ws")
        return
    check(hip.lib().rho_conv_nd_wgrad(C.byref(desc), ptr(dy), dy.shape[-1], ptr(dw), ptr(dbias), stream()), "rho_conv_nd_wgrad")


def wgrad_finalize(dw: Tensor, grad: Tensor, row_src: Optional[Tensor] = None, accumulate: bool = False) -> None:
    cout, cin = grad.shape[0], grad.shape[1]
    taps = grad.numel() // (cout * cin)
    check(hip.lib().rho_wgrad_finalize(ptr(dw), ptr(grad), cout, cin, taps, dw.shape[1], dw.shape[2], ptr(row_src), int(accumulate),
                                       stream()), "rho_wgrad_finalize")


def gn_bwd(g: Tensor, x1: Tensor, x2: Optional[Tensor], a: Tensor, b: Tensor, stats: Tensor, gamma: Tensor, beta: Tensor,
           pre_silu: bool, dx1: Tensor, dx2: Optional[Tensor], dgamma: Tensor, dbeta: Tensor, *, scale=None, film_stride=0,
           dscale=None, dshift=None, dfilm_stride=0, acc_params=False, acc1=False, acc2=False, ws=None, add1: Optional[Tensor] = None):
    """Backward of act(GN(x)*(1+scale)+shift); scale/dscale/dshift may be raw pointers (ints) or tensors.  ``add1``: a further
    addend of dx1 (a residual connection's gradient) folded into the apply pass."""
    N = x1.shape[0]
    c1 = x1.shape[-1]
    c2 = x2.shape[-1] if x2 is not None else 0
    Cc = c1 + c2
    S = x1.numel() // (N * c1)
    nblk = gn_nblk(S)
    dev = x1.device
    if ws is None:
        ws = dict(part=torch.empty(N * nblk * (Cc // 8) * 16, dtype=torch.float32, device=dev),
                  work=torch.empty(2 * N * Cc, dtype=torch.float32, device=dev),
                  cA=torch.empty(N, Cc, dtype=torch.float32, device=dev), cP=torch.empty(N, 32, dtype=torch.float32, device=dev),
                  cQ=torch.empty(N, 32, dtype=torch.float32, device=dev))
    L = hip.lib()
    dt = dtype_code(x1.dtype)
    p = lambda t: t if isinstance(t, int) or t is None else t.data_ptr()  # noqa: E731
    check(L.rho_gn_bwd_reduce(ptr(g), ptr(x1), c1, ptr(x2), c2, dt, N, S, ptr(a), ptr(b), ptr(stats), int(pre_silu), ptr(ws["part"]),
                              stream()), "rho_gn_bwd_reduce")
    check(L.rho_gn_bwd_finalize(ptr(ws["part"]), N, Cc, S, nblk, 0, ptr(gamma), ptr(beta), p(scale), film_stride, ptr(stats),
                                ptr(ws["work"]), ptr(dgamma), ptr(dbeta), int(acc_params), p(dscale), p(dshift), dfilm_stride,
                                ptr(ws["cA"]), ptr(ws["cP"]), ptr(ws["cQ"]), stream()), "rho_gn_bwd_finalize")
    check(L.rho_gn_bwd_apply(ptr(g), ptr(x1), c1, ptr(x2), c2, dt, N, S, ptr(a), ptr(b), int(pre_silu), ptr(ws["cA"]), ptr(ws["cP"]),
                             ptr(ws["cQ"]), ptr(dx1), ptr(dx2), int(acc1), int(acc2), ptr(add1), stream()), "rho_gn_bwd_apply")


def chan_sum(x: Tensor, out_nc: Tensor, out_c: Optional[Tensor] = None, nc_stride: int = 0, acc_nc=False, acc_c=False,
             partials: Optional[Tensor] = None) -> None:
    N, Cc = x.shape[0], x.shape[-1]
    S = x.numel() // (N * Cc)
    nblk = gn_nblk(S)
    partials = torch.empty(N * nblk * (Cc // 8) * 16, dtype=torch.float32, device=x.device) if partials is None else partials
    onc = out_nc if isinstance(out_nc, int) else out_nc.data_ptr()
    check(hip.lib().rho_chan_sum(ptr(x), dtype_code(x.dtype), N, S, Cc, ptr(partials), onc, nc_stride, int(acc_nc), ptr(out_c),
                                 int(acc_c), stream()), "rho_chan_sum")


def upsample2x(x: Tensor, up_hw, out: Optional[Tensor] = None) -> Tensor:
    N, D, H, W, Cc = x.shape
    out = torch.empty(N, D, H * (2 if up_hw[0] else 1), W * (2 if up_hw[1] else 1), Cc, dtype=x.dtype, device=x.device) if out is None else out
    check(hip.lib().rho_upsample2x(ptr(x), ptr(out), dtype_code(x.dtype), N * D, H, W, Cc, int(up_hw[0]), int(up_hw[1]), stream()),
          "rho_upsample2x")
    return out


def avgpool2x(x: Tensor, pool_hw, out: Optional[Tensor] = None) -> Tensor:
    """avg_pool_nd(kernel = stride = 2) over the flagged axes of a channels-last tensor (floor output extents)."""
    N, D, H, W, Cc = x.shape
    out = torch.empty(N, D, H // 2 if pool_hw[0] else H, W // 2 if pool_hw[1] else W, Cc, dtype=x.dtype, device=x.device) if out is None else out
    check(hip.lib().rho_avgpool2x(ptr(x), ptr(out), dtype_code(x.dtype), N * D, H, W, Cc, int(pool_hw[0]), int(pool_hw[1]), stream()),
          "rho_avgpool2x")
    return out


def avgpool2x_bwd(dy: Tensor, dx: Tensor, pool_hw, accumulate: bool = False) -> Tensor:
    N, D, H, W, Cc = dx.shape
    check(hip.lib().rho_avgpool2x_bwd(ptr(dy), ptr(dx), dtype_code(dx.dtype), N * D, H, W, Cc, int(pool_hw[0]), int(pool_hw[1]),
                                      int(accumulate), stream()), "rho_avgpool2x_bwd")
    return dx


def pool2x_sum(dy: Tensor, dx: Tensor, up_hw, accumulate: bool = False) -> Tensor:
    N, D, H, W, Cc = dx.shape
    check(hip.lib().rho_pool2x_sum(ptr(dy), ptr(dx), dtype_code(dx.dtype), N * D, H, W, Cc, int(up_hw[0]), int(up_hw[1]),
                                   int(accumulate), stream()), "rho_pool2x_sum")
    return dx


def linear_bwd(dout, x: Tensor, w: Tensor, dw: Optional[Tensor], db: Optional[Tensor], dx: Optional[Tensor],
               act_in: int = 0, acc_params: bool = False, acc_dx: bool = False, dout_stride: int = 0) -> None:
    """dout may be a tensor or a raw device pointer (a column slice of the batched FiLM gradient).  ``act_in``: activation code
    (see ACT_CODES; True is SiLU)."""
    B, K = x.shape
    O = w.shape[0]
    dp = dout if isinstance(dout, int) else dout.data_ptr()
    check(hip.lib().rho_linear_bwd(dp, dout_stride, ptr(x), ptr(w), ptr(dw), ptr(db), ptr(dx), B, K, O, int(act_in),
                                   int(acc_params), int(acc_dx), stream()), "rho_linear_bwd")


def add_inplace(dst: Tensor, src: Tensor) -> None:
    check(hip.lib().rho_add_inplace(ptr(dst), ptr(src), dtype_code(dst.dtype), dst.numel(), stream()), "rho_add_inplace")


def attention_bwd(qk: Tensor, vt: Tensor, o: Tensor, dout: Tensor, lse: Tensor, heads: int, dqkv: Optional[Tensor] = None,
                  delta_ws: Optional[Tensor] = None):
    """Returns dqkv channels-last [B, T, 3C] = (dq | dk | dv): the output gradient of the qkv projection."""
    B, T, C2 = qk.shape
    Cc = C2 // 2
    dqkv = torch.empty(B, T, 3 * Cc, dtype=qk.dtype, device=qk.device) if dqkv is None else dqkv
    delta_ws = torch.empty(B, heads, T, dtype=torch.float32, device=qk.device) if delta_ws is None else delta_ws
    esz = dqkv.element_size()
    check(hip.lib().rho_attention_bwd(ptr(qk), ptr(vt), ptr(o), ptr(dout), ptr(lse), ptr(delta_ws), dqkv.data_ptr(), 3 * Cc,
                                      dqkv.data_ptr() + 2 * Cc * esz, 3 * Cc, dtype_code(qk.dtype), B, T, heads, Cc // heads,
                                      stream()), "rho_attention_bwd")
    return dqkv


# ----------------------------------------------------------------------------- VisionTransformer (csrc/vit.hip)
def vit_kpad(k: int) -> int:
    """Row width of the patch tokens: K = C * p^dims padded to the multiple of 32 the GEMM reads and writes."""
    return ((int(k) + 31) // 32) * 32


def _rows2d(x: Tensor, name: str):
    hip.require_gpu(x, name)
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous() or x.dim() < 2:
        raise RhoHipError(f"{name} must be a contiguous float32 / bfloat16 [..., E] GPU tensor, got {x.dtype} {tuple(x.shape)}")
    return x.numel() // x.shape[-1], x.shape[-1]


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, add: Optional[Tensor] = None, out: Optional[Tensor] = None,
              stats: Optional[Tensor] = None):
    """(y, stats) = LayerNorm(x + add[sample]) * gamma + beta over the last axis of token rows x [B, N, E] (or [R, E]); ``add`` float32
    [B, E] with B dividing the row count; stats float32 [R, 2] = (mean, rstd) (rho_layernorm_fwd)."""
    R, E = _rows2d(x, "x")
    _f32c(gamma, "gamma"), _f32c(beta, "beta")
    rps = R
    if add is not None:
        _f32c(add, "add")
        if add.dim() != 2 or add.shape[1] != E or R % add.shape[0]:
            raise RhoHipError(f"add must be float32 [B, {E}] with B dividing {R} rows, got {tuple(add.shape)}")
        rps = R // add.shape[0]
    if gamma.numel() != E or beta.numel() != E:
        raise RhoHipError(f"gamma / beta must have {E} elements")
    out = torch.empty_like(x) if out is None else out
    stats = torch.empty(R, 2, dtype=torch.float32, device=x.device) if stats is None else stats
    check(hip.lib().rho_layernorm_fwd(ptr(x), ptr(add), ptr(gamma), ptr(beta), ptr(out), ptr(stats), dtype_code(x.dtype), R, rps, E, stream()),
          "rho_layernorm_fwd")
    return out, stats


def layernorm_bwd(dy: Tensor, x: Tensor, stats: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor, add: Optional[Tensor] = None,
                  dx: Optional[Tensor] = None, dadd: Optional[Tensor] = None, acc_dx: bool = False, acc_params: bool = False,
                  workspace: Optional[Tensor] = None):
    """Backward of ``layernorm``: returns (dx, dadd); dgamma / dbeta float32 [E] are written (acc_params: added to).  dx may be given
    (acc_dx: the result is added to it); dadd float32 [B, E] is produced when ``add`` is given (rho_layernorm_bwd)."""
    R, E = _rows2d(x, "x")
    if dy.shape != x.shape or dy.dtype != x.dtype or not dy.is_contiguous():
        raise RhoHipError("dy must match x in shape, dtype and be contiguous")
    _f32c(stats, "stats"), _f32c(gamma, "gamma"), _f32c(dgamma, "dgamma"), _f32c(dbeta, "dbeta")
    rps = R
    if add is not None:
        _f32c(add, "add")
        if add.dim() != 2 or add.shape[1] != E or R % add.shape[0]:
            raise RhoHipError(f"add must be float32 [B, {E}] with B dividing {R} rows, got {tuple(add.shape)}")
        rps = R // add.shape[0]
        dadd = torch.empty_like(add) if dadd is None else _f32c(dadd, "dadd")
    if dx is None:
        if acc_dx:
            raise RhoHipError("acc_dx needs the buffer to accumulate into")
        dx = torch.empty_like(x)
    need = int(hip.lib().rho_layernorm_bwd_workspace_bytes(R, rps, E, dtype_code(x.dtype), int(add is not None)))
    if need <= 0:
        raise RhoHipError(f"layernorm_bwd: unsupported shape rows={R} E={E}")
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    check(hip.lib().rho_layernorm_bwd(ptr(dy), ptr(x), ptr(add), ptr(stats), ptr(gamma), ptr(dx), int(acc_dx), ptr(dadd), ptr(dgamma),
                                      ptr(dbeta), int(acc_params), ptr(workspace), workspace.numel() * workspace.element_size(),
                                      dtype_code(x.dtype), R, rps, E, stream()), "rho_layernorm_bwd")
    return dx, dadd


def _patch_args(shape, p: int):
    B, Cc = int(shape[0]), int(shape[1])
    sp = [int(v) for v in shape[2:]]
    dims = len(sp)
    if not 1 <= dims <= 3:
        raise RhoHipError(f"patch kernels take 1-D / 2-D / 3-D data, got shape {tuple(shape)}")
    if any(s % p for s in sp):
        raise RhoHipError(f"spatial shape {sp} is not divisible by patch_size {p}")
    s3 = [1] * (3 - dims) + sp
    N = int(math.prod(s // p for s in sp))
    return B, Cc, dims, s3, N, Cc * p ** dims


def patchify(x: Tensor, p: int, dtype: torch.dtype, out: Optional[Tensor] = None, dbias: Optional[Tensor] = None,
             acc_dbias: bool = False) -> Tensor:
    """float32 [B, C, *spatial] -> tokens [B, N, Kp] in ``dtype`` (rho_patchify); ``dbias`` float32 [C] receives the channel sums."""
    _f32c(x, "x")
    B, Cc, dims, s3, N, K = _patch_args(x.shape, p)
    kp = vit_kpad(K)
    out = torch.empty(B, N, kp, dtype=dtype, device=x.device) if out is None else out
    ws = None
    if dbias is not None:
        if _f32c(dbias, "dbias").numel() != Cc:
            raise RhoHipError(f"dbias must be float32 [{Cc}]")
        ws = torch.empty(int(hip.lib().rho_patchify_dbias_workspace_bytes(Cc)) // 4, dtype=torch.float32, device=x.device)
    check(hip.lib().rho_patchify(ptr(x), ptr(out), dtype_code(dtype), B, Cc, dims, s3[0], s3[1], s3[2], int(p), kp, ptr(dbias),
                                 int(acc_dbias), ptr(ws), stream()), "rho_patchify")
    return out


def unpatchify(tokens: Tensor, shape, p: int, bias: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """tokens [B, N, Kp] -> float32 ``shape`` = [B, C, *spatial] (+ bias[c]) (rho_unpatchify)."""
    hip.require_gpu(tokens, "tokens")
    B, Cc, dims, s3, N, K = _patch_args(shape, p)
    kp = vit_kpad(K)
    if tuple(tokens.shape) != (B, N, kp) or not tokens.is_contiguous():
        raise RhoHipError(f"tokens must be contiguous [{B}, {N}, {kp}], got {tuple(tokens.shape)}")
    if bias is not None and _f32c(bias, "bias").numel() != Cc:
        raise RhoHipError(f"bias must be float32 [{Cc}]")
    out = torch.empty(tuple(int(v) for v in shape), dtype=torch.float32, device=tokens.device) if out is None else _f32c(out, "out")
    check(hip.lib().rho_unpatchify(ptr(tokens), ptr(bias), ptr(out), dtype_code(tokens.dtype), B, Cc, dims, s3[0], s3[1], s3[2], int(p), kp,
                                   stream()), "rho_unpatchify")
    return out


def bias_act(x: Tensor, act: int, bias: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """act(x + bias[c]) over the last axis (rho_bias_act); ``act``: an activation code (ACT_CODES)."""
    R, Cc = _rows2d(x, "x")
    out = torch.empty_like(x) if out is None else out
    check(hip.lib().rho_bias_act(ptr(x), ptr(bias), ptr(out), dtype_code(x.dtype), R, Cc, int(act), stream()), "rho_bias_act")
    return out


def bias_act_bwd(x: Tensor, dy: Tensor, act: int, bias: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """dy * act'(x + bias[c]) (rho_bias_act_bwd)."""
    R, Cc = _rows2d(x, "x")
    if dy.shape != x.shape or dy.dtype != x.dtype or not dy.is_contiguous():
        raise RhoHipError("dy must match x in shape, dtype and be contiguous")
    out = torch.empty_like(x) if out is None else out
    check(hip.lib().rho_bias_act_bwd(ptr(x), ptr(bias), ptr(dy), ptr(out), dtype_code(x.dtype), R, Cc, int(act), stream()), "rho_bias_act_bwd")
    return out


def pos_add(x: Tensor, pos: Tensor) -> Tensor:
    """x[b] += pos in place: x [B, N, E] in the engine dtype, pos float32 [N, E] (rho_pos_add)."""
    _rows2d(x, "x"), _f32c(pos, "pos")
    if pos.numel() * x.shape[0] != x.numel():
        raise RhoHipError(f"pos {tuple(pos.shape)} does not match x {tuple(x.shape)}")
    check(hip.lib().rho_pos_add(ptr(x), ptr(pos), dtype_code(x.dtype), x.shape[0], pos.numel(), stream()), "rho_pos_add")
    return x


def pos_add_bwd(dx: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """float32 [N, E] = sum over the batch of dx [B, N, E] (rho_pos_add_bwd)."""
    _rows2d(dx, "dx")
    out = torch.empty(tuple(dx.shape[1:]), dtype=torch.float32, device=dx.device) if out is None else _f32c(out, "out")
    check(hip.lib().rho_pos_add_bwd(ptr(dx), ptr(out), dtype_code(dx.dtype), dx.shape[0], out.numel(), stream()), "rho_pos_add_bwd")
    return out


# ----------------------------------------------------------------------------- sample metrics (csrc/sinkhorn.hip)
SINKHORN_MAX_SAMPLES = 128       # == rho_sinkhorn_max_samples()


def _sinkhorn_xy(x: Tensor, y: Tensor) -> Tuple[int, int, int]:
    """(N, M, D) of two float32 [rows, D] sample sets within the kernels' limits."""
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise RhoHipError(f"x and y must be [N, D] and [M, D], got {tuple(x.shape)} and {tuple(y.shape)}")
    N, M, D = int(x.shape[0]), int(y.shape[0]), int(x.shape[1])
    if not (1 <= N <= SINKHORN_MAX_SAMPLES and 1 <= M <= SINKHORN_MAX_SAMPLES) or D < 1:
        raise RhoHipError(f"the Sinkhorn kernels take 1 <= N, M <= {SINKHORN_MAX_SAMPLES} samples of D >= 1 values, got N = {N}, "
                          f"M = {M}, D = {D}")
    _f32c(x, "x"), _f32c(y, "y")
    return N, M, D


def sinkhorn_workspace(x: Tensor, y: Tensor) -> Tensor:
    """Scratch of rho_pairwise_cost / rho_max_diameter for this pair (float64), allocated in stream order."""
    N, M, D = _sinkhorn_xy(x, y)
    nbytes = int(hip.lib().rho_pairwise_cost_workspace_bytes(N, M, D))
    if nbytes < 0:
        raise RhoHipError("rho_pairwise_cost_workspace_bytes refused the shape")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)


def pairwise_cost(x: Tensor, y: Tensor, p: int, workspace: Optional[Tensor] = None, dtype: torch.dtype = torch.float32):
    """(C_xy [N, M], C_xx [N, N], C_yy [M, M]) of rho_pairwise_cost: sqrt(max(d2, 1e-8)) for p = 1, d2 / 2 for p = 2.  ``dtype``
    float32, or float64: the matrices rho_sinkhorn_loop reads (the sums run in float64 either way)."""
    N, M, D = _sinkhorn_xy(x, y)
    if dtype not in (torch.float32, torch.float64):
        raise RhoHipError(f"pairwise_cost returns float32 or float64 matrices, not {dtype}")
    ws = sinkhorn_workspace(x, y) if workspace is None else workspace
    if ws.dtype != torch.float64 or not ws.is_cuda:
        raise RhoHipError("workspace must be a float64 GPU tensor (sinkhorn_workspace)")

    def split(buf):
        return buf[:N * M].view(N, M), buf[N * M:N * M + N * N].view(N, N), buf[N * M + N * N:].view(M, M)

    buf = torch.empty(N * M + N * N + M * M, dtype=torch.float32, device=x.device)
    buf64 = torch.empty(N * M + N * N + M * M, dtype=torch.float64, device=x.device) if dtype == torch.float64 else None
    c_xy, c_xx, c_yy = split(buf)
    check(hip.lib().rho_pairwise_cost(ptr(x), ptr(y), N, M, D, int(p), ptr(c_xy), ptr(c_xx), ptr(c_yy), ptr(buf64), ptr(ws),
                                      ws.numel() * 8, stream()), "rho_pairwise_cost")
    return split(buf64) if buf64 is not None else (c_xy, c_xx, c_yy)


def max_diameter(x: Tensor, y: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
    """float64 [1]: the norm of the per-coordinate extent of [x; y] (rho_max_diameter)."""
    N, M, D = _sinkhorn_xy(x, y)
    ws = sinkhorn_workspace(x, y) if workspace is None else workspace
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    check(hip.lib().rho_max_diameter(ptr(x), ptr(y), N, M, D, ptr(out), ptr(ws), ws.numel() * 8, stream()), "rho_max_diameter")
    return out


def sinkhorn_loop(c_xy: Tensor, c_xx: Tensor, c_yy: Tensor, eps_list: Tensor, p: int, debias: bool = True, want_weights: bool = False):
    """The whole epsilon schedule in one launch (rho_sinkhorn_loop) from float64 cost matrices (pairwise_cost(..., dtype=torch.float64))
    and a float64 schedule on the device.  Returns a dict of float32 tensors: f_ba, f_aa, h_a [N]; g_ab,
    g_bb, h_b [M]; loss [1]; with ``want_weights`` also wp [N, M], wq [N, N], rp, rq [N]."""
    for name, t in (("c_xy", c_xy), ("c_xx", c_xx), ("c_yy", c_yy), ("eps_list", eps_list)):
        hip.require_gpu(t, name)
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise RhoHipError(f"{name} must be contiguous float64, got {t.dtype} contiguous={t.is_contiguous()}")
    N, M = int(c_xy.shape[0]), int(c_xy.shape[1])
    if tuple(c_xx.shape) != (N, N) or tuple(c_yy.shape) != (M, M) or eps_list.numel() < 1:
        raise RhoHipError("c_xy [N, M], c_xx [N, N], c_yy [M, M] and a non-empty eps_list are required")
    buf = torch.empty(3 * N + 3 * M + 1, dtype=torch.float32, device=c_xy.device)
    o = {"f_ba": buf[:N], "f_aa": buf[N:2 * N], "h_a": buf[2 * N:3 * N], "g_ab": buf[3 * N:3 * N + M],
         "g_bb": buf[3 * N + M:3 * N + 2 * M], "h_b": buf[3 * N + 2 * M:3 * N + 3 * M], "loss": buf[3 * N + 3 * M:]}
    if want_weights:
        w = torch.empty(N * M + N * N + 2 * N, dtype=torch.float32, device=c_xy.device)
        o.update(wp=w[:N * M].view(N, M), wq=w[N * M:N * M + N * N].view(N, N), rp=w[N * M + N * N:N * M + N * N + N],
                 rq=w[N * M + N * N + N:])
    check(hip.lib().rho_sinkhorn_loop(ptr(c_xy), ptr(c_xx), ptr(c_yy), N, M, ptr(eps_list), eps_list.numel(), int(p), 1 if debias else 0,
                                      ptr(o["f_ba"]), ptr(o["g_ab"]), ptr(o["f_aa"]), ptr(o["g_bb"]), ptr(o["h_b"]), ptr(o["h_a"]),
                                      ptr(o["loss"]), ptr(o.get("wp")), ptr(o.get("wq")), ptr(o.get("rp")), ptr(o.get("rq")), stream()),
          "rho_sinkhorn_loop")
    return o


def rows_combine(x: Tensor, y: Tensor, wp: Tensor, wq: Tensor, rp: Tensor, rq: Tensor, g_out: Tensor) -> Tensor:
    """grad_x [N, D] of the Sinkhorn loss from the last step's weights (rho_rows_combine); g_out: float32 [1] on the device."""
    N, M, D = _sinkhorn_xy(x, y)
    for name, t, numel in (("wp", wp, N * M), ("wq", wq, N * N), ("rp", rp, N), ("rq", rq, N), ("g_out", g_out, 1)):
        if _f32c(t, name).numel() != numel:
            raise RhoHipError(f"{name} must hold {numel} float32 values")
    grad = torch.empty_like(x)
    check(hip.lib().rho_rows_combine(ptr(x), ptr(y), N, M, D, ptr(wp), ptr(wq), ptr(rp), ptr(rq), ptr(g_out), ptr(grad), stream()),
          "rho_rows_combine")
    return grad


def psnr(pred: Tensor, target: Tensor, data_range: Optional[float] = None) -> Tensor:
    """float32 [4] = (10 log10(range^2 / mse), mse, min(target), max(target)) from one fused reduction (rho_psnr); ``data_range``
    None: max - min of this target."""
    _f32c(pred, "pred")
    _same(pred, ("target", target))
    ws_bytes = int(hip.lib().rho_psnr_workspace_bytes())
    buf = torch.empty(4 + ws_bytes // 4, dtype=torch.float32, device=pred.device)
    check(hip.lib().rho_psnr(ptr(pred), ptr(target), pred.numel(), 0.0 if data_range is None else float(data_range), ptr(buf),
                             buf.data_ptr() + 16, ws_bytes, stream()), "rho_psnr")
    return buf[:4]


# ----------------------------------------------------------------------------- structural similarity (csrc/ssim.hip)
SSIM_MAX_WINDOW = 15             # == rho_ssim_max_window()


def ssim_range(pred: Tensor, target: Tensor, workspace: Optional[Tensor] = None) -> Tensor:
    """float32 [1] on the device: max(max(pred) - min(pred), max(target) - min(target)) (rho_ssim_range)."""
    _f32c(pred, "pred")
    _same(pred, ("target", target))
    ws = torch.empty(4096, dtype=torch.float32, device=pred.device) if workspace is None else workspace
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    check(hip.lib().rho_ssim_range(ptr(pred), ptr(target), pred.numel(), ptr(out), ptr(ws), ws.numel() * ws.element_size(), stream()),
          "rho_ssim_range")
    return out


def ssim(pred: Tensor, target: Tensor, windows: Sequence[Tensor], data_range=None, clamp: Optional[Tuple[float, float]] = None,
         k1: float = 0.01, k2: float = 0.03, return_map: bool = False, per_sample: Optional[Tensor] = None, out: Optional[Tensor] = None,
         map: Optional[Tensor] = None):
    """SSIM of two float32 fields [B, C, *spatial] over the windows wholly inside the field (rho_ssim).  ``windows``: one float32
    device tensor per spatial dimension.  ``data_range``: None (measured on the device by rho_ssim_range), a float, or a float32
    device tensor [1]; ``clamp`` (lo, hi): both inputs are clamped as they are loaded.  Returns (per_sample [B], out [2] = {mean,
    sum} over the batch, map or None); the map is float32 [B, C, *(size_d - k_d + 1)].  ``per_sample``, ``out``, ``map``: buffers to
    write into.  Shapes and windows are judged by the library: a refusal raises with its code and writes nothing.  Nothing is read
    back and nothing synchronises."""
    _f32c(pred, "pred")
    _same(pred, ("target", target))
    nd = pred.dim() - 2
    if nd < 1 or len(windows) != nd:
        raise RhoHipError(f"pred must be [B, C, *spatial] with one window per spatial dimension, got {tuple(pred.shape)} and "
                          f"{len(windows)} windows")
    for i, w in enumerate(windows):
        _f32c(w, f"windows[{i}]")
    B, Cn = int(pred.shape[0]), int(pred.shape[1])
    sizes = (C.c_int64 * nd)(*[int(v) for v in pred.shape[2:]])
    ks = (C.c_int64 * nd)(*[int(w.numel()) for w in windows])
    wptr = (C.c_void_p * nd)(*[w.data_ptr() for w in windows])
    dev = pred.device
    ws_bytes = int(hip.lib().rho_ssim_workspace_bytes(B, Cn, nd, sizes, ks))
    ws = torch.empty(max(ws_bytes, 16384) // 8, dtype=torch.float64, device=dev)
    mshape = (B, Cn) + tuple(max(int(s) - int(k) + 1, 1) for s, k in zip(sizes, ks))
    per_sample = torch.empty(B, dtype=torch.float32, device=dev) if per_sample is None else _f32c(per_sample, "per_sample")
    out = torch.empty(2, dtype=torch.float32, device=dev) if out is None else _f32c(out, "out")
    if map is None and return_map:
        map = torch.empty(mshape, dtype=torch.float32, device=dev)
    if per_sample.numel() < B or out.numel() < 2 or (map is not None and _f32c(map, "map").numel() < math.prod(mshape)):
        raise RhoHipError("per_sample [B], out [2] or map [B, C, *(size - k + 1)] is too small")
    range_dev, range_val = None, 0.0
    if data_range is None:
        range_dev = ssim_range(pred, target, ws)
    elif isinstance(data_range, Tensor):
        range_dev = _f32c(data_range, "data_range")
    else:
        range_val = float(data_range)
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    check(hip.lib().rho_ssim(ptr(pred), ptr(target), B, Cn, nd, sizes, wptr, ks, range_val, ptr(range_dev), 0 if clamp is None else 1,
                             lo, hi, float(k1), float(k2), ptr(per_sample), ptr(out), ptr(map), ptr(ws), ws.numel() * 8, stream()),
          "rho_ssim")
    return per_sample, out, map
