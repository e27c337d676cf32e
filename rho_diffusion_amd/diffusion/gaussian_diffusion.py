"""GaussianDiffusionPipeline: the pipeline ``scripts/inference.py:122`` instantiates (reference:
rho_diffusion/diffusion/gaussian_diffusion.py:145-1227).  Same constructor; the fixed configuration of the reference
(``diffusion_defaults``, :199-209): cosine betas, x0-prediction (``predict_xstart=True``), fixed-large variance,
MSE loss, no timestep rescaling.  Built here: the coefficient tables (:237-273), ``q_sample`` / ``forward_process``
(:294-312, :1014-1027) and the sampling path ``reverse_process`` (:1029-1099) = DDIM (eta = 0, :654-702) on top of
``p_mean_variance`` with dynamic thresholding (:400-415).

Arithmetic in librho_hip.so:
  * backbone            -> UNet engine (x0 prediction, float32 [B, C, *S] out)
  * dynamic thresholding -> rho_abs_quantile: exact per-sample 0.9-quantile of |x0| (radix select), no sort, no host sync
  * DDIM update          -> rho_ddim_step (clamp / rescale, eps re-derivation, x_{t-1}) in the reference's operation order
  * q_sample             -> rho_q_sample_coef;  noise -> rho_philox_normal
The per-step scalars (four table entries) are kernel arguments computed on the host from the float64 tables exactly as
``_extract_into_tensor`` + the float32 tensor expressions of ``ddim_sample`` do; the loop never synchronises.

``training_step`` (:1153-1210) reproduces the reference's objective as written: the data are noised twice with the same
noise (:1186 then :877) and the backbone output is regressed on the once-noised data.

The rest of the reference class's public API (guided-diffusion's) is built on csrc/gaussian.hip, for the mean types START_X /
EPSILON and every variance type: the distribution helpers (:277-510), ancestral sampling (:512-652), the DDIM loop with eta and
``cond_fn`` (:654-702, :742-824), DDIM inversion (:704-740), the variational bound in bits per dimension (:826-859, :936-1009)
and ``training_losses`` (:861-934).  Every kernel gathers per-sample rows of one packed float32 table (``_tab``) at a device
``t[B]``; the loops never synchronise with the host and poll the error flag once at the end.

Fixed and learned variances take one path.  ``_x0_source`` hands a step its x0 source and, for LEARNED / LEARNED_RANGE (2C-channel
backbone, :368-383), the variance half of the model output; both halves are views that the kernels read in place.  The ops.gd_*
wrappers launch the learned-variance instantiation of a kernel when they are given variance values and the fixed one (variance from
the table) otherwise.  With a learned variance training_losses returns the hybrid loss mse + vb (:893-930).
"""
from __future__ import annotations

import enum
import math
from typing import Any, Mapping, Union

import numpy as np
import torch
from torch import Tensor

from .. import hip
from .. import metrics  # noqa: F401  (rho_diffusion.metrics.losses resolves under install_alias, as the reference imports it here)
from ..engine import ops
from ..utils import sample_from_discrete_parameter_space, save_model_checkpoint
from .abstract_diffusion import AbstractDiffusionPipeline

__all__ = ["GaussianDiffusionPipeline", "get_named_beta_schedule", "betas_for_alpha_bar", "diffusion_tables", "ddim_coefficients",
           "ModelMeanType", "ModelVarType", "LossType"]


class ModelMeanType(enum.Enum):
    """Which type of output the model predicts (:107-113)."""
    PREVIOUS_X = enum.auto()  # the model predicts x_{t-1}
    START_X = enum.auto()  # the model predicts x_0
    EPSILON = enum.auto()  # the model predicts epsilon


class ModelVarType(enum.Enum):
    """What is used as the model's output variance (:116-127)."""
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    """:130-141."""
    MSE = enum.auto()  # use raw MSE loss (and KL when learning variances)
    RESCALED_MSE = enum.auto()  # use raw MSE loss (with RESCALED_KL when learning variances)
    KL = enum.auto()  # use the variational lower-bound
    RESCALED_KL = enum.auto()  # like KL, but rescale to estimate the full VLB

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


def model_variance_tables(tables: Mapping[str, np.ndarray], var_type: ModelVarType):
    """float64 (variance, log_variance) of a fixed variance type (:385-398); a learned variance has no per-t table."""
    if var_type == ModelVarType.FIXED_LARGE:
        v = np.append(tables["posterior_variance"][1], tables["betas"][1:])
        return v, np.log(v)
    if var_type == ModelVarType.FIXED_SMALL:
        return tables["posterior_variance"], tables["posterior_log_variance_clipped"]
    raise NotImplementedError(f"model_var_type {var_type}: learned variances (gaussian_diffusion.py:368-383) take their value from the "
                              "2C-channel model output and have no per-t table; this is a table of FIXED_LARGE or FIXED_SMALL")


def gd_table_rows(tables: Mapping[str, np.ndarray], var_type: ModelVarType) -> np.ndarray:
    """The packed float32 [RHO_GD_ROWS, T] table of csrc/gaussian.hip (row order ops.GD_ROWS): each float64 table cast to float32
    as ``_extract_into_tensor`` (:91-105) casts it."""
    var, logvar = model_variance_tables(tables, var_type)
    ac = tables["alphas_cumprod"]
    rows = {"sqrt_recip": tables["sqrt_recip_alphas_cumprod"], "sqrt_recipm1": tables["sqrt_recipm1_alphas_cumprod"],
            "coef1": tables["posterior_mean_coef1"], "coef2": tables["posterior_mean_coef2"], "model_var": var, "model_logvar": logvar,
            "post_logvar": tables["posterior_log_variance_clipped"], "abar": ac, "abar_prev": tables["alphas_cumprod_prev"],
            "abar_next": tables["alphas_cumprod_next"], "sqrt_abar": tables["sqrt_alphas_cumprod"],
            "log_1m_abar": tables["log_one_minus_alphas_cumprod"], "1m_abar": 1.0 - ac, "post_var": tables["posterior_variance"],
            "log_beta": np.log(tables["betas"])}
    return np.stack([np.asarray(rows[k], dtype=np.float64).astype(np.float32) for k in ops.GD_ROWS])


def gd_table_rows_learned(tables: Mapping[str, np.ndarray]) -> np.ndarray:
    """The packed table of the learned variances (:368-383): their rows are post_logvar (min_log) and log_beta (max_log); the
    model_var / model_logvar rows are FIXED_LARGE's and unused there (a learned variance has no per-t table)."""
    return gd_table_rows(tables, ModelVarType.FIXED_LARGE)


def betas_for_alpha_bar(num_diffusion_timesteps: int, alpha_bar, max_beta: float = 0.999) -> np.ndarray:
    """gaussian_diffusion.py:72-89."""
    betas = []
    for i in range(num_diffusion_timesteps):
        t1 = i / num_diffusion_timesteps
        t2 = (i + 1) / num_diffusion_timesteps
        betas.append(min(1 - alpha_bar(t2) / alpha_bar(t1), max_beta))
    return np.array(betas)


def get_named_beta_schedule(schedule_name: str, num_diffusion_timesteps: int) -> np.ndarray:
    """gaussian_diffusion.py:45-69."""
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps, lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def diffusion_tables(betas: np.ndarray) -> dict:
    """The float64 coefficient tables of GaussianDiffusionPipeline.__init__ (gaussian_diffusion.py:237-273)."""
    betas = np.array(betas, dtype=np.float64)
    assert len(betas.shape) == 1, "betas must be 1-D"
    assert (betas > 0).all() and (betas <= 1).all()
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    pv = betas * (1.0 - ac_prev) / (1.0 - ac)
    return {
        "betas": betas, "alphas_cumprod": ac, "alphas_cumprod_prev": ac_prev, "alphas_cumprod_next": np.append(ac[1:], 0.0),
        "sqrt_alphas_cumprod": np.sqrt(ac), "sqrt_one_minus_alphas_cumprod": np.sqrt(1.0 - ac),
        "log_one_minus_alphas_cumprod": np.log(1.0 - ac), "sqrt_recip_alphas_cumprod": np.sqrt(1.0 / ac),
        "sqrt_recipm1_alphas_cumprod": np.sqrt(1.0 / ac - 1), "posterior_variance": pv,
        "posterior_log_variance_clipped": np.log(np.append(pv[1], pv[1:])),
        "posterior_mean_coef1": betas * np.sqrt(ac_prev) / (1.0 - ac),
        "posterior_mean_coef2": (1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac),
    }


def ddim_coefficients(tables: Mapping[str, np.ndarray], t: int, eta: float = 0.0):
    """The float32 scalars of ddim_sample (:675-697) for a batch-uniform timestep: tables gathered in float64, cast to
    float32 (``_extract_into_tensor``), then combined with float32 arithmetic like the reference's tensor expressions.
    Returns (c_recip, c_recipm1, sqrt_abar_prev, coef_eps, sigma_masked) for rho_ddim_step."""
    f = np.float32
    c_recip, c_recipm1 = f(tables["sqrt_recip_alphas_cumprod"][t]), f(tables["sqrt_recipm1_alphas_cumprod"][t])
    ab, abp = f(tables["alphas_cumprod"][t]), f(tables["alphas_cumprod_prev"][t])
    one = f(1.0)
    sigma = f(eta) * np.sqrt((one - abp) / (one - ab), dtype=f) * np.sqrt(one - ab / abp, dtype=f)
    coef_eps = np.sqrt(one - abp - sigma * sigma, dtype=f)
    mask = f(1.0 if t != 0 else 0.0)
    return float(c_recip), float(c_recipm1), float(np.sqrt(abp, dtype=f)), float(coef_eps), float(mask * sigma)


class GaussianDiffusionPipeline(AbstractDiffusionPipeline):
    def __init__(self, backbone, backbone_kwargs: dict, schedule, loss_func, timesteps: Union[int, Tensor] = 1000,
                 cond_fn: str = None, cond_fn_kwargs: dict = None, optimizer=None,
                 opt_kwargs: Union[Mapping[str, Any], None] = {}, t_checkpoints=None, sampling_batch_size=10,
                 sample_every_n_epochs=5, sample_parameter_space=None, save_checkpoint_every_n_epochs=10):
        super().__init__(backbone=backbone, backbone_kwargs=backbone_kwargs, schedule=schedule, timesteps=timesteps,
                         cond_fn=cond_fn, cond_fn_kwargs=cond_fn_kwargs, optimizer=optimizer, opt_kwargs=opt_kwargs)
        self._init_loss_and_noise(loss_func)
        self.t_checkpoints = t_checkpoints
        self.sampling_batch_size = sampling_batch_size
        self.sample_every_n_epochs = sample_every_n_epochs
        self.sample_parameter_space = sample_parameter_space
        self.save_weights_every_n_epochs = save_checkpoint_every_n_epochs
        self.rescale_timesteps = False
        # the reference's fixed configuration (:199-233); users may set other supported values afterwards
        self.loss_type = LossType.MSE
        self.model_mean_type = ModelMeanType.START_X
        self.model_var_type = ModelVarType.FIXED_LARGE

        # float64 tables (:237-273)
        self.tables = diffusion_tables(get_named_beta_schedule("cosine", int(timesteps)))
        for k_, v_ in self.tables.items():
            setattr(self, k_, v_)
        self.timesteps = int(self.betas.shape[0])
        self.dynamic_thresholding_percentile = 0.9

        self._dev_tables = {}
        self._quant_ws = None
        self._gd_tables = {}
        self._gd_err = None
        self._gd_ws = None

    # ------------------------------------------------------------------ q_sample (noise, :1011-1012, is the base class's Philox draw)
    def _table(self, name: str, device) -> Tensor:
        key = (name, str(device))
        if key not in self._dev_tables:
            self._dev_tables[key] = torch.from_numpy(getattr(self, name)).float().to(device).contiguous()
        return self._dev_tables[key]

    def q_sample(self, x_start: Tensor, t: Tensor, noise: Tensor = None) -> Tensor:
        """:294-312."""
        hip.require_gpu(x_start, "x_start")
        x0 = x_start.float().contiguous()
        if noise is None:
            noise = self.noise(x0)
        assert noise.shape == x_start.shape
        t = t.reshape(-1).to(device=x0.device, dtype=torch.int64).contiguous()
        return ops.q_sample_coef(x0, noise.float().contiguous(), t, self._table("sqrt_alphas_cumprod", x0.device),
                                 self._table("sqrt_one_minus_alphas_cumprod", x0.device))

    def forward_process(self, data: Tensor, t: Union[Tensor, None] = None) -> list:
        """:1014-1027: returns [x_t, noise]."""
        hip.require_gpu(data, "data")
        self.schedule.dtype = data.dtype
        if t is None:
            t = self.random_timesteps(data.size(0))
        noise = self.noise(data)
        return [self.q_sample(x_start=data, t=t, noise=noise), noise]

    # ------------------------------------------------------------------ DDIM coefficients of one step
    def ddim_coefficients(self, t: int, eta: float = 0.0):
        return ddim_coefficients(self.tables, t, eta)

    # ------------------------------------------------------------------ sampling
    @torch.no_grad()
    def reverse_process(self, x_T: Tensor, conditions=None, t_checkpoints=None, eta: float = 0.0) -> dict:
        """:1029-1099.  ``x_T`` is a shape/device template (:1039 starts from randn_like(x_T))."""
        hip.require_gpu(x_T, "x_T")
        dev = x_T.device
        batch_size = x_T.size(0)
        denoise_steps = len(self.betas)
        x_t = self.noise(x_T).contiguous()
        if t_checkpoints is not None:
            num_checkpoints = len(t_checkpoints)
            buf = torch.zeros((batch_size, num_checkpoints) + tuple(x_T.shape[1:]), dtype=torch.float32, device=dev)
            steps_per_ckpt = denoise_steps // num_checkpoints
        else:
            num_checkpoints, buf, steps_per_ckpt = 0, None, denoise_steps
        cc = self._preembed_conditions(self._resolve_conditions(conditions, batch_size, dev))

        engine = self.backbone.engine() if hasattr(self.backbone, "engine") else None
        learned, C = self._learned(), x_T.shape[1]
        t_dev = torch.full((1,), denoise_steps - 1, dtype=torch.int32, device=dev)
        quant = torch.empty(batch_size, dtype=torch.float32, device=dev)
        t_idx = 0
        for t in range(denoise_steps - 1, -1, -1):
            if engine is not None:
                x0_hat = engine.forward(x_t, None, cc, t_scalar_dev=t_dev)
            else:
                x0_hat = self.backbone(x_t, torch.full((batch_size,), t, device=dev, dtype=torch.long), cc)
            if learned:                   # rho_abs_quantile / rho_ddim_step read C channels: the mean half, one copy per step
                x0_hat = x0_hat[:, :C]
            x0_hat = x0_hat.contiguous()
            c_recip, c_recipm1, sqrt_abp, coef_eps, sig = self.ddim_coefficients(t, eta)
            z = self.noise(x_t) if sig != 0.0 else None          # the reference draws it always; with eta = 0 it is multiplied by 0
            self._quantile(x0_hat, out=quant)
            ops.ddim_step(x_t, x0_hat, quant, z, x_t, None, c_recip, c_recipm1, sqrt_abp, coef_eps, sig)
            if buf is not None and t % steps_per_ckpt == 0 and t_idx < num_checkpoints:
                buf[:, t_idx].copy_(x_t)
                t_idx += 1
            ops.step_advance(t_dev, None, 0)
        self._check_backbone_errors()
        return {"buffer": buf, "denoised": x_t}

    # ------------------------------------------------------------------ guided-diffusion API (csrc/gaussian.hip)
    def _mean_code(self) -> int:
        if self.model_mean_type == ModelMeanType.START_X:
            return ops.GD_START_X
        if self.model_mean_type == ModelMeanType.EPSILON:
            return ops.GD_EPSILON
        if self.model_mean_type == ModelMeanType.PREVIOUS_X:
            raise NotImplementedError("model_mean_type PREVIOUS_X (gaussian_diffusion.py:417-422, _predict_xstart_from_xprev :452-460) "
                                      "is not built; use START_X or EPSILON")
        raise NotImplementedError(self.model_mean_type)

    def _var_code(self):
        """var_type of the ops.gd_* calls: None for a fixed variance (that one is in the table)."""
        return {ModelVarType.LEARNED: ops.GD_LEARNED, ModelVarType.LEARNED_RANGE: ops.GD_LEARNED_RANGE}.get(self.model_var_type)

    def _learned(self) -> bool:
        return self._var_code() is not None

    def _tab(self, device) -> Tensor:
        """The packed float32 [RHO_GD_ROWS, T] table every gd kernel of the current ``model_var_type`` reads, on ``device``.  A learned
        variance reads its post_logvar (min_log) and log_beta (max_log) rows."""
        key = (str(device), self.model_var_type)
        if key not in self._gd_tables:
            rows = gd_table_rows_learned(self.tables) if self._learned() else gd_table_rows(self.tables, self.model_var_type)
            self._gd_tables[key] = torch.from_numpy(rows).to(device).contiguous()
        return self._gd_tables[key]

    def _gd_table(self, device) -> Tensor:
        """``_tab`` for a fixed ``model_var_type``, whose model_var / model_logvar rows are the model's; a learned type is refused."""
        model_variance_tables(self.tables, self.model_var_type)
        return self._tab(device)

    def _gd_flag(self, device) -> Tensor:
        if self._gd_err is None or self._gd_err.device != torch.device(device):
            self._gd_err = torch.zeros(1, dtype=torch.int32, device=device)
        return self._gd_err

    def _check_backbone_errors(self) -> None:
        """The backbone's flag, then the timestep flag of the table gathers (bit 4): a t outside [0, T) raises IndexError like the
        reference's table lookup (:91-105).  Polled only where the pipeline synchronises anyway."""
        super()._check_backbone_errors()
        if self._gd_err is not None:
            v = int(self._gd_err.item())
            if v & 4:
                self._gd_err.zero_()
                raise IndexError(f"GaussianDiffusionPipeline: a timestep is outside [0, {self.timesteps}) (gaussian_diffusion.py:91-105)")

    def _gd_view(self, tab: Tensor, row: str, t: Tensor, shape) -> Tensor:
        """``_extract_into_tensor`` (:91-105): the table row gathered at t, as an expanded [B, 1, ...] view.  An out-of-range t reads
        the clamped row here too; the kernels of the same call flag it (IndexError at the next poll)."""
        t = t.clamp(0, tab.shape[1] - 1)
        return tab[ops.GD_ROW[row]][t].view(-1, *([1] * (len(shape) - 1))).expand(shape)

    @staticmethod
    def _gd_x(x: Tensor, name: str) -> Tensor:
        hip.require_gpu(x, name)
        return x.float().contiguous()

    @staticmethod
    def _gd_t(t, batch: int, device) -> Tensor:
        if not torch.is_tensor(t):
            t = torch.tensor(t)
        t = t.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
        assert t.shape == (batch,), f"t must have shape ({batch},), got {tuple(t.shape)}"
        return t

    def _gd_model_kwargs(self, model_kwargs) -> dict:
        kw = dict(model_kwargs or {})
        if kw.get("y") is not None:
            kw["y"] = self._preembed_conditions(kw["y"])
        return kw

    def _gd_model(self, model, x: Tensor, t: Tensor, kw: dict, t_dev: Tensor = None) -> Tensor:
        """model(x, t, **model_kwargs) as a contiguous float32 tensor of x's shape.  The backbone inside a loop (batch-uniform t)
        runs on the engine with the device-resident timestep ``t_dev``, as reverse_process does."""
        if t_dev is not None and model is self.backbone and hasattr(model, "engine") and set(kw) <= {"y"}:
            out = model.engine().forward(x, None, kw.get("y"), t_scalar_dev=t_dev)
        else:
            out = model(x, self._scale_timesteps(t), **kw)
        self._check_output(out, x)
        hip.require_gpu(out, "model output")
        return out.float().contiguous()

    def _check_output(self, out: Tensor, x: Tensor) -> None:
        if self._learned():
            want = (x.shape[0], 2 * x.shape[1], *x.shape[2:])
            if tuple(out.shape) != want:                           # the reference asserts it (:369)
                raise AssertionError(f"model output {tuple(out.shape)}: model_var_type {self.model_var_type.name} needs the 2C-channel "
                                     f"output {want} (gaussian_diffusion.py:368-383)")
        elif tuple(out.shape) != tuple(x.shape):
            raise NotImplementedError(f"model output {tuple(out.shape)} for x {tuple(x.shape)}: a 2C-channel output needs a learned "
                                      f"model_var_type (gaussian_diffusion.py:368-383), not {self.model_var_type.name}")

    def _scale_timesteps(self, t):
        """:468-471."""
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.timesteps)
        return t

    def _quantile(self, x: Tensor, out: Tensor = None) -> Tensor:
        """The per-sample dynamic-thresholding quantile of |x| (x any per-sample view), on the pipeline's workspace."""
        self._quant_ws = ops.quantile_workspace(x.shape[0], x.device, self._quant_ws)
        return ops.abs_quantile(x, self.dynamic_thresholding_percentile, out=out, workspace=self._quant_ws)

    def _x0_source(self, x: Tensor, mo: Tensor, t: Tensor, tab: Tensor, clip_denoised: bool, denoised_fn):
        """(source, variance values or None, mean code, quantile) for the step kernels: ``process_xstart`` (:400-415).  With a learned
        variance the two halves of the [B, 2C, ...] output are views read in place.  The model output goes to the kernel as it is
        unless x0 must exist before the quantile or ``denoised_fn`` (EPSILON with thresholding, any denoised_fn): then x0 is
        materialised first and handed over as a START_X output."""
        C = x.shape[1]
        src, var = (mo[:, :C], mo[:, C:]) if self._learned() else (mo, None)
        code = self._mean_code()
        if denoised_fn is not None or (clip_denoised and code == ops.GD_EPSILON):
            if code == ops.GD_EPSILON and var is None:
                src = ops.gd_affine(x, src, t, tab, "sqrt_recip", "sqrt_recipm1", "ax-by", err_flag=self._gd_flag(x.device))
            elif code == ops.GD_EPSILON:     # gd_affine takes contiguous operands: the posterior kernel reads the half in place, same x0
                x0 = torch.empty_like(x)
                ops.gd_posterior_step(x, src, t, tab, code, None, None, None, None, x0, err_flag=self._gd_flag(x.device), var_values=var,
                                      var_type=self._var_code())
                src = x0
            if denoised_fn is not None:
                src = self._gd_x(denoised_fn(src), "denoised_fn output")
            code = ops.GD_START_X
        return src, var, code, (self._quantile(src) if clip_denoised else None)

    def _cond_grad(self, cond_fn, x: Tensor, t: Tensor, model_kwargs) -> Tensor:
        g = cond_fn(x, self._scale_timesteps(t), **(model_kwargs or {}))
        return self._gd_x(g, "cond_fn output")

    # ---- distribution helpers
    def q_mean_variance(self, x_start: Tensor, t: Tensor):
        """:277-292: (mean, variance, log_variance) of q(x_t | x_0)."""
        x = self._gd_x(x_start, "x_start")
        t = self._gd_t(t, x.shape[0], x.device)
        tab = self._tab(x.device)
        mean = ops.gd_affine(x, None, t, tab, "sqrt_abar", None, "ax", err_flag=self._gd_flag(x.device))
        return mean, self._gd_view(tab, "1m_abar", t, x.shape), self._gd_view(tab, "log_1m_abar", t, x.shape)

    def q_posterior_mean_variance(self, x_start: Tensor, x_t: Tensor, t: Tensor):
        """:314-336: (mean, variance, log_variance_clipped) of q(x_{t-1} | x_t, x_0)."""
        assert x_start.shape == x_t.shape
        xs, xt = self._gd_x(x_start, "x_start"), self._gd_x(x_t, "x_t")
        t = self._gd_t(t, xs.shape[0], xs.device)
        tab = self._tab(xs.device)
        mean = ops.gd_affine(xs, xt, t, tab, "coef1", "coef2", "ax+by", err_flag=self._gd_flag(xs.device))
        return mean, self._gd_view(tab, "post_var", t, xs.shape), self._gd_view(tab, "post_logvar", t, xs.shape)

    def _predict_xstart_from_eps(self, x_t: Tensor, t: Tensor, eps: Tensor) -> Tensor:
        """:445-450."""
        assert x_t.shape == eps.shape
        x = self._gd_x(x_t, "x_t")
        t = self._gd_t(t, x.shape[0], x.device)
        return ops.gd_affine(x, self._gd_x(eps, "eps"), t, self._tab(x.device), "sqrt_recip", "sqrt_recipm1", "ax-by",
                             err_flag=self._gd_flag(x.device))

    def _predict_eps_from_xstart(self, x_t: Tensor, t: Tensor, pred_xstart: Tensor) -> Tensor:
        """:462-466."""
        x = self._gd_x(x_t, "x_t")
        t = self._gd_t(t, x.shape[0], x.device)
        return ops.gd_affine(x, self._gd_x(pred_xstart, "pred_xstart"), t, self._tab(x.device), "sqrt_recip", "sqrt_recipm1",
                             "(ax-y)/b", err_flag=self._gd_flag(x.device))

    def p_mean_variance(self, model, x: Tensor, t: Tensor, clip_denoised: bool = True, denoised_fn=None, model_kwargs=None) -> dict:
        """:338-443 (START_X / EPSILON, FIXED_LARGE / FIXED_SMALL).  ``clip_denoised`` is the reference's dynamic thresholding
        (per-sample 0.9-quantile of |x0|, s = max(q, 1), clamp and divide), applied after ``denoised_fn``."""
        x = self._gd_x(x, "x")
        B = x.shape[0]
        t = self._gd_t(t, B, x.device)
        tab = self._tab(x.device)
        mo = self._gd_model(model, x, t, self._gd_model_kwargs(model_kwargs))
        src, var, code, q = self._x0_source(x, mo, t, tab, clip_denoised, denoised_fn)
        mean, px = torch.empty_like(x), torch.empty_like(x)
        v, lv = (None, None) if var is None else (torch.empty_like(x), torch.empty_like(x))      # learned: per element, from the kernel
        ops.gd_posterior_step(x, src, t, tab, code, q, None, None, mean, px, err_flag=self._gd_flag(x.device), var_values=var,
                              var_type=self._var_code(), variance=v, log_variance=lv)
        if var is None:                                                                           # fixed: expanded views of the table rows
            v, lv = self._gd_view(tab, "model_var", t, x.shape), self._gd_view(tab, "model_logvar", t, x.shape)
        return {"mean": mean, "variance": v, "log_variance": lv, "pred_xstart": px}

    def condition_mean(self, cond_fn, p_mean_var: dict, x: Tensor, t: Tensor, model_kwargs=None) -> Tensor:
        """:473-486: mean + variance * cond_fn(x, t).  The mean is re-derived from ``p_mean_var["pred_xstart"]`` in the same pass
        (bit-equal to the "mean" p_mean_variance returns for it)."""
        x = self._gd_x(x, "x")
        t = self._gd_t(t, x.shape[0], x.device)
        tab = self._tab(x.device)
        g = self._cond_grad(cond_fn, x, t, model_kwargs)
        out = torch.empty_like(x)
        # a learned variance per element: exp of p_mean_var's log_variance (bit-equal to its "variance"), handed over as LEARNED values
        var = self._gd_x(p_mean_var["log_variance"], "log_variance") if self._learned() else None
        ops.gd_posterior_step(x, self._gd_x(p_mean_var["pred_xstart"], "pred_xstart"), t, tab, ops.GD_START_X, None, g, None, out, None,
                              err_flag=self._gd_flag(x.device), var_values=var, var_type=None if var is None else ops.GD_LEARNED)
        return out

    def condition_score(self, cond_fn, p_mean_var: dict, x: Tensor, t: Tensor, model_kwargs=None) -> dict:
        """:488-510: eps = eps(pred_xstart) - sqrt(1 - abar) * cond_fn(x, t); pred_xstart and mean re-derived from it."""
        x = self._gd_x(x, "x")
        t = self._gd_t(t, x.shape[0], x.device)
        tab = self._tab(x.device)
        g = self._cond_grad(cond_fn, x, t, model_kwargs)
        px, scratch = torch.empty_like(x), torch.empty_like(x)
        flag = self._gd_flag(x.device)
        ops.gd_ddim_step(x, self._gd_x(p_mean_var["pred_xstart"], "pred_xstart"), t, tab, ops.GD_START_X, None, g, None, 0.0, False,
                         scratch, px, err_flag=flag)
        out = dict(p_mean_var)
        out["pred_xstart"] = px
        out["mean"] = ops.gd_affine(px, x, t, tab, "coef1", "coef2", "ax+by", out=scratch, err_flag=flag)
        return out

    # ---- ancestral sampling
    def _p_step(self, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, kw, sample, px, t_dev=None) -> dict:
        tab = self._tab(x.device)
        mo = self._gd_model(model, x, t, kw, t_dev)
        src, var, code, q = self._x0_source(x, mo, t, tab, clip_denoised, denoised_fn)
        noise = self.noise(x)                                                  # :545, drawn before cond_fn runs
        g = self._cond_grad(cond_fn, x, t, model_kwargs) if cond_fn is not None else None
        ops.gd_posterior_step(x, src, t, tab, code, q, g, noise, sample, px, err_flag=self._gd_flag(x.device), var_values=var,
                              var_type=self._var_code())
        return {"sample": sample, "pred_xstart": px}

    @torch.no_grad()
    def p_sample(self, model, x: Tensor, t: Tensor, clip_denoised: bool = True, denoised_fn=None, cond_fn=None, model_kwargs=None) -> dict:
        """:512-556: one ancestral step x_t -> x_{t-1} (no noise where t == 0)."""
        x = self._gd_x(x, "x")
        t = self._gd_t(t, x.shape[0], x.device)
        return self._p_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, self._gd_model_kwargs(model_kwargs),
                            torch.empty_like(x), torch.empty_like(x))

    def _loop_device(self, model, device):
        if device is not None:
            return torch.device(device)
        params = model.parameters() if hasattr(model, "parameters") else self.backbone.parameters()
        return next(params).device

    def _loop(self, step, model, shape, noise, device, progress, fresh: bool):
        """Shared body of the sampling loops: start from ``noise`` or ``self.noise`` (:620-623), run t = T-1 .. 0 on device-resident
        timesteps, no host synchronisation; one error poll after the last step."""
        assert isinstance(shape, (tuple, list))
        dev = self._loop_device(model, device)
        if noise is not None:
            img = self._gd_x(noise, "noise")
        else:
            img = self.noise(torch.empty(tuple(shape), dtype=torch.float32, device=dev))
        T = self.timesteps
        ts = torch.arange(T - 1, -1, -1, dtype=torch.int64, device=dev).view(T, 1).expand(T, img.shape[0]).contiguous()
        t_dev = torch.full((1,), T - 1, dtype=torch.int32, device=dev)
        bufs = None if fresh else (torch.empty_like(img), torch.empty_like(img), torch.empty_like(img))
        indices = range(T)
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        for j in indices:
            if fresh:
                sample, px = torch.empty_like(img), torch.empty_like(img)
            else:
                sample, px = bufs[j % 2], bufs[2]
            out = step(img, ts[j], sample, px, t_dev)
            ops.step_advance(t_dev, None, 0)
            yield out
            img = out["sample"]
        self._check_backbone_errors()

    @torch.no_grad()
    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None, device=None,
                      progress=False) -> Tensor:
        """:558-602."""
        final = None
        for final in self._p_loop(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, fresh=False):
            pass
        return final["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                                  device=None, progress=False):
        """:604-652: yields p_sample's dict at every timestep (fresh tensors)."""
        yield from self._p_loop(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, fresh=True)

    def _p_loop(self, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, fresh):
        kw = self._gd_model_kwargs(model_kwargs)

        def step(x, t, sample, px, t_dev):
            return self._p_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, kw, sample, px, t_dev)
        with torch.no_grad():
            yield from self._loop(step, model, shape, noise, device, progress, fresh)

    # ---- DDIM
    def _ddim_step(self, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, kw, eta, reverse, sample, px, t_dev=None) -> dict:
        tab = self._tab(x.device)
        mo = self._gd_model(model, x, t, kw, t_dev)
        src, _, code, q = self._x0_source(x, mo, t, tab, clip_denoised, denoised_fn)     # a learned variance is ignored, as in the reference
        g = self._cond_grad(cond_fn, x, t, model_kwargs) if cond_fn is not None else None
        # :685: the reference draws the noise at every step; with eta = 0 it is multiplied by 0 and no used draw follows it
        noise = self.noise(x) if (not reverse and eta != 0.0) else None
        ops.gd_ddim_step(x, src, t, tab, code, q, g, noise, eta, reverse, sample, px, err_flag=self._gd_flag(x.device))
        return {"sample": sample, "pred_xstart": px}

    @torch.no_grad()
    def ddim_sample(self, model, x: Tensor, t: Tensor, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                    eta=0.0) -> dict:
        """:654-702: one DDIM step with ``eta`` (sigma :687-691); ``cond_fn`` through condition_score."""
        x = self._gd_x(x, "x")
        t = self._gd_t(t, x.shape[0], x.device)
        return self._ddim_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, self._gd_model_kwargs(model_kwargs),
                               float(eta), False, torch.empty_like(x), torch.empty_like(x))

    @torch.no_grad()
    def ddim_reverse_sample(self, model, x: Tensor, t: Tensor, clip_denoised=True, denoised_fn=None, model_kwargs=None, eta=0.0) -> dict:
        """:704-740: x_t -> x_{t+1} along the deterministic DDIM path (alphas_cumprod_next)."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        x = self._gd_x(x, "x")
        t = self._gd_t(t, x.shape[0], x.device)
        return self._ddim_step(model, x, t, clip_denoised, denoised_fn, None, model_kwargs, self._gd_model_kwargs(model_kwargs), 0.0, True,
                               torch.empty_like(x), torch.empty_like(x))

    @torch.no_grad()
    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                         device=None, progress=False, eta=0.0) -> Tensor:
        """:742-775."""
        final = None
        for final in self._ddim_loop(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, eta,
                                     fresh=False):
            pass
        return final["sample"]

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0):
        """:777-824: yields ddim_sample's dict at every timestep (fresh tensors)."""
        yield from self._ddim_loop(model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, eta, fresh=True)

    def _ddim_loop(self, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, eta, fresh):
        kw = self._gd_model_kwargs(model_kwargs)

        def step(x, t, sample, px, t_dev):
            return self._ddim_step(model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, kw, float(eta), False, sample, px, t_dev)
        with torch.no_grad():
            yield from self._loop(step, model, shape, noise, device, progress, fresh)

    # ---- variational bound
    def _vb_step(self, model, x_start, x_t, t, clip_denoised, kw, vb, xstart_mse=None, mse=None, noise=None, raw_kl=None, raw_nll=None,
                 px=None, t_dev=None):
        tab = self._tab(x_start.device)
        mo = self._gd_model(model, x_t, t, kw, t_dev)
        self._gd_ws = ops.gd_workspace(x_start.shape[0], x_start.numel() // x_start.shape[0], x_start.device, self._gd_ws)
        src, var, code, q = self._x0_source(x_t, mo, t, tab, clip_denoised, None)
        ops.gd_vlb_terms(x_start, x_t, src, t, tab, code, q, noise, vb, xstart_mse, mse, raw_kl, raw_nll, px, workspace=self._gd_ws,
                         err_flag=self._gd_flag(x_start.device), var_values=var, var_type=self._var_code())

    @torch.no_grad()
    def _vb_terms_bpd(self, model, x_start: Tensor, x_t: Tensor, t: Tensor, clip_denoised=True, model_kwargs=None) -> dict:
        """:826-859: {"output": [N] decoder NLL (t == 0) or KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) in bits, "pred_xstart"}."""
        xs, xt = self._gd_x(x_start, "x_start"), self._gd_x(x_t, "x_t")
        t = self._gd_t(t, xs.shape[0], xs.device)
        out = torch.empty(xs.shape[0], dtype=torch.float32, device=xs.device)
        px = torch.empty_like(xs)
        self._vb_step(model, xs, xt, t, clip_denoised, self._gd_model_kwargs(model_kwargs), out, px=px)
        return {"output": out, "pred_xstart": px}

    def _vb_terms_raw(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None):
        """Both terms of _vb_terms_bpd, [N] each in bits: (kl, decoder_nll) - what the reference's ``where`` selects from."""
        xs, xt = self._gd_x(x_start, "x_start"), self._gd_x(x_t, "x_t")
        t = self._gd_t(t, xs.shape[0], xs.device)
        B = xs.shape[0]
        vb, kl, nll = (torch.empty(B, dtype=torch.float32, device=xs.device) for _ in range(3))
        with torch.no_grad():
            self._vb_step(model, xs, xt, t, clip_denoised, self._gd_model_kwargs(model_kwargs), vb, raw_kl=kl, raw_nll=nll)
        return kl, nll

    @torch.no_grad()
    def _prior_bpd(self, x_start: Tensor) -> Tensor:
        """:936-951: KL(q(x_{T-1} | x_0) || N(0, 1)) per sample, in bits."""
        xs = self._gd_x(x_start, "x_start")
        out = torch.empty(xs.shape[0], dtype=torch.float32, device=xs.device)
        self._gd_ws = ops.gd_workspace(xs.shape[0], xs.numel() // xs.shape[0], xs.device, self._gd_ws)
        ops.gd_vlb_terms(xs, None, None, None, self._tab(xs.device), ops.GD_START_X, None, None, out, prior=True, workspace=self._gd_ws)
        return out

    @torch.no_grad()
    def calc_bpd_loop(self, model, x_start: Tensor, clip_denoised=True, model_kwargs=None) -> dict:
        """:953-1009: the whole variational bound in bits per dimension.  Column j of vb / xstart_mse / mse holds timestep T-1-j,
        written on the device by the fused kernel; one noise draw per timestep; no host synchronisation until the error poll."""
        xs = self._gd_x(x_start, "x_start")
        dev, B, T = xs.device, xs.shape[0], self.timesteps
        kw = self._gd_model_kwargs(model_kwargs)
        vb, xstart_mse, mse = (torch.empty((B, T), dtype=torch.float32, device=dev) for _ in range(3))
        ts = torch.arange(T - 1, -1, -1, dtype=torch.int64, device=dev).view(T, 1).expand(T, B).contiguous()
        t_dev = torch.full((1,), T - 1, dtype=torch.int32, device=dev)
        x_t = torch.empty_like(xs)
        ca, cb = self._table("sqrt_alphas_cumprod", dev), self._table("sqrt_one_minus_alphas_cumprod", dev)
        flag = self._gd_flag(dev)
        for j in range(T):
            noise = self.noise(xs)
            ops.q_sample_coef(xs, noise.float().contiguous(), ts[j], ca, cb, out=x_t, err_flag=flag)
            self._vb_step(model, xs, x_t, ts[j], clip_denoised, kw, vb[:, j], xstart_mse[:, j], mse[:, j], noise=noise.float().contiguous(),
                          t_dev=t_dev)
            ops.step_advance(t_dev, None, 0)
        prior_bpd = self._prior_bpd(xs)
        total_bpd = vb.sum(dim=1) + prior_bpd
        self._check_backbone_errors()
        return {"total_bpd": total_bpd, "prior_bpd": prior_bpd, "vb": vb, "xstart_mse": xstart_mse, "mse": mse}

    # ---- training loss
    def training_losses(self, model, x_start: Tensor, t: Tensor, model_kwargs={}, noise: Tensor = None) -> dict:
        """:861-934 for MSE / RESCALED_MSE (equal without a learned variance): {"loss", "mse"}, [N] each, differentiable through
        the backbone.  The target is x_start (START_X) or the noise (EPSILON).  With a learned variance (2C-channel output) also "vb"
        and loss = mse + vb: the hybrid objective, the VLB reaching only the variance half."""
        if self.loss_type.is_vb():
            raise NotImplementedError(f"loss_type {self.loss_type}: the variational-bound training loss (gaussian_diffusion.py:877-889) "
                                      "is not built; the pipeline's fixed configuration (:211-216) uses MSE")
        if self.loss_type not in (LossType.MSE, LossType.RESCALED_MSE):
            raise NotImplementedError(self.loss_type)
        learned = self._learned()
        if not learned:
            model_variance_tables(self.tables, self.model_var_type)
        code = self._mean_code()
        xs = self._gd_x(x_start, "x_start")
        t = self._gd_t(t, xs.shape[0], xs.device)
        if noise is None:
            noise = self.noise(xs)
        assert noise.shape == x_start.shape
        noise = self._gd_x(noise, "noise")
        x_t = self.q_sample(xs, t, noise=noise)
        out = model(x_t, self._scale_timesteps(t), **(model_kwargs or {}))
        self._check_output(out, xs)
        target = xs if code == ops.GD_START_X else noise
        if learned:
            # :893-930: mse on the mean half, vb = _vb_terms_bpd on (mean.detach(), variance), clip_denoised=False; one fused pass
            from ..autograd import hybrid_loss
            hip.require_gpu(out, "model output")
            scale = self.timesteps / 1000.0 if self.loss_type == LossType.RESCALED_MSE else None
            loss, mse, vb = hybrid_loss(out, xs, x_t, target, t, self._tab(xs.device), code, self._var_code(), scale, self._gd_flag(xs.device))
            return {"vb": vb, "mse": mse, "loss": loss}
        from ..autograd import mse_per_sample
        mse = mse_per_sample(out, target)
        return {"mse": mse, "loss": mse}

    # ------------------------------------------------------------------ wrappers
    def generate(self, parameter_space=None, random=False, save_figure_as=None):
        """:1102-1146: zero template of the last training batch shape, else ``[sampling_batch_size, out_channels] + data_shape``
        from the backbone kwargs; labels = rows of the discrete parameter space (``sample_parameter_space`` by default);
        reverse_process.  Returns what ``make_image_grid`` returns: the denoised samples (no figure is drawn)."""
        if hasattr(self, "data_shape"):
            shape = [int(x) for x in self.data_shape]
            shape[0] = self.sampling_batch_size
        else:
            # the reference takes out_channels (:1113), which is 2C with a learned variance: the samples have in_channels
            ch = self.backbone_kwargs["in_channels" if self._learned() else "out_channels"]
            shape = [self.sampling_batch_size, ch] + list(self.backbone_kwargs["data_shape"])
            self.data_dtype = torch.float32
        dev = next(self.backbone.parameters()).device
        if parameter_space is None:
            parameter_space = self.sample_parameter_space
        conditions = None
        if parameter_space is not None:
            conditions = sample_from_discrete_parameter_space(parameter_space, shape[0], random=random, device=dev)
        x_T = torch.zeros(shape, dtype=getattr(self, "data_dtype", torch.float32), device=dev)
        res = self.reverse_process(x_T, conditions=conditions, t_checkpoints=self.t_checkpoints)
        res["conditions"] = conditions
        self.last_samples = res
        return self.make_image_grid(res["denoised"], filename=save_figure_as)

    def save_model_weights(self):
        save_model_checkpoint(self.backbone, "model.pth")

    def training_step(self, batch, batch_idx: int = 0):
        """:1153-1210 with ``training_losses`` (:861-934) for the class's fixed configuration (MSE loss, x0 prediction,
        fixed variance): ``forward_process`` noises the data, ``training_losses`` noises that result AGAIN with the same
        noise (:877) and regresses the backbone output on the once-noised data (START_X target, :922);
        ``mean_flat(.).mean()`` over equally sized samples is the plain mean."""
        data, labels = self._parse_batch(batch)
        self.data_shape = data.shape
        self.data_dtype = data.dtype
        t = self.random_timesteps(data.size(0)).to(data.device)
        x_data, noise = self.forward_process(data, t)
        if self._learned():
            # learned variance: the reference as written (:1186-1197), training_losses on the noised data ["loss"].mean()
            self._tick_error_poll()
            kw = {"y": labels} if labels is not None else {}
            loss = self.training_losses(self.backbone, x_data, t, kw, noise)["loss"].mean()
            self.log("train_loss", loss, prog_bar=True)
            return loss
        x_t = self.q_sample(x_data, t, noise=noise)
        self._tick_error_poll()
        if labels is not None:
            out = self.backbone(x_t, t, labels)
        else:
            out = self.backbone(x_t, t)
        from ..autograd import mse_loss
        loss = mse_loss(out, x_data)
        self.log("train_loss", loss, prog_bar=True)
        return loss
