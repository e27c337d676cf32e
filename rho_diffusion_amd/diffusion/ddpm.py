"""DDPM pipeline (reference: rho_diffusion/diffusion/ddpm.py:46-371), same constructor and methods:
``forward_process`` (q_sample), ``reverse_process`` (ancestral p_sample loop), ``training_step``,
``p_sample`` / ``generate``, ``save_model_weights``.

The arithmetic runs in the HIP kernels of librho_hip.so:
  * q_sample       -> rho_q_sample (alpha_bar gathered per batch element on the device)
  * noise          -> rho_philox_normal (counter-based, reproducible per (seed, offset))
  * backbone       -> UNet engine (channels-last conv / GroupNorm / attention kernels)
  * reverse update -> rho_p_sample_step; the step index lives on the device (rho_step_advance), the
                      loop issues no host synchronisation and no per-step H2D copies
  * loss           -> rho_mse
  * guidance       -> classifier-free (not in the reference): label dropout in training_step (rho_cond_keep_mask draws, the
                      engine's rho_cond_drop applies), guided sampling at batch 2B with rho_p_sample_step_cfg
  * few steps      -> DDIM with eta on a spaced timestep sequence (not in the reference): reverse_process(num_steps=, eta=) walks
                      S of the T timesteps with rho_p_sample_step_spaced / rho_spaced_advance; host side in spaced.py
  * objective      -> prediction_type "epsilon" (the reference), "v" or "sample", and min-SNR-gamma loss weights (snr_gamma); neither in
                      the reference: the loss is rho_pred_loss_ws (target formed in the kernel), v / sample models sample on the
                      spaced walk with rho_p_sample_step_spaced_pred; host side in prediction.py
  * solver         -> sampler "dpmpp_2m", DPM-Solver++(2M) on log-SNR spaced timesteps (not in the reference): the spaced walk with
                      rho_dpmpp_2m_step and an x0 history on the device; host side in multistep.py
Reference quirks are kept deliberately: 0.8*sqrt(beta) noise scale, z = 0 for t <= 1,
no update at t = 0 although the backbone is evaluated, clamp to [-1, 1] after every update,
checkpoint spacing T // 10.
"""
from __future__ import annotations

import numbers
import os
from typing import Any, Iterable, Mapping, Union

import torch
from torch import Tensor, nn

from .. import hip
from ..engine import ops
from ..utils import sample_from_discrete_parameter_space, save_model_checkpoint
from .abstract_diffusion import AbstractDiffusionPipeline
from .multistep import SAMPLERS, SPACINGS, dpmpp_2m_coefficients, logsnr_timesteps
from .prediction import PREDICTION_TYPES, check_snr_gamma, min_snr_weights, resolve_prediction_type, spaced_pred_coefficients
from .spaced import resolve_timesteps, spaced_checkpoints

__all__ = ["DDPM"]


class DDPM(AbstractDiffusionPipeline):
    def __init__(self, backbone, backbone_kwargs: dict, schedule, loss_func, timesteps: Union[int, Tensor] = 1000,
                 cond_fn: str = None, cond_fn_kwargs: dict = None, optimizer=None,
                 opt_kwargs: Union[Mapping[str, Any], None] = {}, t_checkpoints=None, sampling_batch_size=10,
                 sample_every_n_epochs=5, sample_parameter_space=None, save_checkpoint_every_n_epochs=10,
                 sampling_steps=None, sampling_eta: float = 0.0, prediction_type: str = "epsilon", snr_gamma=None,
                 sampler: str = "ddim", sampling_spacing=None, guidance_scale=None, cond_drop_prob: float = 0.0):
        super().__init__(backbone=backbone, backbone_kwargs=backbone_kwargs, schedule=schedule, timesteps=timesteps,
                         cond_fn=cond_fn, cond_fn_kwargs=cond_fn_kwargs, optimizer=optimizer, opt_kwargs=opt_kwargs)
        self._init_loss_and_noise(loss_func)
        self.t_checkpoints = t_checkpoints
        self.sampling_batch_size = sampling_batch_size
        self.sample_every_n_epochs = sample_every_n_epochs
        self.sample_parameter_space = sample_parameter_space
        self.save_weights_every_n_epochs = save_checkpoint_every_n_epochs
        # classifier-free guidance (Ho & Salimans 2022): during training the labels of a sample are dropped with probability
        # ``cond_drop_prob`` (its condition becomes the zero row, the null condition); with ``guidance_scale`` = s set, sampling
        # evaluates the backbone on the labels and on the null condition and follows e_u + s * (e_c - e_u).  s = 1 is the
        # conditional model, s = 0 the unconditional one.  The defaults (None, 0) are the reference's behaviour.
        cond_drop_prob = float(cond_drop_prob)
        if not 0.0 <= cond_drop_prob < 1.0:
            raise ValueError(f"cond_drop_prob must lie in [0, 1): got {cond_drop_prob} (at 1 no sample would ever see its labels)")
        self.cond_drop_prob = cond_drop_prob
        self.guidance_scale = None if guidance_scale is None else float(guidance_scale)
        # few-step sampling: the defaults of reverse_process(num_steps=, eta=), so generate() / p_sample() / on_train_epoch_end
        # follow them.  None walks every timestep with the reference's update; a count or an explicit increasing sequence of
        # timesteps takes the DDIM update on those (eta = 0 deterministic, eta = 1 the ancestral variance).  Checked on first use.
        self.sampling_steps = sampling_steps
        self.sampling_eta = float(sampling_eta)
        self._spaced_cache = {}
        # the update of the few-step walk and how a step count picks its timesteps: the defaults of reverse_process_with(sampler=,
        # spacing=).  "ddim" is the first-order update above; "dpmpp_2m" is DPM-Solver++(2M) (Lu et al. 2022), second order at the
        # same number of backbone calls, deterministic (eta must be 0).  Spacing "uniform" is spaced_timesteps, "logsnr" is
        # logsnr_timesteps; None takes "uniform" for ddim and "logsnr" for dpmpp_2m, whose extrapolation needs steps of similar size
        # in log-SNR.
        self.sampler = self._check_sampler(sampler)
        self.sampling_spacing = self._check_spacing(sampling_spacing)
        # what the backbone predicts - "epsilon" (the reference), "v" (Salimans & Ho 2022) or "sample" (x0) - and min-SNR-gamma
        # loss weighting (Hang et al. 2023; None: every timestep weighs 1).  With the defaults training_step and reverse_process issue
        # the reference's launches; anything else trains through rho_pred_loss_ws, which has no torch counterpart on this path.
        self.prediction_type = resolve_prediction_type(prediction_type)
        self.snr_gamma = check_snr_gamma(snr_gamma)
        if (self.prediction_type != "epsilon" or self.snr_gamma is not None) and not (
                isinstance(self.loss_func, nn.MSELoss) and self.loss_func.reduction == "mean"):
            raise ValueError(f"prediction_type={self.prediction_type!r} / snr_gamma={self.snr_gamma} need loss_func nn.MSELoss(reduction='mean'): "
                             f"the weighted loss is a HIP kernel of that form and has no torch fallback; got {self.loss_func!r}")
        self._snr_weights = {}
        self._nan_flag = None
        self.nan_check_every = 50
        self._steps_seen = 0
        # reverse_process: capture one denoising step (Philox draw, UNet forward, update, device-side step advance) in a
        # HIP graph and replay it; the step index and RNG offset live on the device, so one graph serves every t.  Pays
        # where the step is launch-bound (2-D 64^2: ~190 launches of a few microseconds each); bit-identical to the
        # eager loop.  Falls back to the eager loop if capture is not possible (e.g. label lookups that synchronise).
        self.hip_graph_sampling = os.environ.get("RHO_HIP_GRAPH", "1") != "0"
        # training_step: draw t on the device (rho_randint, Philox stream of this rank) instead of the reference's CPU
        # torch.randint + H2D copy (abstract_diffusion.py:163-169, ddpm.py:264).  Off by default: the CPU draw follows
        # torch.manual_seed like the reference; DPTrainer / bench.py switch it on.
        self.device_timesteps = os.environ.get("RHO_DEVICE_TIMESTEPS", "0") == "1"

    # ------------------------------------------------------------------ q_sample (noise, ddpm.py:101-102, is the base class's Philox draw)
    def forward_process(self, data: Tensor, t: Union[Tensor, None] = None) -> list:
        """ddpm.py:104-130: returns [x_t, noise]."""
        hip.require_gpu(data, "data")
        batch_size = data.size(0)
        self.schedule.dtype = data.dtype
        if t is None:
            t = self._draw_timesteps(batch_size, data.device)
        n_rows = len(self.schedule["alpha_bar_t"])
        if not t.is_cuda and t.numel() and (int(t.max()) >= n_rows or int(t.min()) < -n_rows):
            # same failure as the reference's table gather (abstract_diffusion.py:216-220) when `timesteps` exceeds the
            # schedule length; timesteps already on the device are checked by the kernel instead (flag bit 2, see _check_nan)
            raise IndexError(f"index {int(t.max())} is out of bounds for dimension 0 with size {n_rows}")
        t = t.reshape(-1).to(device=data.device, dtype=torch.int64).contiguous()
        x0 = data.float().contiguous()
        noise = self.noise(x0)
        tables = self.schedule.device_tables(data.device)
        if self._nan_flag is None or self._nan_flag.device != data.device:
            self._nan_flag = torch.zeros(1, dtype=torch.int32, device=data.device)
        x_t = ops.q_sample(x0, noise.contiguous(), t, tables["alpha_bar"], nan_flag=self._nan_flag)
        return [x_t.type(data.dtype), noise.type(data.dtype)]

    # ------------------------------------------------------------------ p_sample loop
    def _refuse_unguidable(self, conditions) -> None:
        """The requirements of guided sampling that can be checked before anything is drawn."""
        if conditions is None:
            raise ValueError("guidance_scale needs `conditions`: guidance contrasts the labelled prediction with the unlabelled one")
        if not hasattr(self.backbone, "engine"):
            raise ValueError(f"guidance_scale needs a backbone with a HIP engine that takes labels; {type(self.backbone).__name__} "
                             "is unconditional")
        if getattr(self.backbone, "num_classes", None) is None:
            raise ValueError("guidance_scale needs a class-conditional backbone (num_classes is None)")

    @staticmethod
    def _check_sampler(name) -> str:
        if isinstance(name, str) and name in SAMPLERS:
            return name
        raise ValueError(f"sampler must be one of {', '.join(repr(s) for s in SAMPLERS)}: got {name!r}")

    @staticmethod
    def _check_spacing(name):
        if name is None or (isinstance(name, str) and name in SPACINGS):
            return name
        raise ValueError(f"spacing must be None or one of {', '.join(repr(s) for s in SPACINGS)}: got {name!r}")

    @torch.no_grad()  # (reference: inference_mode; no_grad keeps the plan buffers usable in training too)
    def reverse_process(self, x_T: Tensor, conditions=None, t_checkpoints=None, guidance_scale=None, num_steps=None, eta=None,
                        clip_denoised: bool = True) -> dict:
        """reverse_process_with under the attributes ``sampler`` and ``sampling_spacing``: the reference's method and its keywords,
        unchanged.  The update of the few-step walk and the timestep spacing are chosen on the pipeline (DDPM(sampler=,
        sampling_spacing=), or by setting the attributes), or per call through reverse_process_with."""
        return self.reverse_process_with(x_T, conditions, t_checkpoints, guidance_scale, num_steps, eta, clip_denoised)

    @torch.no_grad()
    def reverse_process_with(self, x_T: Tensor, conditions=None, t_checkpoints=None, guidance_scale=None, num_steps=None, eta=None,
                             clip_denoised: bool = True, sampler=None, spacing=None) -> dict:
        """reverse_process with the sampler and the spacing chosen per call (reverse_process itself keeps the keywords it had).
        ddpm.py:132-229.  ``x_T`` is only a shape/device template (:171).  ``guidance_scale`` (default: the attribute of that
        name; None = the reference's loop) samples with classifier-free guidance: the engine runs at batch 2B on
        cat(x_t, x_t) with cat(embedded labels, zeros), rho_p_sample_step_cfg combines the two predictions, applies the update
        and writes it to both halves.  The noise draws, their Philox offsets and the returned shapes are those of the unguided
        call.

        ``num_steps`` (default: the attribute ``sampling_steps``; None = every timestep, the loop above) samples in few steps:
        a count S takes spaced_timesteps(T, S), a strictly increasing sequence is taken as given, and the walk applies the DDIM
        update with ``eta`` (default: ``sampling_eta``) on those timesteps - _reverse_process_spaced.  ``clip_denoised`` clamps its x0
        estimate to [-1, 1]; the full loop clamps x_t itself and has no such switch.

        The full loop is the reference's (0.8 sqrt(beta) noise, clamp of x_t): parity code for epsilon models, and it stays
        epsilon-only.  With ``prediction_type`` "v" or "sample" every path is the spaced walk on rho_p_sample_step_spaced_pred:
        ``num_steps`` None then walks all T timesteps (taus = range(T)) with ``eta``, and a timestep with alpha_bar == 0 is legal.

        ``sampler`` (default: the attribute of that name) chooses the update of the spaced walk: "ddim" as above, or "dpmpp_2m",
        DPM-Solver++(2M) on rho_dpmpp_2m_step - second order, no noise (``eta`` must be 0), for every prediction type; it needs
        a walk, so an epsilon model must give ``num_steps``.  ``spacing`` (default: ``sampling_spacing``) says how a step COUNT picks
        its timesteps: "uniform" (spaced_timesteps), "logsnr" (logsnr_timesteps), None = "uniform" for ddim and "logsnr" for
        dpmpp_2m; with an explicit sequence a spacing is refused."""
        scale = self.guidance_scale if guidance_scale is None else float(guidance_scale)
        if scale is not None:
            self._refuse_unguidable(conditions)
        sampler = self.sampler if sampler is None else self._check_sampler(sampler)
        if spacing is None and num_steps is not None and not isinstance(num_steps, numbers.Integral):
            spacing = None                                  # a sequence given with the call outranks the attribute's spacing
        else:
            spacing = self.sampling_spacing if spacing is None else self._check_spacing(spacing)
        num_steps = self.sampling_steps if num_steps is None else num_steps
        if num_steps is None and self.prediction_type != "epsilon":
            num_steps = range(len(self.schedule["alpha_bar_t"]))
            spacing = None                                  # every timestep: nothing to choose
        if num_steps is None and sampler != "ddim":
            raise ValueError(f"sampler={sampler!r} walks a timestep sequence: give num_steps (the full loop of an epsilon model is the "
                             "reference's ancestral sampler)")
        spaced = None
        if num_steps is not None:
            spaced = self._spaced_host(num_steps, self.sampling_eta if eta is None else eta, sampler, spacing)   # ValueError before any draw
        elif not clip_denoised:
            raise ValueError("clip_denoised=False needs num_steps: the full loop clamps x_t after every update as the reference does")
        hip.require_gpu(x_T, "x_T")
        dev = x_T.device
        batch_size = x_T.size(0)
        self.schedule.dtype = x_T.dtype
        num_checkpoints = len(t_checkpoints) if t_checkpoints is not None else 0
        buf = None
        if t_checkpoints is not None:
            buf = torch.zeros((batch_size, num_checkpoints) + tuple(x_T.shape[1:]), dtype=torch.float32, device=dev)

        denoise_steps = len(self.schedule["alpha_bar_t"])
        steps_per_ckpt = denoise_steps // 10
        tables = self.schedule.device_tables(dev)

        x_t = self.noise(x_T).contiguous()

        cc = self._preembed_conditions(self._resolve_conditions(conditions, batch_size, dev))

        engine = self.backbone.engine() if hasattr(self.backbone, "engine") else None
        t_dev = torch.full((1,), denoise_steps - 1 if spaced is None else spaced["taus"][-1], dtype=torch.int32, device=dev)
        if scale is None:
            x_all = x_t                                     # what the backbone reads

            def update(pred, z):
                ops.p_sample_step(x_t, pred, z, tables["coef"], t_dev)
        else:
            e = 4 * self.backbone.model_channels
            if not (torch.is_tensor(cc) and cc.dim() == 2 and tuple(cc.shape) == (batch_size, e)):
                raise ValueError(f"guidance_scale needs conditions that embed to [batch, 4 * model_channels] = ({batch_size}, {e}), "
                                 "whose null condition is the zero row: the backbone's cond_fn does not give that form for "
                                 f"{'these conditions' if not torch.is_tensor(cc) else tuple(cc.shape)}")
            # the doubled batch: rows [0, B) carry the labels, rows [B, 2B) the null condition; x_t is its first half from here on
            cc = cc.to(device=dev, dtype=torch.float32)
            cc = torch.cat([cc, torch.zeros_like(cc)]).contiguous()
            x_all = torch.cat([x_t, x_t])
            x_t = x_all[:batch_size]

            def update(pred, z):
                ops.p_sample_step_cfg(x_all, pred, z, tables["coef"], t_dev, scale)
        if spaced is not None:
            return self._reverse_process_spaced(x_all, x_t, cc, engine, scale, spaced, bool(clip_denoised), t_dev, buf)
        return self._run_walk(x_all, x_t, cc, engine, t_dev, buf, denoise_steps, host_t=lambda t: t, z_from=2, update=update,
                              advance=lambda off_dev, delta: ops.step_advance(t_dev, off_dev, delta), state=(t_dev,),
                              is_checkpoint=lambda t: t % steps_per_ckpt == 0)

    def _run_walk(self, x_all, x_t, cc, engine, t_dev, buf, steps, host_t, z_from, update, advance, state, is_checkpoint) -> dict:
        """The loop of every reverse process over the step index i = steps-1 .. 0 (t itself in the full loop, k in the spaced walk):
        draw z where i >= ``z_from`` (None: never; before the backbone call, :196-199), evaluate the backbone at the timestep in
        ``t_dev``, ``update(pred, z)``, copy x_t to the next row of ``buf`` where ``is_checkpoint(i)``, ``advance(offset_dev, delta)``.
        ``x_all`` is what the backbone reads and ``update`` writes - ``x_t`` itself, or under guidance the doubled batch whose first
        half ``x_t`` is (``cc`` then carries the null rows).  The step index and the timestep live on the device (``state``: the
        scalars that ``advance`` moves), so the loop issues no host synchronisation and one captured graph serves every step
        (_replay_walk); ``host_t(i)`` is the timestep on the host, which only a backbone without an engine needs.  At t = 0 the full
        loop's update kernel writes nothing although the backbone is evaluated, as in the reference."""
        num_checkpoints = buf.size(1) if buf is not None else 0
        t_idx = 0

        def checkpoint(i):
            nonlocal t_idx
            if buf is not None and is_checkpoint(i) and t_idx < num_checkpoints:
                buf[:, t_idx].copy_(x_t)
                t_idx += 1

        if (self.hip_graph_sampling and engine is not None and steps > 2 and "noise" not in self.__dict__
                and type(self).noise is AbstractDiffusionPipeline.noise):
            if self._replay_walk(x_all, x_t, cc, engine, t_dev, buf, steps, z_from, update, advance, state, checkpoint):
                self._check_backbone_errors()
                return {"buffer": buf, "denoised": x_t}
            t_idx = 0
        for i in range(steps - 1, -1, -1):
            z = self.noise(x_t) if z_from is not None and i >= z_from else None
            if engine is not None:
                pred = engine.forward(x_all, None, cc, t_scalar_dev=t_dev)
            else:
                pred = self.backbone(x_t, torch.full((x_t.size(0),), host_t(i), device=x_t.device, dtype=torch.long), cc)
            update(pred.contiguous(), z)
            checkpoint(i)
            advance(None, 0)
        self._check_backbone_errors()
        return {"buffer": buf, "denoised": x_t}

    def _replay_walk(self, x_all, x_t, cc, engine, t_dev, buf, steps, z_from, update, advance, state, checkpoint) -> bool:
        """The loop of _run_walk with steps i = steps-2 .. 0 replayed from one captured HIP graph (step steps-1 runs eagerly: it
        builds the engine plan and its buffers).  Same arithmetic and the same Philox stream as the eager loop: where the walk draws
        at all, the captured step draws z at every replay from a device-side offset that ``advance`` moves; the draws below
        ``z_from`` are ignored by the update kernel (t <= 1 in the full loop, row 0 of the spaced walk has sigma = 0) and not counted,
        so the offset ends where the eager loop leaves it.  A walk without noise has no Philox kernel in its graph.  Returns False
        (x_all, ``state`` and ``buf`` as they were) if the capture fails."""
        delta = (x_t.numel() + 3) // 4
        noisy = z_from is not None
        z = torch.empty_like(x_t) if noisy else None
        off_dev = torch.full((1,), self._noise_offset, dtype=torch.int64, device=x_t.device) if noisy else None
        x_save, state_save = x_all.clone(), [s.clone() for s in state]

        def step():
            if noisy:
                ops.philox_normal(z, self.noise_seed, 0, offset_dev=off_dev)
            pred = engine.forward(x_all, None, cc, t_scalar_dev=t_dev)
            update(pred, z)
            advance(off_dev, delta)

        try:
            step()                                      # i = steps-1, eager
            checkpoint(steps - 1)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):   # other threads (RCCL watchdog) may call HIP
                step()
        except Exception as exc:  # noqa: BLE001  (capture is an optimisation; any failure -> eager loop)
            torch.cuda.synchronize()
            x_all.copy_(x_save)
            for s, saved in zip(state, state_save):
                s.copy_(saved)
            if buf is not None:
                buf.zero_()
            self.hip_graph_sampling = False
            import warnings
            warnings.warn(f"HIP graph capture of the sampling step failed ({type(exc).__name__}: {exc}); using the eager loop")
            return False
        for i in range(steps - 2, -1, -1):
            graph.replay()
            checkpoint(i)
        if noisy:
            self._noise_offset += delta * (steps - z_from)      # eager-loop bookkeeping: one draw per i >= z_from
        return True

    # ------------------------------------------------------------------ few-step sampling
    def _alpha_bar32(self) -> Tensor:
        with self.schedule:                                                          # float32 tables whatever the data dtype
            return self.schedule["alpha_bar_t"].clone()

    def _spaced_host(self, num_steps, eta, sampler: str = "ddim", spacing=None) -> dict:
        """Timesteps and coefficient rows of a spaced walk, cached per (taus, eta, prediction type, sampler): host work only, refusals
        included.  ``spacing`` picks the timesteps of a step count (None: "uniform" for ddim, "logsnr" for dpmpp_2m) and is refused
        with an explicit sequence; the rows are spaced_pred_coefficients for "ddim", dpmpp_2m_coefficients for "dpmpp_2m"."""
        T = len(self.schedule["alpha_bar_t"])
        sampler, spacing = self._check_sampler(sampler), self._check_spacing(spacing)
        eta = float(eta)
        if sampler == "dpmpp_2m" and eta != 0.0:
            raise ValueError(f"sampler='dpmpp_2m' is deterministic and takes no eta: got {eta}")
        is_count = isinstance(num_steps, numbers.Integral) and not isinstance(num_steps, bool)
        if not is_count and spacing is not None:
            raise ValueError(f"spacing={spacing!r} chooses the timesteps of a step count; num_steps is an explicit timestep sequence")
        if is_count and (spacing or ("logsnr" if sampler == "dpmpp_2m" else "uniform")) == "logsnr":
            taus = tuple(logsnr_timesteps(self._alpha_bar32(), num_steps))
        else:
            taus = tuple(resolve_timesteps(T, num_steps))
        pred = self.prediction_type
        key = (taus, eta, pred, sampler)
        if key not in self._spaced_cache:
            ab = self._alpha_bar32()
            rows = dpmpp_2m_coefficients(ab, taus, pred) if sampler == "dpmpp_2m" else spaced_pred_coefficients(ab, taus, eta, pred)
            self._spaced_cache[key] = {"taus": taus, "eta": eta, "pred": pred, "sampler": sampler, "rows": rows, "T": T, "dev": {}}
        return self._spaced_cache[key]

    def _spaced_device(self, spaced: dict, dev):
        """(rows [S, 8] float32, taus [S] int32) on ``dev``, uploaded once per (device, taus, eta, prediction type)."""
        key = str(torch.device(dev))
        if key not in spaced["dev"]:
            spaced["dev"][key] = (spaced["rows"].contiguous().to(dev), torch.tensor(spaced["taus"], dtype=torch.int32).to(dev))
        return spaced["dev"][key]

    def _spaced_update(self, x_all, pred, z, rows, k_dev, scale, clip, kind, hist=None) -> None:
        """The update of one step of the spaced walk, by the sampler and by what the backbone predicts: the rows are of that kind
        (_spaced_host).  ``hist`` is the multistep solver's x0 history and marks its walk; the DDIM walks carry None."""
        if hist is not None:
            ops.dpmpp_2m_step(x_all, pred, hist, rows, k_dev, PREDICTION_TYPES[kind], scale, clip)
        elif kind == "epsilon":
            ops.p_sample_step_spaced(x_all, pred, z, rows, k_dev, scale, clip)
        else:
            ops.p_sample_step_spaced_pred(x_all, pred, z, rows, k_dev, PREDICTION_TYPES[kind], scale, clip)

    def _reverse_process_spaced(self, x_all, x_t, cc, engine, scale, spaced, clip, t_dev, buf) -> dict:
        """The walk over ``spaced["taus"]`` from the top, k = S-1 .. 0, as _run_walk drives it: z is drawn for eta > 0 and k >= 1 only,
        the backbone is evaluated at t = tau_k, the update is rho_p_sample_step_spaced (rho_p_sample_step_spaced_pred for a v or x0
        model) on row k, the advance rho_spaced_advance on k and t.

        With sampler "dpmpp_2m" the update is rho_dpmpp_2m_step on the rows of dpmpp_2m_coefficients: no z is drawn, and ``hist``, an
        ordinary device tensor of x_t's shape, carries the x0 estimate from one step to the next - read and written by the captured
        step like x_all.  It is not zeroed: row S-1 is first order and does not read it."""
        taus, kind = spaced["taus"], spaced["pred"]
        S = len(taus)
        rows, taus_dev = self._spaced_device(spaced, x_all.device)
        k_dev = torch.full((1,), S - 1, dtype=torch.int32, device=x_all.device)
        ckpt = spaced_checkpoints(spaced["T"], taus) if buf is not None else ()
        hist = torch.empty_like(x_t) if spaced.get("sampler", "ddim") == "dpmpp_2m" else None
        return self._run_walk(x_all, x_t, cc, engine, t_dev, buf, S, host_t=lambda k: taus[k], z_from=1 if spaced["eta"] > 0.0 else None,
                              update=lambda pred, z: self._spaced_update(x_all, pred, z, rows, k_dev, scale, clip, kind, hist),
                              advance=lambda off_dev, delta: ops.spaced_advance(k_dev, t_dev, taus_dev, off_dev, delta),
                              state=(k_dev, t_dev), is_checkpoint=lambda k: taus[k] in ckpt)

    # ------------------------------------------------------------------ training
    def _draw_timesteps(self, batch_size: int, device) -> Tensor:
        """random_timesteps on the device when ``device_timesteps`` is set (no H2D copy), else the reference's CPU draw."""
        if self.device_timesteps and torch.device(device).type == "cuda" and "random_timesteps" not in self.__dict__:
            t = ops.randint(batch_size, int(self.timesteps), self.noise_seed ^ 0x5DEECE66D, self._noise_offset, device=device)
            self._noise_offset += (batch_size + 3) // 4
            return t
        return self.random_timesteps(batch_size).to(device)

    def _draw_cond_keep(self, batch_size: int, device) -> Tensor:
        """uint8 [B] keep mask of the label dropout: 1 with probability 1 - cond_drop_prob, drawn on the device from this rank's
        Philox stream under a seed of its own (rho_cond_keep_mask), the shared offset advanced as ``_draw_timesteps`` does.
        Tests override it to inject a mask, as they inject ``noise``."""
        keep = ops.cond_keep_mask(batch_size, self.cond_drop_prob, self.noise_seed ^ 0x2545F4914F6CDD1D, self._noise_offset, device=device)
        self._noise_offset += (batch_size + 3) // 4
        return keep

    def _snr_weight_table(self, dev):
        """float32 [T] min-SNR-gamma weights of this objective on ``dev`` (None without ``snr_gamma``), built once per (device, objective, gamma)."""
        if self.snr_gamma is None:
            return None
        key = (str(torch.device(dev)), self.prediction_type, self.snr_gamma)
        if key not in self._snr_weights:
            with self.schedule:                                                      # float32 tables whatever the data dtype
                ab = self.schedule["alpha_bar_t"].clone()
            self._snr_weights[key] = min_snr_weights(ab, self.prediction_type, self.snr_gamma).contiguous().to(dev)
        return self._snr_weights[key]

    def _check_nan(self, force: bool = False) -> None:
        """Device-side form of the per-step host check at ddpm.py:268-272: the flag is set by the
        q_sample kernel and polled every ``nan_check_every`` steps instead of syncing each step.
        Bit 0: NaN in the noised data; bit 2: a timestep outside the schedule table (IndexError in the reference)."""
        self._steps_seen += 1
        due = force or self._steps_seen % self.nan_check_every == 0
        if due:
            self._check_backbone_errors()      # labels of the PREVIOUS steps (the flag is sticky until polled)
        if self._nan_flag is not None and due:
            v = int(self._nan_flag.item())
            if v & 4:
                self._nan_flag.zero_()
                raise IndexError(f"a timestep is out of bounds for the schedule tables of size {len(self.schedule['alpha_bar_t'])}")
            if v & 1:
                print("Error: Noised data contains NaNs. Check your noise scheduler.")
                import sys
                sys.exit(0)

    def training_step(self, batch: Iterable[Any], batch_idx: int = 0):
        """ddpm.py:231-288: eps-prediction objective; with ``prediction_type`` / ``snr_gamma`` set the backbone is regressed onto v or
        x0 instead and timestep t weighs min_snr_weights[t] (rho_pred_loss_ws: the target is formed in the kernel from the clean data,
        the noise and t)."""
        if isinstance(batch, list):
            data, labels = batch
        elif isinstance(batch, dict):
            data = batch.get("data")
            labels = batch.get("label")
        else:
            data = batch
            labels = None
        self.data_shape = data.shape
        self.data_dtype = data.dtype
        batch_size = data.size(0)
        t = self._draw_timesteps(batch_size, data.device)
        x_data, noise = self.forward_process(data, t)
        self._check_nan()
        if labels is not None and self.cond_drop_prob > 0.0 and self.backbone.training and torch.is_grad_enabled():
            if not hasattr(self.backbone, "engine"):
                raise ValueError(f"cond_drop_prob needs a backbone with a HIP engine that takes labels, not {type(self.backbone).__name__}")
            engine = self.backbone.engine()
            engine.set_cond_keep(self._draw_cond_keep(batch_size, data.device))     # consumed by the training forward below
            try:
                pred_noise = self.backbone(x_data, t, labels)
            finally:
                engine.set_cond_keep(None)
        elif labels is not None:
            pred_noise = self.backbone(x_data, t, labels)
        else:
            pred_noise = self.backbone(x_data, t)
        if self.prediction_type != "epsilon" or self.snr_gamma is not None:
            from ..autograd import pred_loss
            dev = pred_noise.device
            loss = pred_loss(pred_noise, data, noise, t.reshape(-1).to(device=dev, dtype=torch.int64).contiguous(),
                             self.schedule.device_tables(dev)["alpha_bar"], self._snr_weight_table(dev),
                             PREDICTION_TYPES[self.prediction_type], self._nan_flag)       # a bad t: bit 2, raised by _check_nan
        elif isinstance(self.loss_func, nn.MSELoss) and self.loss_func.reduction == "mean":
            from ..autograd import mse_loss
            loss = mse_loss(pred_noise, noise)           # HIP reduction + gradient (rho_mse)
        else:
            loss = self.loss_func(pred_noise, noise)
        # whatever the user put into self.metrics (empty by default), between the noised and the clean data (ddpm.py:283-285)
        for key, metric in self.metrics.items():
            with torch.no_grad():
                self.log(f"train_{key}", metric(x_data, data))
        self.log("train_loss", loss, prog_bar=True)
        return loss

    def forward(self, batch):
        return self.backbone(batch)

    def on_train_epoch_end(self) -> None:
        if (self.current_epoch > 0 and self.sample_every_n_epochs > 0
                and self.current_epoch % self.sample_every_n_epochs == 0):
            self.eval()
            self.generate()
        if (self.current_epoch > 0 and self.save_weights_every_n_epochs > 0
                and self.current_epoch % self.save_weights_every_n_epochs == 0):
            self.eval()
            self.save_model_weights()

    def p_sample(self, parameter_space, random=False):
        """ddpm.py:319-355."""
        if hasattr(self, "data_shape"):
            shape = [int(x) for x in self.data_shape]
            shape[0] = self.sampling_batch_size
        else:
            shape = [self.sampling_batch_size, self.backbone_kwargs["out_channels"]] + list(self.backbone_kwargs["data_shape"])
            self.data_dtype = torch.float32
        sample_data = torch.zeros(shape, dtype=self.data_dtype, device=self.device)
        cond = None
        if parameter_space is not None:
            cond = sample_from_discrete_parameter_space(parameter_space, sample_data.shape[0], random=random, device=self.device)
        results = self.reverse_process(x_T=sample_data, conditions=cond, t_checkpoints=self.t_checkpoints, guidance_scale=self.guidance_scale)
        self.last_samples = results
        return self.make_image_grid(results["denoised"], filename="output_%d.png" % self.current_epoch)

    def generate(self, parameter_space=None, random=False):
        if parameter_space is None:
            parameter_space = self.sample_parameter_space
        return self.p_sample(parameter_space=parameter_space, random=random)

    def save_model_weights(self):
        print("saving model checkpoints...")
        save_model_checkpoint(self.backbone, "model.pth")

    def validation_step(self, batch, batch_idx: int = 0):
        return 0
