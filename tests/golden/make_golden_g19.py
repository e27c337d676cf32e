"""Generate tests/golden/g19_learned_variance.npz from the REAL reference: GaussianDiffusionPipeline with a learned variance
(model_var_type LEARNED / LEARNED_RANGE, gaussian_diffusion.py:368-383), a UNetv2 with out_channels = 2 * in_channels, and the hybrid
training loss L_simple + L_vlb (:893-930).

Run in the build container only:  ``python tests/golden/make_golden_g19.py``.  As make_golden_g18.py: the reference is imported in
place through ``make_golden.load_reference``, weights come from ``detdata.det_state_dict`` on both sides and every random draw of the
reference is replaced by a recorded tape.  Only inputs and outputs are written (CPU, float32, one thread)."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from detdata import det_normal, det_state_dict, det_uniform  # noqa: E402
from golden_cfg import UNET_CASES  # noqa: E402
from make_golden import grad_digest, load_reference, np_  # noqa: E402
from make_golden_g18 import GRAD_KEYS, Tape, tape_tensors  # noqa: E402

CASES = (("tiny2d", 50), ("tiny3d", 20))
VAR_TYPES = ("LEARNED", "LEARNED_RANGE")
MEAN_TYPES = ("START_X", "EPSILON")


def lv_kwargs(case):
    kw, xshape, _ = UNET_CASES[case]
    return dict(kw, out_channels=2 * kw["in_channels"]), xshape


def model_output(xshape, vt):
    """A [B, 2C, ...] output: the mean half like g18's fake output, the variance half in the range each type expects."""
    B = xshape[0]
    scale = torch.tensor([0.3] + [2.5 + i for i in range(B - 1)]).view(-1, *([1] * (len(xshape) - 1)))
    mean = det_normal(xshape, "g19_fake") * scale
    v = det_uniform(xshape, "g19_var", -1.0, 1.0)
    if vt == "LEARNED":
        v = v * 3.0 - 6.0                                     # log-variances around the schedule's
    return torch.cat([mean, v], dim=1)


def x_start_with_edges(xshape):
    """x_start in [-1, 1] with exact +-1 entries (both where-branches of the decoder likelihood) and +-0.999 neighbours."""
    x = det_uniform(xshape, "g19_x0", -1.0, 1.0)
    flat = x.view(xshape[0], -1)
    f = np.float32
    edges = torch.tensor([f(-1.0), f(1.0), f(-0.999), f(0.999), np.nextafter(f(0.999), f(1)), np.nextafter(f(-0.999), f(-1))])
    flat[:, : len(edges)] = edges
    return x


def gen_case(R, GD, case, T, g):
    U = R.unet_v2
    kw, xshape = lv_kwargs(case)
    gd = GD.GaussianDiffusionPipeline(U.UNet, dict(kw), R.sched.LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T)
    gd.backbone.load_state_dict(det_state_dict(gd.backbone.state_dict(), case + "_lv"))
    gd.backbone.eval()
    gd.log = lambda *a, **k: None
    tag = f"{case}_T{T}"
    B = xshape[0]
    g[f"{tag}/tab/min_log"] = np.asarray(gd.posterior_log_variance_clipped, dtype=np.float64)
    g[f"{tag}/tab/max_log"] = np.log(gd.betas)

    x0 = x_start_with_edges(xshape)
    xt = det_normal(xshape, "g19_xt")
    g[f"{tag}/x0"], g[f"{tag}/xt"] = np_(x0), np_(xt)
    tt = torch.tensor([0, T - 1] + [T // 2] * (B - 2))
    g[f"{tag}/t"] = np_(tt)
    noise = det_normal(xshape, "g19_step_noise")
    grad = lambda x, t, **k: -x
    for vt in VAR_TYPES:
        out2 = model_output(xshape, vt)
        g[f"{tag}/mo_{vt}"] = np_(out2)
        model = lambda x, t, o=out2, **k: o
        for mt in MEAN_TYPES:
            gd.model_mean_type, gd.model_var_type = GD.ModelMeanType[mt], GD.ModelVarType[vt]
            for clip in (True, False):
                o = gd.p_mean_variance(model, xt, tt, clip_denoised=clip)
                k = f"{tag}/pmv_{vt}_{mt}_{int(clip)}"
                for n in ("mean", "variance", "log_variance", "pred_xstart"):
                    g[f"{k}/{n}"] = np_(o[n])
            for cn, cf in (("nocond", None), ("cond", grad)):
                with Tape([noise]):
                    o = gd.p_sample(model, xt, tt, clip_denoised=True, cond_fn=cf, model_kwargs={})
                g[f"{tag}/psample_{vt}_{mt}_{cn}/sample"] = np_(o["sample"])
            with Tape([noise]):
                o = gd.ddim_sample(model, xt, tt, clip_denoised=True, model_kwargs={}, eta=0.5)
            g[f"{tag}/ddim_{vt}_{mt}/sample"] = np_(o["sample"])
            # variational-bound terms: t = 0 (decoder NLL, x_start hits both where-branches) and t > 0 (KL)
            for tn, tv in (("t0", torch.zeros(B, dtype=torch.long)), ("tk", torch.full((B,), T // 3, dtype=torch.long))):
                x_t = gd.q_sample(x0, tv, noise=det_normal(xshape, "g19_vb_noise"))
                o = gd._vb_terms_bpd(model, x0, x_t, tv, clip_denoised=False)
                g[f"{tag}/vb_{vt}_{mt}_{tn}"] = np_(o["output"])

    # ---- training_losses terms and the gradient of loss.mean() w.r.t. the model output (a leaf)
    tq = torch.tensor([0] + [(5 * i + 2) % T for i in range(1, B)])           # sample 0 at t = 0: the decoder NLL's gradient
    g[f"{tag}/train_t"] = np_(tq)
    tnoise = det_normal(xshape, "g19_train_noise")
    for vt in VAR_TYPES:
        for mt in MEAN_TYPES:
            for lt in ("MSE", "RESCALED_MSE"):
                gd.model_mean_type, gd.model_var_type, gd.loss_type = GD.ModelMeanType[mt], GD.ModelVarType[vt], GD.LossType[lt]
                leaf = model_output(xshape, vt).requires_grad_(True)
                terms = gd.training_losses(lambda *a, **k: leaf, x0, tq, noise=tnoise)
                terms["loss"].mean().backward()
                k = f"{tag}/train_{vt}_{mt}_{lt}"
                for n in ("loss", "mse", "vb"):
                    g[f"{k}/{n}"] = np_(terms[n])
                g[f"{k}/dout"] = np_(leaf.grad)

    # ---- the backbone: loops, bits/dim, training_losses and training_step parameter gradients (LEARNED_RANGE, the improved-DDPM setup)
    gd.model_mean_type, gd.model_var_type, gd.loss_type = GD.ModelMeanType.EPSILON, GD.ModelVarType.LEARNED_RANGE, GD.LossType.RESCALED_MSE
    with torch.no_grad():
        tape = tape_tensors(xshape, f"g19tape{T}", T + 1)
        with Tape(tape):
            g[f"{tag}/p_sample_loop"] = np_(gd.p_sample_loop(gd.backbone, xshape, device="cpu"))
        with Tape(tape):
            g[f"{tag}/ddim_sample_loop"] = np_(gd.ddim_sample_loop(gd.backbone, xshape, device="cpu", eta=0.5))
        if T == 20:
            with Tape(tape_tensors(xshape, f"g19bpd{T}", T)):
                res = gd.calc_bpd_loop(gd.backbone, x0, clip_denoised=True)
            for k, v in res.items():
                g[f"{tag}/bpd/{k}"] = np_(v)
        # reverse_process (generate's body): DDIM with eta = 0 on the mean half, x0-predicting (the pipeline's reverse_process)
        gd.model_mean_type = GD.ModelMeanType.START_X
        with Tape(tape):
            g[f"{tag}/reverse_process"] = np_(gd.reverse_process(torch.zeros(xshape))["denoised"])
    gd.backbone.train()
    for mt in MEAN_TYPES:
        gd.model_mean_type = GD.ModelMeanType[mt]
        gd.backbone.zero_grad(set_to_none=True)
        terms = gd.training_losses(gd.backbone, x0, tq, noise=tnoise)
        terms["loss"].mean().backward()
        k = f"{tag}/bb_train_{mt}"
        for n in ("loss", "mse", "vb"):
            g[f"{k}/{n}"] = np_(terms[n])
        sd = dict(gd.backbone.named_parameters())
        for name, v in grad_digest([(n, sd[n].grad) for n in GRAD_KEYS]).items():
            g[f"{k}/grad/{name}"] = v
    # training_step (:1153-1210): fixed t, tape noise; the data are noised twice
    gd.model_mean_type = GD.ModelMeanType.EPSILON
    gd.backbone.zero_grad(set_to_none=True)
    gd.random_timesteps = lambda n, tq=tq: tq
    gd.noise = lambda data, e=tnoise: e
    loss = gd.training_step(x0)
    loss.backward()
    g[f"{tag}/step/loss"] = np_(loss.detach())
    sd = dict(gd.backbone.named_parameters())
    for name, v in grad_digest([(n, sd[n].grad) for n in GRAD_KEYS]).items():
        g[f"{tag}/step/grad/{name}"] = v
    print("G19", tag, float(loss.detach()), float(g[f"{tag}/p_sample_loop"].std()))


def main():
    torch.set_num_threads(1)
    R = load_reference()
    GD = importlib.import_module("rho_diffusion.diffusion.gaussian_diffusion")
    g = {}
    for case, T in CASES:
        gen_case(R, GD, case, T, g)
    np.savez_compressed(os.path.join(HERE, "g19_learned_variance.npz"), **g)
    print("wrote", len(g), "arrays")


if __name__ == "__main__":
    main()
