"""Cost of a learned variance (model_var_type LEARNED_RANGE, UNetv2 with out_channels = 2) in GaussianDiffusionPipeline.

    python tools/gd_learned_probe.py [--configs c3 c5] [--steps 8] [--reps 3] [--out DIR]

Sibling of gd_api_probe.py on the same geometries (c3: bf16 3-D 64^3, mc 64, B 32; c5: bf16 3-D 128^3, mc 32, B 2, labels).  For a
fixed-variance pipeline (1-channel head) and a learned-variance one (2-channel head, same weights elsewhere): per-step time of
reverse_process, p_sample_loop, ddim_sample_loop(eta=0.5) and calc_bpd_loop (HIP events around loops of ``--steps`` steps after a
warm-up, median of ``--reps``), the engine forward alone, the hybrid-loss passes on their own (rho_gd_hybrid_loss /
rho_gd_hybrid_loss_bwd, bytes they must move and TB/s) and, on c3, one training step with the hybrid loss against the MSE step.
One JSON line per configuration on stdout (and in DIR/gd_learned_probe.jsonl)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gd_api_probe import PRESETS, event_ms, labels  # noqa: E402


def pipelines(cfg, T, dev):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType
    from rho_diffusion_amd.models import UNet
    from gd_api_probe import DEEP_GALAXY_SPACE
    from torch import nn
    out = {}
    for kind, oc in (("fixed", 1), ("learned", 2)):
        torch.manual_seed(777)
        kw = dict(data_shape=[cfg["grid"]] * 3, in_channels=1, out_channels=oc, model_channels=cfg["mc"], num_res_blocks=2,
                  channel_mult=(1, 2, 4, 8), attention_resolutions=[16, 8], num_heads=4, use_scale_shift_norm=True, dims=3,
                  activation="SiLU", compute_dtype="bf16")
        extra = {}
        if cfg["labels"]:
            kw["num_classes"] = 25
            extra = dict(cond_fn="MultiEmbeddings", cond_fn_kwargs={"parameter_space": DEEP_GALAXY_SPACE, "embedding_dim": 4 * cfg["mc"]})
        pipe = GaussianDiffusionPipeline(UNet, kw, LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T, **extra)
        with torch.no_grad():
            for p in pipe.backbone.parameters():
                if float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
        if kind == "learned":
            pipe.model_var_type, pipe.loss_type = ModelVarType.LEARNED_RANGE, LossType.RESCALED_MSE
            pipe.model_mean_type = ModelMeanType.START_X
        pipe.log = lambda *a, **k: None
        out[kind] = pipe.to(dev).eval()
    return out


def timed(loops, reps):
    with torch.no_grad():
        for fn in loops.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in loops}
        for _ in range(reps):
            for k, fn in loops.items():
                times[k].append(event_ms(fn))
    return {k: statistics.median(v) for k, v in times.items()}


def probe(name, cfg, steps, reps, dev, train):
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    pipes = pipelines(cfg, steps, dev)
    B, G = cfg["batch"], cfg["grid"]
    shape = (B, 1, G, G, G)
    y = labels(B, dev) if cfg["labels"] else None
    kw = {"y": y} if y is not None else None
    x0 = (torch.rand(shape, device=dev) * 2 - 1).contiguous()
    res = {"config": name, "steps": steps, "reps": reps, "build": hip.lib().rho_build_info().decode(), "per_step_ms": {}}
    for kind, pipe in pipes.items():
        m = pipe.backbone
        tdev = torch.zeros(1, dtype=torch.int32, device=dev)
        cc = pipe._preembed_conditions(y) if y is not None else None
        loops = {
            "engine_forward": lambda: [m.engine().forward(x0, None, cc, t_scalar_dev=tdev) for _ in range(steps)],
            "reverse_process": lambda: pipe.reverse_process(torch.zeros(shape, device=dev), conditions=y),
            "p_sample_loop": lambda: pipe.p_sample_loop(m, shape, model_kwargs=kw),
            "ddim_sample_loop_eta0.5": lambda: pipe.ddim_sample_loop(m, shape, model_kwargs=kw, eta=0.5),
            "calc_bpd_loop": lambda: pipe.calc_bpd_loop(m, x0, model_kwargs=kw),
        }
        res["per_step_ms"][kind] = {k: round(v / steps, 4) for k, v in timed(loops, reps).items()}
    f, lr = res["per_step_ms"]["fixed"], res["per_step_ms"]["learned"]
    res["learned_minus_fixed_ms"] = {k: round(lr[k] - f[k], 4) for k in f}

    # the hybrid passes alone: fwd reads x_start, x_t, target and both halves (5 x 4 B / element); bwd the same + 2 writes
    pipe = pipes["learned"]
    n = x0.numel()
    xt, nz = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
    mo = torch.cat([torch.randn(shape, device=dev), torch.rand(shape, device=dev) * 2 - 1], dim=1).contiguous()
    t = torch.full((B,), steps // 2, dtype=torch.int64, device=dev)
    tab = pipe._tab(dev)
    ws = ops.gd_workspace(B, n // B, dev)
    gl = torch.full((B,), 1.0 / B, device=dev)
    kern = {
        "hybrid_loss_fwd": (lambda: ops.gd_hybrid_loss(x0, xt, nz, mo, t, tab, ops.GD_START_X, ops.GD_LEARNED_RANGE, 0.008, ws), 20 * n),
        "hybrid_loss_bwd": (lambda: ops.gd_hybrid_loss_bwd(x0, xt, nz, mo, t, tab, ops.GD_START_X, ops.GD_LEARNED_RANGE, 0.008, gl, None,
                                                           None), 28 * n),
        "gd_vlb_terms_lv": (lambda: ops.gd_vlb_terms(x0, xt, mo[:, :1], t, tab, ops.GD_START_X, None, None, torch.empty(B, device=dev),
                                                     workspace=ws, var_values=mo[:, 1:], var_type=ops.GD_LEARNED_RANGE), 16 * n),
    }
    res["kernel_us"], res["kernel_TBps"], res["kernel_GB"] = {}, {}, {}
    for k, (fn, nbytes) in kern.items():
        event_ms(fn, 5)
        ms = event_ms(fn, 50)
        res["kernel_us"][k] = round(ms * 1e3, 2)
        res["kernel_TBps"][k] = round(nbytes / (ms * 1e-3) / 1e12, 2)
        res["kernel_GB"][k] = round(nbytes / 1e9, 3)

    if train:
        data = (torch.rand(shape, device=dev) * 2 - 1).contiguous()
        tr = {}
        for kind, p in pipes.items():
            p.train()
            batch = [data, y] if y is not None else data

            def step(p=p, batch=batch):
                p.training_step(batch).backward()
            step()
            torch.cuda.synchronize()
            tr[kind] = statistics.median([event_ms(step, 3) for _ in range(reps)])
        res["train_step_ms"] = {"mse_fixed": round(tr["fixed"], 3), "hybrid_learned": round(tr["learned"], 3),
                                "delta": round(tr["learned"] - tr["fixed"], 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"], choices=sorted(PRESETS))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gd_learned_probe needs a GPU"
    os.makedirs(args.out, exist_ok=True)
    for name in args.configs:
        res = probe(name, PRESETS[name], args.steps, args.reps, "cuda:0", train=(name == "c3"))
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out, "gd_learned_probe.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
