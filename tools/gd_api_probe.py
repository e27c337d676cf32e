"""Per-step cost of GaussianDiffusionPipeline's sampling / likelihood loops and of the csrc/gaussian.hip kernels on their own.

    python tools/gd_api_probe.py [--configs c3 c5] [--steps 8] [--reps 3] [--out DIR]

For each bench geometry (c3: bf16 3-D 64^3, mc 64, B 32; c5: bf16 3-D 128^3, mc 32, B 2, labels): the per-step time of
reverse_process, p_sample_loop, ddim_sample_loop(eta=0.5) and calc_bpd_loop (HIP events around whole loops of ``--steps`` steps
after a warm-up loop, median of ``--reps``, loops alternated), and the isolated kernels (HIP events around 50 launches after 5):
rho_abs_quantile, rho_ddim_step, rho_gd_posterior_step, rho_gd_ddim_step, rho_gd_vlb_terms with the bytes each must move.
One JSON line per configuration on stdout (and in DIR/gd_api_probe.jsonl)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {"c3": dict(grid=64, mc=64, batch=32, labels=False), "c5": dict(grid=128, mc=32, batch=2, labels=True)}
DEEP_GALAXY_SPACE = {"s": [0.25, 0.5, 0.75, 1, 1.25, 1.5], "m": [0.25, 0.5, 0.75, 1, 1.25, 1.5],
                     "t": list(range(300, 655, 5)), "c": list(range(14))}


def pipeline(cfg, T, dev):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.models import UNet
    torch.manual_seed(777)
    kw = dict(data_shape=[cfg["grid"]] * 3, in_channels=1, out_channels=1, model_channels=cfg["mc"], num_res_blocks=2,
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
    return pipe.to(dev).eval()


def labels(B, dev):
    keys = list(DEEP_GALAXY_SPACE)
    rows = [[float(DEEP_GALAXY_SPACE[k][(3 * i + 5 * j + 1) % len(DEEP_GALAXY_SPACE[k])]) for j, k in enumerate(keys)] for i in range(B)]
    return torch.tensor(rows, dtype=torch.float32, device=dev)


def event_ms(fn, n=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def probe(name, cfg, steps, reps, dev):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd import hip
    pipe = pipeline(cfg, steps, dev)
    B, G = cfg["batch"], cfg["grid"]
    shape = (B, 1, G, G, G)
    y = labels(B, dev) if cfg["labels"] else None
    kw = {"y": y} if y is not None else None
    x0 = (torch.rand(shape, device=dev) * 2 - 1).contiguous()
    m = pipe.backbone
    loops = {
        "reverse_process": lambda: pipe.reverse_process(torch.zeros(shape, device=dev), conditions=y),
        "p_sample_loop": lambda: pipe.p_sample_loop(m, shape, model_kwargs=kw),
        "ddim_sample_loop_eta0.5": lambda: pipe.ddim_sample_loop(m, shape, model_kwargs=kw, eta=0.5),
        "calc_bpd_loop": lambda: pipe.calc_bpd_loop(m, x0, model_kwargs=kw),
    }
    with torch.no_grad():
        for fn in loops.values():                               # warm-up: engine plans, workspaces, code objects
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in loops}
        for _ in range(reps):
            for k, fn in loops.items():
                times[k].append(event_ms(fn) / steps)
    res = {"config": name, "steps": steps, "reps": reps, "build": hip.lib().rho_build_info().decode(),
           "per_step_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
           "per_step_ms_all": {k: [round(x, 4) for x in v] for k, v in times.items()}}
    rp = res["per_step_ms"]["reverse_process"]
    res["vs_reverse_process_pct"] = {k: round(100.0 * (v / rp - 1.0), 2) for k, v in res["per_step_ms"].items()}

    # isolated kernels on the geometry, fp32 tensors as the loops hand them over
    n = x0.numel()
    xt, mo, nz = torch.randn(shape, device=dev), torch.randn(shape, device=dev) * 2, torch.randn(shape, device=dev)
    t = torch.full((B,), steps // 2, dtype=torch.int64, device=dev)
    tab = pipe._gd_table(dev)
    q = pipe._quantile(mo)
    out, px = torch.empty_like(xt), torch.empty_like(xt)
    vb = torch.empty(B, device=dev)
    ws = ops.gd_workspace(B, n // B, dev)
    c = pipe.ddim_coefficients(steps // 2, 0.0)
    kern = {
        "abs_quantile": (lambda: pipe._quantile(mo), 4 * n),
        "ddim_step_host_scalars": (lambda: ops.ddim_step(xt, mo, q, None, out, None, *c), 12 * n),
        "gd_posterior_step_noise": (lambda: ops.gd_posterior_step(xt, mo, t, tab, ops.GD_START_X, q, None, nz, out, px), 20 * n),
        "gd_ddim_step_eta": (lambda: ops.gd_ddim_step(xt, mo, t, tab, ops.GD_START_X, q, None, nz, 0.5, False, out, None), 16 * n),
        "gd_vlb_terms": (lambda: ops.gd_vlb_terms(x0, xt, mo, t, tab, ops.GD_START_X, q, nz, vb, workspace=ws), 16 * n),
    }
    res["kernel_us"], res["kernel_TBps"] = {}, {}
    for k, (fn, nbytes) in kern.items():
        event_ms(fn, 5)
        ms = event_ms(fn, 50)
        res["kernel_us"][k] = round(ms * 1e3, 2)
        res["kernel_TBps"][k] = round(nbytes / (ms * 1e-3) / 1e12, 2)
    res["bytes_note"] = "bytes the kernel must move: quantile 4 reads of x (upper bound); ddim_step 2 reads + 1 write; " \
                        "posterior 3 reads + 2 writes; ddim eta 3 reads + 1 write; vlb 4 reads (x_start, x_t, model out, noise)"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"], choices=sorted(PRESETS))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gd_api_probe needs a GPU"
    os.makedirs(args.out, exist_ok=True)
    for name in args.configs:
        res = probe(name, PRESETS[name], args.steps, args.reps, "cuda:0")
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(args.out, "gd_api_probe.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
