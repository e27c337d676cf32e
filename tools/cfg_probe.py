"""Timing probe of guided sampling (classifier-free guidance), quoted in DESIGN.md section 7 "Classifier-free guidance".  Not a
product path.

    python tools/cfg_probe.py [--steps 16] [--reps 5] [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

1. The guided update alone, at the element counts of c3 (32 x 64^3) and c5 (2 x 128^3): rho_p_sample_step_cfg against
   rho_p_sample_step (the unguided update it extends) and against the torch formulation it replaces - combine the two predictions,
   rho_p_sample_step, copy the result into the second half - with the combine as one torch.lerp and as the two-op expression
   e_u + s * (e_c - e_u).  HIP events around each call, the candidates alternated call by call in this one process, median of --iters
   after --warmup.  Bytes are the algorithmic ones, 4 per float: fused 6n (x, e_c, e_u, z read; both rows written), unguided 4n,
   torch + lerp 9n (3n + 4n + 2n), torch two-op 12n (3n + 3n + 4n + 2n).  t = 500: z is used.
2. One reverse_process of --steps steps at c5 shapes: guided at batch 2 (the engine runs at batch 4) next to unguided at batch 4,
   alternated --reps times, per-step milliseconds.

Prints one JSON line and writes it to DIR/cfg_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

SIZES = {"c3": 32 * 64 ** 3, "c5": 2 * 128 ** 3}
HBM_PEAK_TBPS = 8.0
DEEP_GALAXY_SPACE = {"s": [0.25, 0.5, 0.75, 1, 1.25, 1.5], "m": [0.25, 0.5, 0.75, 1, 1.25, 1.5],
                     "t": list(range(300, 655, 5)), "c": list(range(14))}


def timed(fns, iters: int, warmup: int):
    """Median device time in microseconds of each fn, the fns alternated call by call (one event pair per call)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs[k].append((a, b))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in p) for p in pairs]


def step_rows(n: int, iters: int, warmup: int, dev):
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.engine import ops
    coef = LinearSchedule(1000, 1e-3, 0.02).device_tables(dev)["coef"]
    t_dev = torch.full((1,), 500, dtype=torch.int32, device=dev)
    x2 = torch.randn(2 * n, device=dev) * 0.5
    e2, z, g = torch.randn(2 * n, device=dev), torch.randn(n, device=dev), torch.empty(n, device=dev)
    xa, xb, ec, eu = x2[:n], x2[n:], e2[:n], e2[n:]
    s = 3.0

    def fused():
        ops.p_sample_step_cfg(x2, e2, z, coef, t_dev, s)

    def unguided():
        ops.p_sample_step(xa, ec, z, coef, t_dev)

    def torch_lerp():
        torch.lerp(eu, ec, s, out=g)
        ops.p_sample_step(xa, g, z, coef, t_dev)
        xb.copy_(xa)

    def torch_two_op():
        torch.sub(ec, eu, out=g)
        torch.add(eu, g, alpha=s, out=g)
        ops.p_sample_step(xa, g, z, coef, t_dev)
        xb.copy_(xa)

    names = [("rho_p_sample_step_cfg", 6), ("rho_p_sample_step", 4), ("torch lerp + step + copy", 9), ("torch sub, add + step + copy", 12)]
    us = timed([fused, unguided, torch_lerp, torch_two_op], iters, warmup)
    return [{"what": w, "floats_per_elem": f, "MB": round(4 * f * n * 1e-6, 1), "us": round(u, 1), "TBps": round(4 * f * n / u * 1e-6, 2),
             "frac_of_hbm_peak": round(4 * f * n / u * 1e-6 / HBM_PEAK_TBPS, 3)} for (w, f), u in zip(names, us)]


def labels(B, dev):
    keys = list(DEEP_GALAXY_SPACE)
    rows = [[float(DEEP_GALAXY_SPACE[k][(3 * i + 5 * j + 1) % len(DEEP_GALAXY_SPACE[k])]) for j, k in enumerate(keys)] for i in range(B)]
    return torch.tensor(rows, dtype=torch.float32, device=dev)


def chain_rows(steps: int, reps: int, dev):
    """Per-step ms of reverse_process at c5 shapes: guided at batch B = 2 against unguided at batch 2B = 4."""
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    torch.manual_seed(777)
    G, mc, B = 128, 32, 2
    kw = dict(data_shape=[G] * 3, in_channels=1, out_channels=1, model_channels=mc, num_res_blocks=2, channel_mult=(1, 2, 4, 8),
              attention_resolutions=[16, 8], num_heads=4, use_scale_shift_norm=True, dims=3, activation="SiLU", compute_dtype="bf16",
              num_classes=25)
    ddpm = DDPM(UNet, kw, LinearSchedule(steps, 1e-3, 0.02), nn.MSELoss, timesteps=steps, cond_fn="MultiEmbeddings",
                cond_fn_kwargs={"parameter_space": DEEP_GALAXY_SPACE, "embedding_dim": 4 * mc})
    with torch.no_grad():
        for p in ddpm.backbone.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02)
    ddpm = ddpm.to(dev).eval()
    y2, y4 = labels(B, dev), labels(2 * B, dev)
    z2, z4 = torch.zeros(B, 1, G, G, G, device=dev), torch.zeros(2 * B, 1, G, G, G, device=dev)
    runs = {"guided_batch2": lambda: ddpm.reverse_process(z2, y2, guidance_scale=3.0),
            "unguided_batch4": lambda: ddpm.reverse_process(z4, y4)}
    for fn in runs.values():                                     # warm-up: engine plans, code objects
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / steps)
    return {"steps": steps, "reps": reps, "hip_graph": bool(ddpm.hip_graph_sampling),
            "per_step_ms": {k: round(statistics.median(v), 3) for k, v in ms.items()},
            "per_step_ms_all": {k: [round(x, 3) for x in v] for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true", help="the update kernels only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cfg_probe needs the GPU: nothing is measured without one")
    from rho_diffusion_amd import hip
    dev = "cuda"
    res = {"build": hip.load().rho_build_info().decode(), "iters": args.iters,
           "update": {name: {"n": n, "rows": step_rows(n, args.iters, args.warmup, dev)} for name, n in SIZES.items()}}
    if not args.no_chain:
        res["chain_c5"] = chain_rows(args.steps, args.reps, dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "cfg_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
