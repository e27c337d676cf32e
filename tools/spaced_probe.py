"""Timing probe of few-step sampling on a spaced timestep sequence, quoted in DESIGN.md section 7 "Few-step sampling".  Not a
product path.

    python tools/spaced_probe.py [--num-steps 50] [--reps 3] [--no-chain] [--no-full] [--out DIR]        (DIR: $RHO_RUN_OUT, else runs/)

1. The update alone at the c3 sample size (32 x 1 x 64^3 floats): rho_p_sample_step_spaced in its four forms - plain and guided,
   eta = 0 (z is not read) and eta > 0 - next to rho_p_sample_step, the full loop's update, in the same run.  HIP events around each
   call, the candidates alternated call by call in this one process, the device kept busy by a spin kernel while the host
   queues the timed calls, median of --iters after --warmup.  Bytes are the algorithmic
   ones, 4 per float: plain 3n / 4n (x and the prediction read, z with eta > 0, x written), guided 5n / 6n (two predictions read,
   both rows written), rho_p_sample_step 4n (t = 500: z is used).  Row k = 24 of a 50-step table: an ordinary row, clip on.  Two
   more forms of the plain update move the same bytes with less arithmetic per element (clip off; row 0, which writes the x0
   estimate): they separate the cost of the longer expression from the cost of the bytes.
2. One c3 reverse_process (bf16 engine, batch 32, LinearSchedule(1000)) with num_steps = --num-steps against the full chain of 1000
   steps, wall time of each call ending in a synchronise; the few-step chain --reps times (median), the full chain once.

Prints one JSON line and writes it to DIR/spaced_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

N_C3 = 32 * 64 ** 3


def timed(fns, iters: int, warmup: int, plug_ms: float = 40.0):
    """Median device time in microseconds of each fn, the fns alternated call by call (one event pair per call)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    # keep the device busy while the host queues the timed calls: with an idle device an event pair also spans the host time
    # between its two records (the wrapper's argument checks), which differs from candidate to candidate
    torch.cuda._sleep(int(plug_ms * 2.0e6))
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            pairs[k].append((a, b))
    torch.cuda.synchronize()
    return [statistics.median(a.elapsed_time(b) * 1e3 for a, b in p) for p in pairs]


def update_rows(n: int, iters: int, warmup: int, dev):
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients, spaced_timesteps
    from rho_diffusion_amd.engine import ops
    sched = LinearSchedule(1000, 1e-3, 0.02)
    taus = spaced_timesteps(1000, 50)
    rows0 = spaced_coefficients(sched["alpha_bar_t"], taus, 0.0).to(dev)
    rows1 = spaced_coefficients(sched["alpha_bar_t"], taus, 1.0).to(dev)
    coef = sched.device_tables(dev)["coef"]
    k_dev = torch.full((1,), 24, dtype=torch.int32, device=dev)
    k0_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    t_dev = torch.full((1,), 500, dtype=torch.int32, device=dev)
    x2 = torch.randn(2 * n, device=dev) * 0.5
    e2, z = torch.randn(2 * n, device=dev), torch.randn(n, device=dev)
    xa, ec = x2[:n], e2[:n]
    s = 3.0
    cands = [("rho_p_sample_step_spaced plain, eta = 0", 3, lambda: ops.p_sample_step_spaced(xa, ec, None, rows0, k_dev)),
             ("rho_p_sample_step_spaced plain, eta > 0", 4, lambda: ops.p_sample_step_spaced(xa, ec, z, rows1, k_dev)),
             ("rho_p_sample_step_spaced guided, eta = 0", 5, lambda: ops.p_sample_step_spaced(x2, e2, None, rows0, k_dev, s)),
             ("rho_p_sample_step_spaced guided, eta > 0", 6, lambda: ops.p_sample_step_spaced(x2, e2, z, rows1, k_dev, s)),
             ("rho_p_sample_step", 4, lambda: ops.p_sample_step(xa, ec, z, coef, t_dev)),
             # the same bytes with less arithmetic per element: where the difference to rho_p_sample_step comes from
             ("rho_p_sample_step_spaced plain, eta > 0, clip off", 4, lambda: ops.p_sample_step_spaced(xa, ec, z, rows1, k_dev, clip=False)),
             ("rho_p_sample_step_spaced plain, row 0 (x0 only)", 3, lambda: ops.p_sample_step_spaced(xa, ec, None, rows0, k0_dev))]
    us = timed([c[2] for c in cands], iters, warmup)
    return [{"what": w, "floats_per_elem": f, "MB": round(4 * f * n * 1e-6, 1), "us": round(u, 1), "GBps": round(4 * f * n / u * 1e-3, 1)}
            for (w, f, _), u in zip(cands, us)]


def chain_rows(num_steps: int, reps: int, full: bool, dev):
    """Wall seconds of reverse_process at the c3 configuration: num_steps of the 1000 timesteps against all of them."""
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    torch.manual_seed(777)
    G, mc, B = 64, 64, 32
    kw = dict(data_shape=[G] * 3, in_channels=1, out_channels=1, model_channels=mc, num_res_blocks=2, channel_mult=(1, 2, 4, 8),
              attention_resolutions=[16, 8], num_heads=4, use_scale_shift_norm=True, dims=3, activation="SiLU", compute_dtype="bf16")
    ddpm = DDPM(UNet, kw, LinearSchedule(1000, 1e-3, 0.02), nn.MSELoss, timesteps=1000)
    with torch.no_grad():
        for p in ddpm.backbone.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02)
    ddpm = ddpm.to(dev).eval()
    x = torch.zeros(B, 1, G, G, G, device=dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    wall(lambda: ddpm.reverse_process(x, num_steps=3))                    # warm-up: engine plan, code objects
    few = [wall(lambda: ddpm.reverse_process(x, num_steps=num_steps)) for _ in range(reps)]
    out = {"num_steps": num_steps, "reps": reps, "hip_graph": bool(ddpm.hip_graph_sampling),
           "few_step_s": round(statistics.median(few), 3), "few_step_s_all": [round(v, 3) for v in few],
           "few_step_ms_per_step": round(statistics.median(few) / num_steps * 1e3, 2)}
    if full:
        t_full = wall(lambda: ddpm.reverse_process(x))
        out.update({"full_chain_steps": 1000, "full_chain_s": round(t_full, 3), "full_chain_ms_per_step": round(t_full / 1000 * 1e3, 2),
                    "speedup": round(t_full / statistics.median(few), 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--num-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-chain", action="store_true", help="the update kernels only")
    ap.add_argument("--no-full", action="store_true", help="skip the full chain of 1000 steps (about two minutes)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spaced_probe needs the GPU: nothing is measured without one")
    from rho_diffusion_amd import hip
    dev = "cuda"
    res = {"build": hip.load().rho_build_info().decode(), "iters": args.iters, "n": N_C3,
           "update": update_rows(N_C3, args.iters, args.warmup, dev)}
    if not args.no_chain:
        res["chain_c3"] = chain_rows(args.num_steps, args.reps, not args.no_full, dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "spaced_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
