"""Timing probe of the prediction-type training loss (rho_pred_loss_ws) against rho_mse_ws, quoted in DESIGN.md section 7
"Prediction types and min-SNR weighting".  Not a product path.

    python tools/pred_loss_probe.py [--batch 32] [--per-sample 262144] [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

Operands of batch x per-sample float32 (default: the c3 training size, 32 x 64^3).  HIP events around each call (the partial-sum
launch and the one-wave final launch together), median of --iters calls after --warmup, the variants alternated call by call in
this one process: rho_mse_ws with its gradient, and rho_pred_loss_ws for epsilon / v / sample with the min-SNR table and with
w == NULL.  TB/s over the algorithmic bytes: rho_mse_ws reads 2 n floats and writes n, rho_pred_loss_ws reads 3 n and writes n.
Prints one JSON line and writes it to DIR/pred_loss_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--per-sample", type=int, default=64 ** 3)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT") or os.path.join(ROOT, "runs"))
    args = ap.parse_args()

    from rho_diffusion_amd import hip
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.prediction import PREDICTION_TYPES, min_snr_weights
    lib, st = hip.load(), hip.stream
    dev = "cuda:0"
    B, P, T = args.batch, args.per_sample, args.timesteps
    n = B * P
    gen = torch.Generator(device=dev).manual_seed(7)
    pred, x0, eps = (torch.randn(n, device=dev, generator=gen) for _ in range(3))
    grad = torch.empty(n, device=dev)
    t = torch.randint(0, T, (B,), device=dev, generator=gen)
    ab = LinearSchedule(T, 1e-3, 0.02)["alpha_bar_t"].float().contiguous()
    ab_d = ab.to(dev)
    out = torch.zeros(1 + 1024, device=dev)
    loss_p, part_p = out.data_ptr(), out.data_ptr() + 4

    def mse():
        hip.check(lib.rho_mse_ws(pred.data_ptr(), eps.data_ptr(), loss_p, grad.data_ptr(), n, part_p, 1024, st()), "rho_mse_ws")

    def pred_loss(code, w):
        def fn():
            hip.check(lib.rho_pred_loss_ws(pred.data_ptr(), x0.data_ptr(), eps.data_ptr(), ab_d.data_ptr(), w.data_ptr() if w is not None else None,
                                           t.data_ptr(), B, P, T, code, loss_p, grad.data_ptr(), part_p, 1024, None, st()), "rho_pred_loss_ws")
        return fn

    labels, fns, nbytes = ["rho_mse_ws"], [mse], [12.0 * n]
    tables = []
    for kind, code in PREDICTION_TYPES.items():
        w = min_snr_weights(ab, kind, 5.0).to(dev)
        tables.append(w)
        for name, tab in ((f"rho_pred_loss_ws {kind} min-SNR", w), (f"rho_pred_loss_ws {kind} w=NULL", None)):
            labels.append(name)
            fns.append(pred_loss(code, tab))
            nbytes.append(16.0 * n)
    us = timed(fns, args.iters, args.warmup)
    rows = [{"kernel": lb, "us": round(u, 2), "bytes": b, "TBps": round(b / (u * 1e-6) / 1e12, 3), "vs_mse": round(u / us[0], 3)}
            for lb, u, b in zip(labels, us, nbytes)]
    result = {"probe": "pred_loss", "batch": B, "per_sample": P, "n": n, "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "build": lib.rho_build_info().decode(), "rows": rows}
    line = json.dumps(result)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "pred_loss_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
