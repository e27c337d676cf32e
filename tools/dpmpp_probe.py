"""Timing probe of the DPM-Solver++(2M) update (rho_dpmpp_2m_step) against the DDIM update it replaces on the spaced walk
(rho_p_sample_step_spaced with eta = 0), quoted in DESIGN.md section 7 "DPM-Solver++(2M)".  Not a product path.

    python tools/dpmpp_probe.py [--n 8388608] [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

Operands of n float32 (default: the c3 sampling size, 32 x 64^3), the same x and pred for every variant.  HIP events around each
call, median of --iters calls after --warmup, the variants alternated call by call in this one process: rho_p_sample_step_spaced
plain and guided, and rho_dpmpp_2m_step for epsilon and v, plain and guided, on a second-order row (k = S / 2 of 50 log-SNR spaced
timesteps of LinearSchedule(1000)), clip on so that x stays bounded over the repeated in-place calls.  TB/s over the algorithmic
bytes: the DDIM update reads x and pred and writes x (12 n; guided 20 n: two rows of pred read, two rows of x written), the 2M
update also reads and writes hist (20 n; guided 28 n).  Prints one JSON line and writes it to DIR/dpmpp_probe.json."""
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
    ap.add_argument("--n", type=int, default=32 * 64 ** 3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT") or os.path.join(ROOT, "runs"))
    args = ap.parse_args()

    from rho_diffusion_amd import hip
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients, logsnr_timesteps
    from rho_diffusion_amd.diffusion.prediction import PREDICTION_TYPES
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients
    lib, st = hip.load(), hip.stream
    dev = "cuda:0"
    n, S = args.n, args.steps
    k = S // 2
    gen = torch.Generator(device=dev).manual_seed(7)
    x2 = torch.randn(2 * n, device=dev, generator=gen)                        # plain calls use the first row
    pred2 = torch.randn(2 * n, device=dev, generator=gen)
    hist = torch.randn(n, device=dev, generator=gen)
    ab = LinearSchedule(1000)["alpha_bar_t"].float()
    taus = logsnr_timesteps(ab, S)
    k_dev = torch.tensor([k], dtype=torch.int32, device=dev)
    ddim_rows = spaced_coefficients(ab, taus, 0.0).contiguous().to(dev)
    rows = {kind: dpmpp_2m_coefficients(ab, taus, kind).contiguous().to(dev) for kind in ("epsilon", "v")}
    assert all(float(r[k, 4]) != 0.0 for r in rows.values())                  # a second-order row: hist is read

    def ddim(guided):
        def fn():
            hip.check(lib.rho_p_sample_step_spaced(x2.data_ptr(), pred2.data_ptr(), None, ddim_rows.data_ptr(), k_dev.data_ptr(), S, n,
                                                   guided, 3.0, 1, st()), "rho_p_sample_step_spaced")
        return fn

    def dpmpp(kind, guided):
        r, code = rows[kind], PREDICTION_TYPES[kind]

        def fn():
            hip.check(lib.rho_dpmpp_2m_step(x2.data_ptr(), pred2.data_ptr(), hist.data_ptr(), r.data_ptr(), k_dev.data_ptr(), S, n, guided,
                                            3.0, 1, code, st()), "rho_dpmpp_2m_step")
        return fn

    labels = ["rho_p_sample_step_spaced eta=0", "rho_p_sample_step_spaced eta=0 guided"]
    fns, nbytes, base = [ddim(0), ddim(1)], [12.0 * n, 20.0 * n], [0, 1]
    for kind in ("epsilon", "v"):
        for guided in (0, 1):
            labels.append(f"rho_dpmpp_2m_step {kind}{' guided' if guided else ''}")
            fns.append(dpmpp(kind, guided))
            nbytes.append((28.0 if guided else 20.0) * n)
            base.append(guided)
    us = timed(fns, args.iters, args.warmup)
    out_rows = [{"kernel": lb, "us": round(u, 2), "bytes": b, "TBps": round(b / (u * 1e-6) / 1e12, 3), "vs_ddim": round(u / us[g], 3),
                 "bytes_vs_ddim": round(b / nbytes[g], 3)} for lb, u, b, g in zip(labels, us, nbytes, base)]
    result = {"probe": "dpmpp", "n": n, "S": S, "k": k, "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "build": lib.rho_build_info().decode(), "rows": out_rows}
    line = json.dumps(result)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dpmpp_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
