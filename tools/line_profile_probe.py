"""Timing probe of SpectroscopyDataset's device path (rho_line_profile), quoted in DESIGN.md "Spectra on the device".

    python tools/line_profile_probe.py [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

HIP events around each call, median of --iters launches after --warmup: ``ops.line_profile`` alone (memset, profile launch,
normalise launch) at batch 64 and 1024 on the default 50 000-point grid with 600 and with 3000 lines per item, and the fraction of
(line, grid point) pairs the windowing evaluates; ``ds.batch(64)`` (the whole API call: permutation slice, width draw, kernels,
gathers) from a file of --rows items with 600 lines; and the host path as the reference computes it (numpy, float32 differences,
float64 [lines, grid] temporary, exp, sum, division by the maximum, H2D copy; host clock) for the same 64 items at 600 lines and
for --host-items items at 3000 lines.  Prints one JSON line and writes it to DIR/line_profile_probe.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_median(fn, iters: int, warmup: int) -> float:
    """Median device time of fn() in microseconds (one event pair per call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in pairs)


def reference_item(grid, centers, log_intensity, width):
    """spectroscopy.py:117-134 for one item on the host."""
    inten = 10 ** np.clip(log_intensity, -10.0, -2.0)
    width = np.array([width])
    mask = np.all([centers <= grid.max(), grid.min() <= centers], axis=0)
    profile = inten[mask, None] * np.exp(-((grid[None, :] - centers[mask, None]) ** 2.0) / (2 * width[:, None] ** 2.0))
    profile = profile.sum(axis=0)
    profile /= profile.max()
    return torch.Tensor(profile)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-items", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU"
    from rho_diffusion_amd import h5io
    from rho_diffusion_amd.data import SpectroscopyDataset
    from rho_diffusion_amd.data.spectroscopy import pack_lines
    from rho_diffusion_amd.engine import ops
    dev = "cuda"
    N, G = args.rows, 50_000
    rng = np.random.default_rng(0)
    grid_np = np.linspace(1000, 32000, G, dtype=np.float32)
    grid = torch.from_numpy(grid_np).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {"rows": N, "grid_size": G}
    sets = {}
    for C in (600, 3000):
        trans = [np.stack([rng.uniform(1000.0, 32000.0, C), rng.uniform(-7.0, -2.0, C)]).astype(np.float32) for _ in range(N)]
        centers, intensity, offsets, _ = pack_lines(trans)
        sets[C] = (trans, torch.from_numpy(centers).to(dev), torch.from_numpy(intensity).to(dev), torch.from_numpy(offsets).to(dev))
    # 1. the kernel alone
    for C, (_, centers, intensity, offsets) in sets.items():
        for B in (64, 1024):
            idx = torch.randint(0, N, (B,), device=dev)
            widths = (1.0 + 0.1 * torch.randn(B, device=dev)).abs()
            out = torch.empty(B, G, device=dev)
            fn = lambda: ops.line_profile(grid, centers, intensity, offsets, idx, widths, out=out, err_flag=flag)      # noqa: E731
            t = event_median(fn, args.iters if B == 64 else max(args.iters // 4, 20), args.warmup)
            res[f"lines{C}_batch{B}_us"] = t
            res[f"lines{C}_batch{B}_us_per_item"] = t / B
    ops.line_profile_check(flag)
    # the share of (line, point) pairs inside a wave's reach of 13.25 w: 256-point segments of 0.62 MHz
    seg = 256 * float(grid_np[1] - grid_np[0])
    res["pairs_evaluated_fraction_w1"] = (seg + 2 * 13.25) / 31000.0
    # 2. ds.batch(64) and the host path for the same items, 600 lines
    trans600 = sets[600][0]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "spectra.h5")
        arrays = {}
        for i, t in enumerate(trans600):
            arrays[f"{i}/transitions"] = t
            arrays[f"{i}/constants"] = np.array([float(i), 1.0, 2.0])
        h5io.write(path, arrays)
        t0 = time.perf_counter()
        ds = SpectroscopyDataset(path)
        res["load_s"] = time.perf_counter() - t0
    res["batch64_api_us"] = event_median(lambda: ds.batch(64), args.iters, args.warmup)
    ds.check_errors()
    rows64 = torch.randperm(N)[:64].tolist()
    w64 = [abs(float(w)) for w in rng.normal(1.0, 0.1, 64)]
    t0 = time.perf_counter()
    host = torch.stack([reference_item(grid_np, trans600[i][0], trans600[i][1], w) for i, w in zip(rows64, w64)]).to(dev)
    torch.cuda.synchronize()
    res["host_path64_lines600_s"] = time.perf_counter() - t0
    got = ds.batch(rows64, widths=w64)["spectrum"]
    res["host_vs_device_max_abs"] = float((got - host).abs().max())
    # 3. the host path at 3000 lines, per item
    trans3k = sets[3000][0]
    ts = []
    for i in range(args.host_items):
        t0 = time.perf_counter()
        reference_item(grid_np, trans3k[i][0], trans3k[i][1], 1.0)
        ts.append(time.perf_counter() - t0)
    res["host_path_item_lines3000_s"] = statistics.median(ts)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "line_profile_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
