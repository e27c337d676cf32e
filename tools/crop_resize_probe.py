"""Timing probe of DeepGalaxyDataset's device transform (rho_crop_resize), quoted in DESIGN.md "DeepGalaxy images on the device".

    python tools/crop_resize_probe.py [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

HIP events around each call, median of --iters launches after --warmup: ``batch(64)`` from a resident 512^2 uint8 set with the default
transform (the whole API call: permutation slice, kernel, label gather) and the kernel alone; the kernel at batch 1024 with its
effective bandwidth (bytes of the crop windows read + float32 output written, over the kernel time); the reference-style host path
for the same 64 items (float32 rows resident on the host, per-item crop + F.interpolate(antialias=True) + 2 t - 1 on 16 threads,
stack, H2D copy; host clock around a device synchronise); and one training step of the example config's model (UNetv2 2-D 128^2,
mc 32, num_classes 25, MultiEmbeddings(128), batch 64) fed by ``batch(64)`` against the same step fed by a resident batch,
alternated.  Prints one JSON line and writes it to DIR/crop_resize_probe.json."""
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
import torch.nn.functional as F  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--train-steps", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU"
    from rho_diffusion_amd import h5io
    from rho_diffusion_amd.data import DeepGalaxyDataset
    from rho_diffusion_amd.engine import ops
    dev = "cuda"
    N, S = args.rows, 512
    rng = np.random.default_rng(0)
    half = N // 2
    arrays = {}
    for g, (s, m) in enumerate([(0.5, 1.0), (1.25, 0.25)]):
        arrays[f"s_{s}_m_{m}/images_camera_00"] = rng.integers(0, 256, size=(half, S, S, 1), dtype=np.uint8)
        arrays[f"s_{s}_m_{m}/t_myr_camera_00"] = np.asarray([300.0 + 5 * (i % 71) for i in range(half)])
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "dg.h5")
        h5io.write(path, arrays)
        ds = DeepGalaxyDataset(path, use_emb_as_labels=False, camera_pos=[0])
    assert ds.raw.dtype == torch.uint8 and len(ds) == N
    res["rows"], res["image"] = N, [S, S, 1]
    # 1. batch(64), whole API call and kernel alone
    res["batch64_api_us"] = event_median(lambda: ds.batch(64), args.iters, args.warmup)
    idx64 = torch.randperm(N, device=dev)[:64].contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ds.batch(1)
    out64 = torch.empty(64, 1, 128, 128, device=dev)
    k64 = lambda: ops.crop_resize(ds.raw, ds.rowmax, idx64, 256, (128, 128), True, taps=ds._taps, out=out64, err_flag=flag)  # noqa: E731
    res["batch64_kernel_us"] = event_median(k64, args.iters, args.warmup)
    # 2. batch 1024 (rows repeat), effective bandwidth
    idx1k = torch.randint(0, N, (1024,), device=dev)
    out1k = torch.empty(1024, 1, 128, 128, device=dev)
    k1k = lambda: ops.crop_resize(ds.raw, ds.rowmax, idx1k, 256, (128, 128), True, taps=ds._taps, out=out1k, err_flag=flag)  # noqa: E731
    t1k = event_median(k1k, max(args.iters // 3, 100), args.warmup)
    moved = 1024 * (256 * 256 * 1 + 128 * 128 * 4)
    res["batch1024_kernel_us"] = t1k
    res["batch1024_bytes"] = moved
    res["batch1024_GBps"] = moved / (t1k * 1e-6) / 1e9
    ops.crop_resize_check(flag)
    # 3. the reference-style host path for the same 64 items
    torch.set_num_threads(16)
    host = (ds.raw.cpu().to(torch.float64) / ds.rowmax.cpu().view(-1, 1, 1, 1)).to(torch.float32).permute(0, 3, 2, 1).contiguous()
    rows64 = idx64.cpu().tolist()

    def host_batch():
        items = []
        for i in rows64:
            x = host[i][:, 128:384, 128:384]
            x = F.interpolate(x[None], size=[128, 128], mode="bilinear", align_corners=False, antialias=True)[0]
            items.append(x * 2 - 1)
        out = torch.stack(items).to(dev)
        torch.cuda.synchronize()
        return out

    assert float((host_batch() - k64()).abs().max()) <= 2e-6
    for _ in range(3):
        host_batch()
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        host_batch()
        ts.append((time.perf_counter() - t0) * 1e6)
    res["host_path64_us"] = statistics.median(ts)
    # 4. one training step fed by the dataset vs by a resident batch
    from torch import nn
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    from rho_diffusion_amd.optim import HipAdamW
    torch.manual_seed(777)
    kw = dict(dims=2, in_channels=1, out_channels=1, model_channels=32, num_res_blocks=2, data_shape=[128, 128],
              attention_resolutions=[16, 8], use_scale_shift_norm=True, num_heads=4, num_classes=25, activation="SiLU",
              use_new_attention_order=False)
    ddpm = DDPM(UNet, kw, LinearSchedule(500), nn.MSELoss, timesteps=500, cond_fn="MultiEmbeddings",
                cond_fn_kwargs={"parameter_space": ds.parameter_space, "embedding_dim": 128}).to(dev)
    opt = HipAdamW(ddpm.parameters(), lr=1e-4)
    pool_x, pool_y = ds.batch(64)
    pool_x, pool_y = pool_x.clone(), pool_y.clone()

    def step(feed):
        x, y = ds.batch(64) if feed == "dataset" else (pool_x, pool_y)
        opt.zero_grad()
        loss = ddpm.training_step([x, y])
        loss.backward()
        opt.step()

    times = {"dataset": [], "pool": []}
    for _ in range(3):
        step("dataset")
        step("pool")
    torch.cuda.synchronize()
    for _ in range(args.train_steps):
        for feed in ("dataset", "pool"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(feed)
            b.record()
            torch.cuda.synchronize()
            times[feed].append(a.elapsed_time(b))
    res["train_step_dataset_ms"] = statistics.median(times["dataset"])
    res["train_step_pool_ms"] = statistics.median(times["pool"])
    res["train_step_spread_ms"] = {k: [min(v), max(v)] for k, v in times.items()}
    ds.check_errors()
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "crop_resize_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
