"""Timing probe of MNISTDataset / CIFAR10Dataset's device transform (rho_u8_image_batch), quoted in DESIGN.md "MNIST / CIFAR-10 on the
device".

    python tools/u8_image_probe.py [--out DIR]            (DIR: $RHO_RUN_OUT, else runs/)

HIP events around each call, median of --iters launches after --warmup, for both geometries with the full training sets resident
(MNIST: 60 000 rows of 28 x 28 x 1 resized to 32 x 32; CIFAR-10: 50 000 rows of 32 x 32 x 3, no resize; random bytes, written as
fixture files and loaded through the datasets): the kernel alone at batch 64 and at a large batch with its effective bandwidth (item
bytes read + float32 output written, over the kernel time) and the time those bytes would take at 8 TB/s; ``ds.batch(64)`` (the whole
API call: permutation slice, kernel, label gather); and the reference-style host path for the same 64 items (per item a PIL.Image,
Image.resize(BILINEAR) for MNIST, ToTensor's arithmetic, 2 t - 1; stack; H2D copy; host clock around a device synchronise).  The
device output is compared bit for bit with the host path before anything is timed.  Prints one JSON line and writes it to
DIR/u8_image_probe.json."""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

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


def probe(name: str, ds, big: int, args) -> dict:
    from PIL import Image
    from rho_diffusion_amd.engine import ops
    dev = "cuda"
    N, H, W, C = ds.raw.shape
    oh, ow = (H, W) if ds.image_size is None else ds.image_size
    res = {"rows": N, "image": [H, W, C], "size": [oh, ow]}
    ds.batch(1)                                             # builds the tap tables and the LUT
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for B in (64, big):
        idx = torch.randint(0, N, (B,), device=dev, generator=gen)
        out = torch.empty(B, C, oh, ow, device=dev)
        run = lambda: ops.u8_image_batch(ds.raw, idx, (oh, ow), lut=ds._lut, taps=ds._taps, out=out, err_flag=flag)  # noqa: E731
        t = event_median(run, args.iters, args.warmup)
        moved = B * (H * W * C + C * oh * ow * 4)
        res[f"batch{B}_kernel_us"] = t
        res[f"batch{B}_bytes"] = moved
        res[f"batch{B}_GBps"] = moved / (t * 1e-6) / 1e9
        res[f"batch{B}_floor_8TBps_us"] = moved / 8e12 * 1e6
    ops.u8_image_check(flag)
    res["batch64_api_us"] = event_median(lambda: ds.batch(64), args.iters, args.warmup)
    ds.check_errors()
    # the reference-style host path for 64 items
    rows64 = torch.randint(0, N, (64,), generator=torch.Generator().manual_seed(1)).tolist()
    host = ds.data.numpy() if isinstance(ds.data, torch.Tensor) else ds.data

    def host_batch():
        items = []
        for i in rows64:
            img = Image.fromarray(host[i])
            if ds.image_size is not None:
                img = img.resize((ow, oh), Image.BILINEAR)
            a = np.array(img, copy=True)
            a = a[:, :, None] if a.ndim == 2 else a
            t = torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div(255)
            items.append(t * 2 - 1)
        out = torch.stack(items).to(dev)
        torch.cuda.synchronize()
        return out

    assert torch.equal(host_batch(), ds.batch(rows64)[0]), f"{name}: the device items differ from the host path"
    for _ in range(3):
        host_batch()
    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        host_batch()
        ts.append((time.perf_counter() - t0) * 1e6)
    res["host_path64_us"] = statistics.median(ts)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.environ.get("RHO_RUN_OUT", "runs"))
    ap.add_argument("--big", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--mnist-rows", type=int, default=60000)
    ap.add_argument("--cifar-rows", type=int, default=50000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the GPU"
    from make_golden_g22 import write_cifar_batches, write_mnist
    from rho_diffusion_amd.data import CIFAR10Dataset, MNISTDataset
    rng = np.random.default_rng(0)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        n = args.mnist_rows
        pair = (rng.integers(0, 256, size=(n, 28, 28), dtype=np.uint8), rng.integers(0, 10, size=n))
        write_mnist(tmp, pair, (pair[0][:16], pair[1][:16]))
        res["mnist"] = probe("mnist", MNISTDataset(tmp), args.big, args)
        n = args.cifar_rows
        pair = (rng.integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8), rng.integers(0, 10, size=n))
        write_cifar_batches(tmp, pair, (pair[0][:16], pair[1][:16]))
        res["cifar"] = probe("cifar", CIFAR10Dataset(tmp), args.big, args)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "u8_image_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
