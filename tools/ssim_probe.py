"""StructuralSimilarityIndexMeasure on the device against the same algorithm written with torch ops, on one GPU (DESIGN "Structural
similarity").

Shapes: the c3 sample batch (32 x 1 x 64^3), the c2 one (64 x 1 x 128^2) and the c5 one (2 x 1 x 128^3).  Per shape, alternated in
one process, HIP events, median of ``--reps`` runs after ``--warmup``, a fresh ``preds`` each run: the HIP path with a given
data_range, the torch-op form (five depthwise ``F.conv3d`` / ``F.conv2d`` calls with the dense window plus the elementwise formula:
what a user without the kernel writes), the HIP path with data_range=None and the range pass alone.  A step that has used up
``--limit`` seconds stops early and reports how many runs it timed.  Prints one JSON line per shape, with the kernel's effective
rate over the 8 bytes per voxel it must read.  The working sets (34 to 67 MB) sit inside the 256 MB Infinity Cache, which is not
flushed between runs: these are not HBM rates."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rho_diffusion_amd.engine import ops  # noqa: E402
from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure  # noqa: E402

SHAPES = {"c3": (32, 1, 64, 64, 64), "c2": (64, 1, 128, 128), "c5": (2, 1, 128, 128, 128)}


def torch_ssim(p, t, wins, data_range, k1=0.01, k2=0.03):
    """The valid-window index with stock torch ops: the dense n-D window, one depthwise convolution per moment."""
    nd = p.dim() - 2
    C = p.shape[1]
    w = wins[0]
    for g in wins[1:]:
        w = w[..., None] * g
    w = w.expand(C, 1, *w.shape).contiguous()
    conv = F.conv3d if nd == 3 else F.conv2d
    mu_p, mu_t = conv(p, w, groups=C), conv(t, w, groups=C)
    s_pp = (conv(p * p, w, groups=C) - mu_p * mu_p).clamp_min(0.0)
    s_tt = (conv(t * t, w, groups=C) - mu_t * mu_t).clamp_min(0.0)
    s_pt = conv(p * t, w, groups=C) - mu_p * mu_t
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    S = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))
    return S.flatten(1).mean(1).mean()


def timed(fn, xs, warmup, limit):
    """Median / min / max ms over the runs after the warm-up, run i on xs[i]; stops once ``limit`` seconds are used up."""
    ms, start = [], time.monotonic()
    for i, x in enumerate(xs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
        if time.monotonic() - start > limit and ms:
            break
    return {"median": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4),
            "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c2", "c5"], choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds per timed step")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_probe needs a GPU")
    dev = "cuda:0"
    for cfg in args.configs:
        shape = SHAPES[cfg]
        g = torch.Generator(device=dev).manual_seed(0)
        t = torch.rand(shape, device=dev, generator=g)
        ps = [t + 0.1 * torch.randn(shape, device=dev, generator=g) for _ in range(args.reps + args.warmup)]
        given, measured = StructuralSimilarityIndexMeasure(data_range=1.0), StructuralSimilarityIndexMeasure(data_range=None)
        wins = given._device_windows(t.device, len(shape) - 2)

        def hip_given(p):
            return given(p, t)

        def hip_none(p):
            return measured(p, t)

        def range_only(p):
            return ops.ssim_range(p, t)

        def torch_form(p):
            with torch.no_grad():
                return torch_ssim(p, t, wins, 1.0)

        res = {"config": cfg, "shape": list(shape), "reps": args.reps}
        # alternate the forms so that neither owns a quiet stretch of the machine
        steps = [("hip", hip_given), ("torch", torch_form), ("hip_2", hip_given), ("torch_2", torch_form), ("hip_range_none", hip_none),
                 ("range_pass", range_only)]
        for name, fn in steps:
            if args.skip_torch and name.startswith("torch"):
                continue
            res[name + "_ms"] = timed(fn, ps, args.warmup, args.limit)
        voxels = int(np.prod(shape))
        res["hip_GBps_over_8B_per_voxel"] = round(8 * voxels / (res["hip_ms"]["median"] * 1e-3) / 1e9, 1)
        res["range_pass_share_of_none_mode"] = round(res["range_pass_ms"]["median"] / res["hip_range_none_ms"]["median"], 3)
        res["ssim_hip"] = float(hip_given(ps[0]))
        if not args.skip_torch:
            res["ssim_torch"] = float(torch_form(ps[0]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
