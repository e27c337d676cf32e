"""WassersteinWrapper on the device against the same algorithm written with torch ops, on one GPU (DESIGN "Sample metrics").

Shapes: the c3 sample batch (32 x 32 x 262 144) and the c5 one (2 x 2 x 2 097 152).  Per shape, alternated in one process, HIP
events, median of ``--reps`` runs after ``--warmup``, a fresh ``y`` each run: forward and forward + backward of the HIP path
(schedule measured on the device, as a user gets it) and of the torch-op form (``torch.cdist`` + a ``logsumexp`` loop, autograd for the
gradient); then ``rho_pairwise_cost`` alone with its achieved GB/s over the (N + M) * D * 4 bytes it must read.  Prints one JSON
line per shape."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rho_diffusion_amd.engine import ops  # noqa: E402
from rho_diffusion_amd.metrics import WassersteinWrapper, epsilon_schedule  # noqa: E402

SHAPES = {"c3": (32, 262144), "c5": (2, 2097152)}


def torch_sinkhorn(x, y, p=1, blur=0.01, scaling=0.5):
    """The algorithm of metrics/geom.py with stock torch ops (what a user without the kernels would write)."""
    N, M = x.shape[0], y.shape[0]
    z = torch.cat([x.detach(), y])
    diameter = float((z.max(0).values - z.min(0).values).norm())
    eps_list = epsilon_schedule(diameter, p, blur, scaling)

    def cost(u, v, self_cost=False):
        d = torch.cdist(u, v)
        if self_cost:        # cdist expands |u|^2 - 2 u.v + |v|^2 for more than 25 rows: the diagonal comes out as rounding noise, not 0
            d = d.masked_fill(torch.eye(u.shape[0], dtype=torch.bool, device=u.device), 0.0)
        return d.clamp_min(1e-4) if p == 1 else d * d / 2

    def softmin(eps, C, h):
        return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)

    C_xy, C_xx, C_yy = cost(x, y), cost(x, x.detach(), True), cost(y, y, True)
    Dxy, Dyx, Dxx = C_xy.detach(), C_xy.detach().T, C_xx.detach()
    a_log = torch.full((N,), -math.log(N), device=x.device)
    b_log = torch.full((M,), -math.log(M), device=x.device)
    eps = eps_list[0]
    g_ab, f_ba, f_aa, g_bb = softmin(eps, Dyx, a_log), softmin(eps, Dxy, b_log), softmin(eps, Dxx, a_log), softmin(eps, C_yy, b_log)
    for eps in eps_list:
        ft_ba, gt_ab = softmin(eps, Dxy, b_log + g_ab / eps), softmin(eps, Dyx, a_log + f_ba / eps)
        ft_aa, gt_bb = softmin(eps, Dxx, a_log + f_aa / eps), softmin(eps, C_yy, b_log + g_bb / eps)
        f_ba, g_ab, f_aa, g_bb = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab), 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
    eps = eps_list[-1]
    f_ba, g_ab, f_aa, g_bb = (softmin(eps, C_xy, (b_log + g_ab / eps).detach()), softmin(eps, Dyx, a_log + f_ba / eps),
                              softmin(eps, C_xx, (a_log + f_aa / eps).detach()), softmin(eps, C_yy, b_log + g_bb / eps))
    return (f_ba - f_aa).mean() + (g_ab - g_bb).mean()


def timed(fn, ys, warmup):
    """Median ms over the runs after the warm-up; run i uses ys[i]."""
    ms = []
    for i, y in enumerate(ys):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(y)
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c5"], choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_probe needs a GPU")
    dev = "cuda:0"
    w = WassersteinWrapper()
    for cfg in args.configs:
        B, D = SHAPES[cfg]
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(B, D, device=dev, generator=g)
        ys = [torch.randn(B, D, device=dev, generator=g) + 0.5 for _ in range(args.reps + args.warmup)]

        def hip_fwd(y):
            with torch.no_grad():
                return w(x, y)

        def hip_fwd_bwd(y):
            xr = x.detach().requires_grad_(True)
            w(xr, y).backward()
            return xr.grad

        def torch_fwd(y):
            with torch.no_grad():
                return torch_sinkhorn(x, y)

        def torch_fwd_bwd(y):
            xr = x.detach().requires_grad_(True)
            torch_sinkhorn(xr, y).backward()
            return xr.grad

        ws = ops.sinkhorn_workspace(x, ys[0])

        def cost_only(y):
            return ops.pairwise_cost(x, y, 1, workspace=ws)

        res = {"config": cfg, "N": B, "M": B, "D": D, "reps": args.reps}
        # alternate the two forms so that neither owns a quiet stretch of the machine
        for name, fn in (("hip_fwd", hip_fwd), ("torch_fwd", torch_fwd), ("hip_fwd_bwd", hip_fwd_bwd), ("torch_fwd_bwd", torch_fwd_bwd),
                         ("hip_fwd_2", hip_fwd), ("torch_fwd_2", torch_fwd), ("cost_pass", cost_only)):
            med, lo, hi = timed(fn, ys, args.warmup)
            res[name + "_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        res["cost_pass_GBps"] = round(2 * B * D * 4 / (res["cost_pass_ms"]["median"] * 1e-3) / 1e9, 1)
        res["loss_hip"] = float(hip_fwd(ys[0]))
        res["loss_torch"] = float(torch_fwd(ys[0]))
        gh, gt = hip_fwd_bwd(ys[0]), torch_fwd_bwd(ys[0])
        res["grad_rel_l2_hip_vs_torch"] = float((gh - gt).norm() / gt.norm())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
