"""The yardstick of the Sinkhorn tests: the debiased Sinkhorn divergence with epsilon scaling (what geomloss's
SamplesLoss("sinkhorn") computes for uniform weights, metrics/geom.py:28-37), restated with torch on the CPU.

float64 by default, gradient w.r.t. ``x`` through autograd: the last step is differentiated with the potentials that enter it held
constant and with the other argument of every cost detached.  ``fp32=True`` measures what float32 costs: every cost entry is
accumulated left to right in float32 (a cumulative sum) and the loop runs in float32.  It is never the code under test."""
import math

import numpy as np
import torch


def epsilon_schedule(diameter, p, blur, scaling):
    return ([diameter ** p] + [float(np.exp(e)) for e in np.arange(p * math.log(diameter), p * math.log(blur), p * math.log(scaling))]
            + [blur ** p])


def diameter_of(x, y):
    z = torch.cat([x, y]).double()
    return float((z.max(0).values - z.min(0).values).norm())


def sq_dists(u, v, fp32=False):
    """d2[i, j] = sum_d (u[i, d] - v[j, d])^2: float64, or float32 accumulated sequentially."""
    if fp32:
        sq = (u.float()[:, None, :] - v.float()[None, :, :]) ** 2
        seq = torch.from_numpy(np.cumsum(sq.detach().numpy(), axis=-1, dtype=np.float32)[..., -1].copy())
        tree = sq.sum(-1)                        # carries the gradient; the value is the sequential sum (both differences are exact)
        return tree + (seq - tree.detach())
    return ((u.double()[:, None, :] - v.double()[None, :, :]) ** 2).sum(-1)


def cost_of(d2, p):
    return torch.sqrt(torch.clamp(d2, min=1e-8)) if p == 1 else d2 / 2


def softmin(eps, C, h):
    return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)


def sinkhorn(x, y, p=1, blur=0.01, scaling=0.5, debias=True, fp32=False, diameter=None, want_grad=False, upstream=1.0, costs=None):
    """dict(loss, f = f_ba - f_aa, g = g_ab - g_bb, grad (d (upstream * loss) / dx or None), c_max, costs = (C_xy, C_xx, C_yy)).
    ``costs``: use these cost matrices (cast to the working dtype) instead of computing them - no gradient then."""
    dt = torch.float32 if fp32 else torch.float64
    x = x.detach().flatten(1).to(dt).clone().requires_grad_(want_grad)
    y = y.detach().flatten(1).to(dt)
    N, M = x.shape[0], y.shape[0]
    if diameter is None:
        diameter = diameter_of(x.detach(), y)
    if costs is None:
        xd = x.detach()
        C_xy, C_xx, C_yy = cost_of(sq_dists(x, y, fp32), p), cost_of(sq_dists(x, xd, fp32), p), cost_of(sq_dists(y, y, fp32), p)
    else:
        C_xy, C_xx, C_yy = [c.to(dt) for c in costs]
    c_max = float(max(C_xy.detach().max(), C_xx.detach().max(), C_yy.detach().max()))
    if diameter == 0.0:
        z = torch.zeros((), dtype=dt)
        return dict(loss=z, f=torch.zeros(N, dtype=dt), g=torch.zeros(M, dtype=dt), grad=torch.zeros_like(x) if want_grad else None,
                    c_max=c_max, costs=(C_xy.detach(), C_xx.detach(), C_yy.detach()))
    eps_list = [torch.tensor(e, dtype=dt) for e in epsilon_schedule(diameter, p, blur, scaling)]
    a_log = torch.full((N,), -math.log(N), dtype=dt)
    b_log = torch.full((M,), -math.log(M), dtype=dt)
    Dxy, Dyx, Dxx, Dyy = C_xy.detach(), C_xy.detach().T, C_xx.detach(), C_yy.detach()
    zero_n, zero_m = torch.zeros(N, dtype=dt), torch.zeros(M, dtype=dt)

    def sweep(eps, Cxy, Cxx, g_ab, f_ba, f_aa, g_bb):
        ft_ba = softmin(eps, Cxy, b_log + g_ab / eps)
        gt_ab = softmin(eps, Dyx, a_log + f_ba / eps)
        ft_aa = softmin(eps, Cxx, a_log + f_aa / eps) if debias else zero_n
        gt_bb = softmin(eps, Dyy, b_log + g_bb / eps) if debias else zero_m
        return ft_ba, gt_ab, ft_aa, gt_bb

    eps = eps_list[0]
    g_ab, f_ba = softmin(eps, Dyx, a_log), softmin(eps, Dxy, b_log)
    f_aa = softmin(eps, Dxx, a_log) if debias else zero_n
    g_bb = softmin(eps, Dyy, b_log) if debias else zero_m
    for eps in eps_list:
        ft_ba, gt_ab, ft_aa, gt_bb = sweep(eps, Dxy, Dxx, g_ab, f_ba, f_aa, g_bb)
        f_ba, g_ab, f_aa, g_bb = 0.5 * (f_ba + ft_ba), 0.5 * (g_ab + gt_ab), 0.5 * (f_aa + ft_aa), 0.5 * (g_bb + gt_bb)
    # the last step: plain, and the only one autograd sees (through C_xy and C_xx's first argument)
    h_b, h_a = (b_log + g_ab / eps_list[-1]).detach(), (a_log + f_aa / eps_list[-1]).detach()
    f_ba, g_ab, f_aa, g_bb = sweep(eps_list[-1], C_xy, C_xx, g_ab, f_ba, f_aa, g_bb)
    loss = (f_ba - f_aa).mean() + (g_ab - g_bb).mean()
    grad = None
    if want_grad and costs is None:
        (grad,) = torch.autograd.grad(upstream * loss, x)
    return dict(loss=loss.detach(), f=(f_ba - f_aa).detach(), g=(g_ab - g_bb).detach(), grad=grad, c_max=c_max, h_b=h_b, h_a=h_a,
                eps_last=float(eps_list[-1]),
                costs=(C_xy.detach(), C_xx.detach(), C_yy.detach()))


def closed_form_grad(x, y, p, eps, h_b, h_a, upstream=1.0):
    """The gradient formula the kernels implement, in float64, from the inputs h_b = b_log + g_ab / eps and h_a = a_log + f_aa / eps of
    the last step."""
    x, y = x.double().flatten(1), y.double().flatten(1)
    N = x.shape[0]
    d2xy, d2xx = sq_dists(x, y), sq_dists(x, x)
    C_xy, C_xx = cost_of(d2xy, p), cost_of(d2xx, p)
    P = torch.softmax(h_b[None, :] - C_xy / eps, dim=1)
    Q = torch.softmax(h_a[None, :] - C_xx / eps, dim=1)
    if p == 1:
        P = torch.where(d2xy <= 1e-8, torch.zeros_like(P), P / C_xy)
        Q = torch.where(d2xx <= 1e-8, torch.zeros_like(Q), Q / C_xx)
    return (upstream / N) * ((P.sum(1) - Q.sum(1))[:, None] * x - P @ y + Q @ x)
