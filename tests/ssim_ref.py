"""The structural similarity index restated in float64 with numpy only: the yardstick of tests/test_ssim_host.py and
tests/test_gpu_ssim.py.  Nothing here is shared with rho_diffusion_amd.

Inputs [B, C, *spatial] with 1 to 3 spatial dimensions.  Per dimension a window g (float32 values, used as float64); the n-D window
is their outer product, applied as a direct separable correlation over the windows that lie wholly inside the field.  ``fp32=True``
runs the same separable sums in float32 on the unshifted data: it only measures what float32 costs and is never a yardstick."""
import numpy as np


def window(gaussian_kernel, sigma, kernel_size):
    """One dimension's window, rounded once to float32."""
    if gaussian_kernel:
        k = 2 * int(3.5 * sigma + 0.5) + 1
        j = np.arange(k, dtype=np.float64)
        g = np.exp(-(((j - (k - 1) / 2.0) / sigma) ** 2) / 2.0)
        g = g / g.sum()
    else:
        g = np.full(kernel_size, 1.0 / kernel_size, dtype=np.float64)
    return g.astype(np.float32)


def windows(nd, gaussian_kernel=True, sigma=1.5, kernel_size=11):
    sig = list(sigma) if isinstance(sigma, (tuple, list)) else [sigma] * nd
    ks = list(kernel_size) if isinstance(kernel_size, (tuple, list)) else [kernel_size] * nd
    assert len(sig) == nd and len(ks) == nd
    return [window(gaussian_kernel, s, k) for s, k in zip(sig, ks)]


def correlate_valid(x, g, axis):
    """sum_j g[j] x[.., i + j, ..] for every i with the whole window inside: size - k + 1 outputs along ``axis``."""
    n = x.shape[axis] - len(g) + 1
    assert n >= 1
    acc = None
    for j in range(len(g)):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(j, j + n)
        term = g[j].astype(x.dtype) * x[tuple(sl)]
        acc = term if acc is None else acc + term
    return acc


def wsum(x, wins):
    """W[x]: the separable window sum over the spatial axes (2 ..)."""
    for d, g in enumerate(wins):
        x = correlate_valid(x, g, 2 + d)
    return x


def data_range_of(p, t):
    """data_range = None: the larger of the two extents."""
    return max(float(p.max()) - float(p.min()), float(t.max()) - float(t.min()))


def ssim(preds, target, wins, data_range=None, k1=0.01, k2=0.03, fp32=False):
    """dict: map [B, C, *(size - k + 1)], per_sample [B], mean, sum, R, the five moments (mu_p, mu_t, s_pp, s_tt, s_pt), and - for
    error bounds - the window sums of |a|, |b|, a^2, b^2, a b, |a b| and of a, b on the data shifted by target[b, c, 0, .., 0]."""
    dt = np.float32 if fp32 else np.float64
    p = np.asarray(preds, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    assert p.shape == t.shape and 3 <= p.ndim <= 5 and len(wins) == p.ndim - 2
    if isinstance(data_range, (tuple, list)):
        lo, hi = float(data_range[0]), float(data_range[1])
        p, t = np.clip(p, lo, hi), np.clip(t, lo, hi)
        R = hi - lo
    elif data_range is None:
        R = data_range_of(p, t)
    else:
        R = float(data_range)
    c1, c2 = (k1 * R) ** 2, (k2 * R) ** 2
    pp, tt = p.astype(dt), t.astype(dt)
    mu_p, mu_t = wsum(pp, wins), wsum(tt, wins)
    s_pp = np.maximum(wsum(pp * pp, wins) - mu_p * mu_p, 0)
    s_tt = np.maximum(wsum(tt * tt, wins) - mu_t * mu_t, 0)
    s_pt = wsum(pp * tt, wins) - mu_p * mu_t
    c1d, c2d = dt(c1), dt(c2)
    S = ((2 * mu_p * mu_t + c1d) * (2 * s_pt + c2d)) / ((mu_p * mu_p + mu_t * mu_t + c1d) * (s_pp + s_tt + c2d))
    S64 = S.astype(np.float64)
    per_sample = S64.reshape(S64.shape[0], -1).mean(axis=1)
    out = {"map": S, "per_sample": per_sample, "mean": float(per_sample.mean()), "sum": float(per_sample.sum()), "R": R, "c1": c1, "c2": c2,
           "mu_p": mu_p, "mu_t": mu_t, "s_pp": s_pp, "s_tt": s_tt, "s_pt": s_pt}
    if not fp32:
        shift = t[(slice(None), slice(None)) + (slice(0, 1),) * (p.ndim - 2)]
        a, b = p - shift, t - shift
        out.update(shift=shift, w_a=wsum(a, wins), w_b=wsum(b, wins), w_abs_a=wsum(np.abs(a), wins), w_abs_b=wsum(np.abs(b), wins),
                   w_aa=wsum(a * a, wins), w_bb=wsum(b * b, wins), w_ab=wsum(a * b, wins), w_abs_ab=wsum(np.abs(a * b), wins))
    return out


def brute_force(preds, target, wins, data_range, k1=0.01, k2=0.03):
    """The same index from the full outer-product window with explicit loops over every window position (tiny shapes only)."""
    p = np.asarray(preds, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    nd = p.ndim - 2
    full = np.ones((), dtype=np.float64)
    for g in wins:
        full = np.multiply.outer(full, g.astype(np.float64))
    R = float(data_range)
    c1, c2 = (k1 * R) ** 2, (k2 * R) ** 2
    oshape = tuple(p.shape[2 + d] - len(wins[d]) + 1 for d in range(nd))
    S = np.zeros(p.shape[:2] + oshape)
    for b in range(p.shape[0]):
        for c in range(p.shape[1]):
            for idx in np.ndindex(*oshape):
                sl = tuple(slice(i, i + len(g)) for i, g in zip(idx, wins))
                x, y = p[b, c][sl], t[b, c][sl]
                mu_p, mu_t = (full * x).sum(), (full * y).sum()
                s_pp = max((full * x * x).sum() - mu_p ** 2, 0.0)
                s_tt = max((full * y * y).sum() - mu_t ** 2, 0.0)
                s_pt = (full * x * y).sum() - mu_p * mu_t
                S[(b, c) + idx] = (2 * mu_p * mu_t + c1) * (2 * s_pt + c2) / ((mu_p ** 2 + mu_t ** 2 + c1) * (s_pp + s_tt + c2))
    return S
