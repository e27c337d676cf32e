"""Float64 reference, float32 restatement and per-element error bounds for the loss side of csrc/gaussian.hip (importable without a
GPU).  Formulas: the reference's metrics/losses.py (normal_kl, approx_standard_normal_cdf, discretized_gaussian_log_likelihood) and
gaussian_diffusion.py:826-934 (_vb_terms_bpd, training_losses) with :368-383 (learned variances) and :445-450 (x0 from epsilon).

Three evaluations of the same expressions:
  * ``T64``: torch float64 on the CPU.  The branch thresholds -0.999, 0.999, 1/255 and 1e-12 are the float32 constants widened, so the
    branches agree with the kernel on every exactly representable input; the tables are the float32 rows the kernel reads, widened.
    The gradient of the hybrid loss is torch autograd of this expression (clamp(min=1e-12) and where cut the path as in the reference).
  * ``N32``: numpy float32 in the kernels' own operation order, one rounding per operation (what the device computes up to the ulps
    of its tanhf / expf / logf); the backward is the kernels' closed form (gd_nll_bwd, gd_kl_bwd).
  * the bounds: float64 arrays of the shape check_bound (gpu_util.py) takes, u = 2^-24:
      dgll           K * u * (1/max(d, 1e-12) + |log d| + 1)      d: the pre-clamp argument of the log (float64); the 1/d term is the
                                                                  cancellation of two CDF values good to a few ulps of 1
      normal_kl      K * u * sum |addends|
      NLL gradient   K_g * u * (|a1| + |a2|) * inv_stdv / 2 * (1 + (cdf_plus + cdf_min) / d)      a1, a2: the two addends of g_inv;
                     in the lower tail the mirrored 2 - cdf_plus - cdf_min (cdf(-u) = 1 - cdf(u) carries the same ulps of 1)
      KL gradient    K_g * u * sum |addends of gd_kl_bwd|
      squared diffs  K * u * (e^2 + 2 |e| * sum |addends of e|)
      per-sample     mean of the element bounds + 4 * u * |result|  (the final float32 division and scaling)

Regimes of a dgll element by its float64 d: ``BOUNDED`` d >= 1e-6; ``SATURATED`` both tanh arguments beyond +-12 on one side (the
float32 CDFs are exactly 0 or 1: the forward is logf(1e-12f), the gradient 0); ``BETWEEN`` the rest, where float32 quantises d to
multiples of 2^-25 and no useful bound exists: left out of element checks, at most 5 % of a case (none by construction: offsets of
0, 0.3, 1, 3 sigma and >= 14 sigma).  Where a per-sample mean holds such elements (only behind the quantile threshold, which moves the
offsets) their share of the bound is the interval |log(max(d -+ K u, 1e-12)) - log d| that an absolute error of K u on d allows.
A SATURATED element enters a mean with the ulps of log(1e-12) alone (plus the reference's distance from it, 0 for d < 1e-12).

The constants K: worst ratio error / (u * condition term) of N32 against T64 over every input set of the GPU tests (measured by
test_gd_loss_ref_host.py, which asserts ratio <= K / 2), times 4 for the device's tanhf / expf / logf (a few ulps each), rounded up:
    quantity                                   measured ratio     K
    cdf                                             1.33           6
    dgll (metric operands)                          2.38          10
    normal_kl (metric operands, prior)              4.62          19     (exp of a rounded lv1 - lv2 of up to 8: |lv1 - lv2| ulps)
    VLB chain: kl                                   9.12          37
    VLB chain: nll                                 13.40          54
    VLB chain / hybrid: squared differences         2.47          10
    hybrid gradient, NLL (K_g)                     16.23          65     (3-sigma elements: 1 - tanh^2 carries tanh's ulp of 1)
    hybrid gradient, KL  (K_g)                      9.43          38

In the chain (x0 -> model mean -> kl / nll, and their gradients) the bounds' condition terms are extended by what the rounding of the
chain's own operands propagates (``_propagated``): the terms above take the operands of dgll / normal_kl as exact, but the model mean
is a rounded float32 sum whose error in units of sigma grows as 1 / sigma (without this term the same measurement gives ratios in
the thousands at log-scales near -6 and for x0 from epsilon at t = T - 1, where sqrt_recip * x_t cancels).
"""
from __future__ import annotations

import numpy as np
import torch

from detdata import det_normal, det_uniform

f32 = np.float32
U = 2.0 ** -24
GD_THREADS = 256
X_LO, X_HI = float(f32(-0.999)), float(f32(0.999))
BIN = float(f32(1.0 / 255.0))
CLAMP = float(f32(1e-12))
LOG_CLAMP32 = f32(np.log(np.float64(f32(1e-12))))          # logf(1e-12f), correctly rounded
LOG_QUANT32 = f32(np.log(2.0 ** -26))                      # the smallest nonzero float32 d of the BETWEEN regime is 2^-25 > 2^-26
LN2_32 = float(f32(0.69314718055994530942))
SQ2PI, C3 = float(np.sqrt(2.0 / np.pi)), 0.044715
BOUNDED, SATURATED, BETWEEN = 0, 1, 2
LEARNED, LEARNED_RANGE = "LEARNED", "LEARNED_RANGE"

K = {"cdf": 6, "dgll": 10, "kl": 19, "vlb_kl": 37, "vlb_nll": 54, "sq": 10, "g_nll": 65, "g_kl": 38}


# ---------------------------------------------------------------------------------------------------------------- the two arithmetics
class T64:
    exp, tanh, log, where, abs = torch.exp, torch.tanh, torch.log, torch.where, torch.abs

    @staticmethod
    def a(v):
        """operand -> float64 tensor (float32 values widen exactly)"""
        return v.double() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))

    c = staticmethod(float)                                 # a float32 constant of the kernel, widened
    k = staticmethod(float)                                 # a mathematical constant, in full precision

    @staticmethod
    def clamp_min(v, lo):
        return v.clamp(min=lo)

    @staticmethod
    def clamp(v, lo, hi):
        return torch.minimum(torch.maximum(v, lo), hi)


class N32:
    exp, tanh, log, where, abs = np.exp, np.tanh, np.log, np.where, np.abs

    @staticmethod
    def a(v):
        v = v.numpy() if torch.is_tensor(v) else np.asarray(v)
        assert v.dtype == np.float32
        return v

    c = staticmethod(f32)
    k = staticmethod(f32)

    @staticmethod
    def clamp_min(v, lo):
        return np.maximum(v, lo)

    @staticmethod
    def clamp(v, lo, hi):
        return np.minimum(np.maximum(v, lo), hi)


def _tanh_arg(A, u):
    x3 = (u * u) * u
    return A.k(SQ2PI) * (u + A.k(C3) * x3)


def _cdf(A, u):
    return A.c(0.5) * (A.c(1.0) + A.tanh(_tanh_arg(A, u)))


def _dgll(A, x, mean, log_scale):
    """(log-likelihood, d, branch [0: x < -0.999, 1: x > 0.999, 2: interior], cdf_plus, cdf_min, tanh arguments)"""
    centered = x - mean
    inv = A.exp(-log_scale)
    plus_in, min_in = inv * (centered + A.c(BIN)), inv * (centered - A.c(BIN))
    cp, cm = _cdf(A, plus_in), _cdf(A, min_in)
    lo, hi = x < A.c(X_LO), x > A.c(X_HI)
    d = A.where(lo, cp, A.where(hi, A.c(1.0) - cm, cp - cm))
    branch = np.where(np.asarray(lo), 0, np.where(np.asarray(hi), 1, 2)) + np.zeros(np.asarray(d.detach() if torch.is_tensor(d) else d).shape, int)
    return A.log(A.clamp_min(d, A.c(CLAMP))), d, branch, (cp, cm, inv, plus_in, min_in)


def _kl(A, m1, lv1, m2, lv2):
    d = m1 - m2
    k0 = ((A.c(-1.0) + lv2) - lv1) + A.exp(lv1 - lv2)
    return A.c(0.5) * (k0 + (d * d) * A.exp(-lv2))


# ---------------------------------------------------------------------------------------------------------------- metrics, float64
def cdf(u):
    return _cdf(T64, T64.a(u))


def cdf32(u):
    return _cdf(N32, N32.a(u))


def cdf_bound(u, k=None):
    return torch.full_like(T64.a(u), (K["cdf"] if k is None else k) * U)


def regimes(d, branch, plus_in, min_in):
    """BOUNDED / SATURATED / BETWEEN per element, from the float64 d and the float64 tanh arguments"""
    vp, vm = _tanh_arg(T64, plus_in), _tanh_arg(T64, min_in)
    b = torch.from_numpy(np.asarray(branch))
    sat = torch.where(b == 0, vp < -12.0, torch.where(b == 1, vm > 12.0, ((vp > 12.0) & (vm > 12.0)) | ((vp < -12.0) & (vm < -12.0))))
    r = torch.where(d >= 1e-6, BOUNDED, torch.where(sat, SATURATED, BETWEEN))
    return r.numpy()


def dgll_bound_of(d, k, regime=None, propagated=None):
    """The bound from the float64 d.  BOUNDED (d >= 1e-6): the linear form of the docstring (+ k u ``propagated`` in the chain).
    SATURATED (with ``regime``): float32 gives logf(1e-12f) whatever float64 still resolves, so the distance of the reference from
    log(1e-12) plus the ulps of that value, k u (|log 1e-12| + 1); for d < 1e-12 (every element built beyond 14 sigma) the distance is 0.
    BETWEEN: the interval an absolute error of k u on d allows."""
    dc = d.clamp(min=CLAMP)
    ulps = k * U * (dc.log().abs() + 1.0)
    lin = k * U / dc + ulps
    if propagated is not None:
        lin = lin + k * U * propagated
    up = (d + k * U).clamp(min=CLAMP).log() - dc.log()
    dn = dc.log() - (d - k * U).clamp(min=CLAMP).log()
    out = torch.where(d >= 1e-6, lin, torch.maximum(up, dn) + ulps + (0.0 if propagated is None else k * U * propagated))
    if regime is not None:
        sat = (dc.log() - np.log(CLAMP)).abs() + k * U * (abs(np.log(CLAMP)) + 1.0)
        out = torch.where(torch.from_numpy(np.asarray(regime)) == SATURATED, sat, out)
    return out


def dgll(x, mean, log_scale, k=None):
    """float64 discretized_gaussian_log_likelihood: dict(value, d, branch, regime, bound)"""
    x, mean, log_scale = (T64.a(v) for v in (x, mean, log_scale))
    x, mean, log_scale = torch.broadcast_tensors(x, mean, log_scale)
    val, d, branch, (cp, cm, inv, pi, mi) = _dgll(T64, x, mean, log_scale)
    reg = regimes(d, branch, pi, mi)
    return {"value": val, "d": d, "branch": branch, "regime": reg, "bound": dgll_bound_of(d, K["dgll"] if k is None else k, reg)}


def dgll32(x, mean, log_scale):
    x, mean, log_scale = np.broadcast_arrays(*(N32.a(v) for v in (x, mean, log_scale)))
    return _dgll(N32, x, mean, log_scale)[0]


def normal_kl(m1, lv1, m2, lv2, k=None):
    """float64 normal_kl and its bound"""
    m1, lv1, m2, lv2 = torch.broadcast_tensors(*(T64.a(v) for v in (m1, lv1, m2, lv2)))
    return _kl(T64, m1, lv1, m2, lv2), kl_bound_of(m1, lv1, m2, lv2, K["kl"] if k is None else k)


def kl_bound_of(m1, lv1, m2, lv2, k):
    return k * U * 0.5 * (1.0 + lv2.abs() + lv1.abs() + torch.exp(lv1 - lv2) + (m1 - m2) ** 2 * torch.exp(-lv2))


def normal_kl32(m1, lv1, m2, lv2):
    m1, lv1, m2, lv2 = np.broadcast_arrays(*(N32.a(v) for v in (m1, lv1, m2, lv2)))
    return _kl(N32, m1, lv1, m2, lv2)


# ---------------------------------------------------------------------------------------------------------------- the chain
ROWS = ("sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "model_logvar", "post_logvar", "log_beta", "sqrt_abar", "log_1m_abar", "1m_abar")


def rows_at(A, tab32: np.ndarray, t) -> dict:
    """the float32 table rows at t as [B, 1] operands of arithmetic A; ``t0`` = (t == 0) as a [B, 1] bool array"""
    from rho_diffusion_amd.engine.ops import GD_ROW
    t = np.asarray(t)
    r = {k: A.a(np.ascontiguousarray(tab32[GD_ROW[k]][t].reshape(-1, 1))) for k in ROWS}
    r["t0"] = (t == 0).reshape(-1, 1)
    return r


def _x0(A, r, xt, m, eps_mode, s=None):
    x0 = m
    if eps_mode:
        p0, p1 = r["sqrt_recip"] * xt, r["sqrt_recipm1"] * m
        x0 = p0 - p1
    if s is not None:
        x0 = A.clamp(x0, -s, s) / s
    return x0


def _logvar(A, r, v, var):
    if var is None:
        return r["model_logvar"]
    if var == LEARNED:
        return v
    frac = (v + A.c(1.0)) / A.c(2.0)
    p0, p1 = frac * r["log_beta"], (A.c(1.0) - frac) * r["post_logvar"]
    return p0 + p1


def _means(A, r, xs, xt, x0):
    cx = r["coef2"] * xt
    return (r["coef1"] * xs) + cx, (r["coef1"] * x0) + cx


def _elements(A, tab32, t, xs, xt, m, v, eps_mode, var, s=None, noise=None):
    """per-element terms of _vb_terms_bpd in arithmetic A, [B, n] each"""
    r = rows_at(A, tab32, t)
    xs, xt, m = A.a(xs), A.a(xt), A.a(m)
    s = None if s is None else A.a(s).reshape(-1, 1)
    x0 = _x0(A, r, xt, m, eps_mode, s)
    lv2 = _logvar(A, r, A.a(v) if v is not None else None, var)
    tm, mm = _means(A, r, xs, xt, x0)
    lv1 = r["post_logvar"]
    out = {"r": r, "x0": x0, "lv2": lv2, "tm": tm, "mm": mm, "kl": _kl(A, tm, lv1, mm, lv2)}
    ll, d, branch, (cp, cm, inv, pi, mi) = _dgll(A, xs, mm, A.c(0.5) * lv2)
    out.update(nll=-ll, d=d, branch=branch, cp=cp, cm=cm, inv=inv, plus_in=pi, min_in=mi)
    dx = x0 - xs
    out["dx2"] = dx * dx
    if noise is not None:
        ax = r["sqrt_recip"] * xt
        eps = (ax - x0) / r["sqrt_recipm1"]
        de = eps - A.a(noise)
        out.update(de2=de * de, de=de, ax=ax)
    return out


def _mean64(v):
    v = torch.as_tensor(np.asarray(v, dtype=np.float64)) if not torch.is_tensor(v) else v.double()
    return v.reshape(v.shape[0], -1).mean(1)


def _mean_bound(eb, result, scale=1.0):
    return _mean64(eb) * scale + 4.0 * U * result.abs()


def _sq_bound(e2, addends, k):
    """the bound of a squared difference e^2 whose e carries an error of a few u * addends: k u (e^2 + 2 |e| addends + k u addends^2)"""
    return k * U * (e2 + 2.0 * e2.sqrt() * addends + k * U * addends ** 2)


def _propagated(e, xs, xt, m, v, eps_mode, var, g_el=None):
    """What the float32 rounding of the chain's own operands adds to a bound, per unit of K * u: |d f / d operand| times the sum of
    the absolute addends that form the operand (model mean, true mean, learned log-variance), for f = kl and nll; with the upstream
    gradient ``g_el`` of one element's term also for f = d kl / d logvar and d nll / d logvar (second derivatives by autograd).
    The bounds' own condition terms take their operands as exact; in the chain the model mean is a rounded float32 sum whose error,
    in units of sigma, grows as 1 / sigma (and with sqrt_recip * x_t where x0 comes from epsilon)."""
    r = e["r"]
    xs, xt, m = T64.a(xs), T64.a(xt), T64.a(m).detach()
    x0, tm, mm, lv2 = e["x0"].detach(), e["tm"].detach(), e["mm"].detach(), e["lv2"].detach().expand_as(e["tm"])
    lv1 = r["post_logvar"]
    a_x0 = x0.abs() + ((r["sqrt_recip"] * xt).abs() + (r["sqrt_recipm1"] * m).abs() if eps_mode else 0.0)
    a_mm = (r["coef1"] * x0).abs() + (r["coef2"] * xt).abs() + r["coef1"].abs() * a_x0
    a_tm = (r["coef1"] * xs).abs() + (r["coef2"] * xt).abs()
    a_lv = torch.zeros_like(tm)
    if var == LEARNED_RANGE:
        frac = (T64.a(v).detach() + 1.0) / 2.0
        a_lv = (frac * r["log_beta"]).abs() + ((1.0 - frac) * r["post_logvar"]).abs()
    d, e2, e12 = tm - mm, torch.exp(-lv2), torch.exp(lv1 - lv2)
    out = {"kl": d.abs() * e2 * (a_mm + a_tm) + 0.5 * (1.0 - e12 - d * d * e2).abs() * a_lv}
    mm_, lv_ = mm.clone().requires_grad_(True), lv2.clone().requires_grad_(True)
    ll = _dgll(T64, xs, mm_, 0.5 * lv_)[0]
    s_mm, s_lv = torch.autograd.grad(ll.sum(), (mm_, lv_), create_graph=g_el is not None)
    out["nll"] = (s_mm.abs() * a_mm + s_lv.abs() * a_lv).detach()
    if g_el is not None:
        g1 = (g_el * 0.5).abs()
        out["g_kl"] = g1 * (2.0 * d.abs() * e2 * (a_mm + a_tm) + (e12 + d * d * e2) * a_lv)
        if s_lv.requires_grad:
            h_mm, h_lv = torch.autograd.grad(s_lv.sum(), (mm_, lv_), allow_unused=True)
            z = torch.zeros_like(tm)
            out["g_nll"] = g_el.abs() * ((z if h_mm is None else h_mm).abs() * a_mm + (z if h_lv is None else h_lv).abs() * a_lv)
        else:
            out["g_nll"] = torch.zeros_like(tm)
    return out


def vlb_terms(tab32, t, xs, xt, m, v, eps_mode, var, s=None, noise=None):
    """float64 per-sample kl, nll (bits), xstart_mse, mse, vb = where(t == 0, nll, kl), each with its bound, the regimes of the NLL's
    elements, and the float32 restatement's pred_xstart and per-sample values (float64 means of the float32 elements)."""
    e = _elements(T64, tab32, t, xs, xt, m, v, eps_mode, var, s, noise)
    r, em = e["r"], int(bool(eps_mode))
    lv1 = r["post_logvar"].expand_as(e["tm"])
    lv2 = e["lv2"].expand_as(e["tm"])
    out = {"regime": regimes(e["d"], e["branch"], e["plus_in"], e["min_in"]), "elements": e}
    pr = _propagated(e, xs, xt, m, v, eps_mode, var)
    b_kl = kl_bound_of(e["tm"], lv1, e["mm"], lv2, K["vlb_kl"]) + K["vlb_kl"] * U * pr["kl"]
    b_nll = dgll_bound_of(e["d"], K["vlb_nll"], out["regime"], pr["nll"])
    out["elem_bound"] = {"kl": b_kl, "nll": b_nll}
    kl, nll = _mean64(e["kl"]) / LN2_32, _mean64(e["nll"]) / LN2_32
    out["kl"], out["kl_bound"] = kl, _mean_bound(b_kl, kl, 1.0 / LN2_32)
    out["nll"], out["nll_bound"] = nll, _mean_bound(b_nll, nll, 1.0 / LN2_32)
    t0 = torch.from_numpy(np.asarray(t) == 0)
    out["vb"], out["vb_bound"] = torch.where(t0, nll, kl), torch.where(t0, out["nll_bound"], out["kl_bound"])
    xm = _mean64(e["dx2"])
    add_x0 = (r["sqrt_recip"] * T64.a(xt)).abs() + (r["sqrt_recipm1"] * T64.a(m)).abs() if eps_mode else T64.a(m).abs()
    out["elem_bound"]["dx2"] = _sq_bound(e["dx2"], add_x0 + T64.a(xs).abs(), K["sq"])
    out["xstart_mse"], out["xstart_mse_bound"] = xm, _mean_bound(out["elem_bound"]["dx2"], xm)
    if noise is not None:
        ms = _mean64(e["de2"])
        out["elem_bound"]["de2"] = _sq_bound(e["de2"], (e["ax"].abs() + add_x0) / r["sqrt_recipm1"] + T64.a(noise).abs(), K["sq"])
        out["mse"], out["mse_bound"] = ms, _mean_bound(out["elem_bound"]["de2"], ms)
    out["n32"] = _elements(N32, tab32, t, xs, xt, m, v, eps_mode, var, s, noise)
    return out


def prior_terms(tab32, xs):
    """float64 _prior_bpd per sample (bits) and its bound"""
    from rho_diffusion_amd.engine.ops import GD_ROW
    xs = T64.a(xs)
    sa, lv1 = float(tab32[GD_ROW["sqrt_abar"], -1]), float(tab32[GD_ROW["log_1m_abar"], -1])
    m1, z = sa * xs, torch.zeros_like(xs)
    kl = _kl(T64, m1, z + lv1, z, z)
    res = _mean64(kl) / LN2_32
    return res, _mean_bound(kl_bound_of(m1, z + lv1, z, z, K["kl"]), res, 1.0 / LN2_32)


def prior32(tab32, xs):
    from rho_diffusion_amd.engine.ops import GD_ROW
    xs = N32.a(xs)
    z = np.zeros_like(xs)
    return _kl(N32, tab32[GD_ROW["sqrt_abar"], -1] * xs, z + tab32[GD_ROW["log_1m_abar"], -1], z, z)


# ---------------------------------------------------------------------------------------------------------------- hybrid loss
def _hybrid_elems(A, tab32, t, xs, xt, tg, m, v, eps_mode, var):
    e = _elements(A, tab32, t, xs, xt, m, v, eps_mode, var)
    d = A.a(tg) - A.a(m)
    e["sq"] = d * d
    t0 = e["r"]["t0"]
    e["vbe"] = A.where(torch.from_numpy(t0) if A is T64 else t0, e["nll"], e["kl"])
    return e


def hybrid_loss(tab32, t, xs, xt, tg, mo, eps_mode, var, vb_scale=None, g_loss=None, g_mse=None, g_vb=None):
    """float64 training_losses (MSE / RESCALED_MSE, learned variance) on mo [B, 2n]: mse, vb, loss with bounds; with upstream
    gradients also d/d mo by float64 autograd and the bound of its variance half (the mean half is exact: see hybrid_grad32)."""
    B, n = xs.shape
    em = int(bool(eps_mode))
    leaf = T64.a(mo).clone().requires_grad_(True)
    m, v = leaf[:, :n], leaf[:, n:]
    e = _hybrid_elems(T64, tab32, t, xs, xt, tg, m.detach(), v, eps_mode, var)
    sq = (T64.a(tg) - m) ** 2
    scale = 1.0 if vb_scale is None else float(f32(vb_scale))
    mse = sq.mean(1)
    vb = e["vbe"].mean(1) / LN2_32 * scale
    loss = mse + vb
    r = e["r"]
    t0 = torch.from_numpy(r["t0"])
    lv1 = r["post_logvar"].expand_as(e["tm"])
    have_g = not (g_loss is None and g_mse is None and g_vb is None)
    z = torch.zeros(B, dtype=torch.float64)
    gl, gm, gv = (z if g is None else T64.a(g) for g in (g_loss, g_mse, g_vb))
    g_el = ((gl + gv) * scale / LN2_32 / n).reshape(-1, 1)              # the upstream gradient of one element's VLB term
    pr = _propagated(e, xs, xt, m, v, eps_mode, var, g_el if have_g else None)
    reg = regimes(e["d"].detach(), e["branch"], e["plus_in"].detach(), e["min_in"].detach())
    eb = torch.where(t0, dgll_bound_of(e["d"].detach(), K["vlb_nll"], reg, pr["nll"]),
                     kl_bound_of(e["tm"], lv1, e["mm"], e["lv2"].detach().expand_as(e["tm"]), K["vlb_kl"]) + K["vlb_kl"] * U * pr["kl"])
    out = {"mse": mse.detach(), "vb": vb.detach(), "loss": loss.detach(), "regime": reg, "t0": r["t0"]}
    sqd = sq.detach()
    out["elements"] = {"sq": sqd, "vbe": e["vbe"].detach()}
    out["elem_bound"] = {"sq": K["sq"] * U * sqd, "vbe": eb}
    out["mse_bound"] = _mean_bound(out["elem_bound"]["sq"], out["mse"])
    out["vb_bound"] = _mean_bound(eb, out["vb"], scale / LN2_32)
    out["loss_bound"] = out["mse_bound"] + out["vb_bound"] + 2 * U * out["loss"].abs()
    if not have_g:
        return out
    ((loss * gl).sum() + (mse * gm).sum() + (vb * gv).sum()).backward()
    out["grad"] = leaf.grad.detach()
    # the bound of the variance half: the upstream gradient of one element's term, then the addends of the kernels' closed forms
    with torch.no_grad():
        lv2, inv = e["lv2"], e["inv"]
        dcdf = lambda u: 0.5 * (1.0 - torch.tanh(_tanh_arg(T64, u)) ** 2) * SQ2PI * (1.0 + 3.0 * C3 * u * u)
        cpb, cmb = e["plus_in"] / inv, e["min_in"] / inv
        b = torch.from_numpy(e["branch"])
        dc = e["d"].clamp(min=CLAMP)
        g_cp = torch.where(b == 1, 0.0, g_el / dc)
        g_cm = torch.where(b == 0, 0.0, g_el / dc)
        a1, a2 = (g_cp * dcdf(e["plus_in"]) * cpb).abs(), (g_cm * dcdf(e["min_in"]) * cmb).abs()
        # (cdf_plus + cdf_min) / d: the CDF values' ulps against d.  0.5 * (1 + tanh) is good to a few ulps of 1 at either end
        # (tanh near -1 has the ulp of tanh near 1), so the lower tail takes the mirrored sum 2 - cdf_plus - cdf_min
        csum = torch.maximum(e["cp"] + e["cm"], 2.0 - e["cp"] - e["cm"])
        nll_b = K["g_nll"] * U * ((a1 + a2) * inv / 2.0 * (1.0 + csum / dc) + pr["g_nll"])
        nll_b = torch.where(e["d"] >= CLAMP, nll_b, 0.0)                                    # the clamp cuts the path: exactly 0
        g1 = (g_el * 0.5).abs()
        kl_b = K["g_kl"] * U * (g1 + g1 * torch.exp(lv1 - lv2) + g1 * (e["tm"] - e["mm"]) ** 2 * torch.exp(-lv2) + pr["g_kl"])
        dv = 1.0 if var == LEARNED else (r["log_beta"].abs() + r["post_logvar"].abs()) / 2.0
        out["grad_v_bound"] = torch.where(t0, nll_b, kl_b) * dv
    return out


def _cdf_bwd32(g, u):
    """gd_cdf_bwd: (d u, cdf)"""
    x3 = (u * u) * u
    w = f32(SQ2PI) * (u + f32(C3) * x3)
    th = np.tanh(w)
    gw = (g * f32(0.5)) * (f32(1.0) - th * th)
    gin = gw * f32(SQ2PI)
    return gin + (gin * f32(C3)) * (f32(3.0) * (u * u)), f32(0.5) * (f32(1.0) + th)


def hybrid32(tab32, t, xs, xt, tg, mo, eps_mode, var, vb_scale=None, g_loss=None, g_mse=None, g_vb=None):
    """the float32 restatement of k_gd_hybrid_partial / _final (float64 means of float32 elements, then the float32 tail) and, with
    upstream gradients, of k_gd_hybrid_bwd: grad [B, 2n] float32"""
    B, n = xs.shape
    mo = N32.a(mo)
    m, v = mo[:, :n], mo[:, n:]
    e = _hybrid_elems(N32, tab32, t, xs, xt, tg, m, v, eps_mode, var)
    mse = e["sq"].astype(np.float64).mean(1).astype(f32)
    vb = e["vbe"].astype(np.float64).mean(1).astype(f32) / f32(LN2_32)
    if vb_scale is not None:
        vb = vb * f32(vb_scale)
    out = {"mse": mse, "vb": vb, "loss": mse + vb, "elements": e}
    if g_loss is None and g_mse is None and g_vb is None:
        return out
    z = np.zeros(B, f32)
    gl = z if g_loss is None else N32.a(g_loss)
    gms = gl if g_mse is None else gl + N32.a(g_mse)
    gvs = gl if g_vb is None else gl + N32.a(g_vb)
    if vb_scale is not None:
        gvs = gvs * f32(vb_scale)
    gm = (gms / f32(n)).reshape(-1, 1)
    gv = ((gvs / f32(LN2_32)) / f32(n)).reshape(-1, 1)
    dm = -(gm * (f32(2.0) * (N32.a(tg) - m)))
    r, xs_ = e["r"], N32.a(xs)
    lv2 = e["lv2"] + np.zeros_like(xs_)
    # gd_nll_bwd
    centered = xs_ - e["mm"]
    inv = np.exp(-(f32(0.5) * lv2))
    cpb, cmb = centered + f32(BIN), centered - f32(BIN)
    plus_in, min_in = inv * cpb, inv * cmb
    zero = np.zeros_like(xs_)
    _, cp = _cdf_bwd32(zero, plus_in)
    _, cm = _cdf_bwd32(zero, min_in)
    g_lp = -gv + zero
    one_m = f32(1.0) - cm
    dd = cp - cm
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lo, hi = xs_ < f32(X_LO), xs_ > f32(X_HI)
        g_cp = np.where(lo, np.where(cp >= f32(CLAMP), g_lp / cp, zero), np.where(hi, zero, np.where(dd >= f32(CLAMP), g_lp / dd, zero)))
        g_cm = np.where(lo, zero, np.where(hi, np.where(one_m >= f32(CLAMP), -(g_lp / one_m), zero), -g_cp))
    g_inv = _cdf_bwd32(g_cp, plus_in)[0] * cpb + _cdf_bwd32(g_cm, min_in)[0] * cmb
    d_nll = -(g_inv * inv) * f32(0.5)
    # gd_kl_bwd
    g1 = gv * f32(0.5) + zero
    d = e["tm"] - e["mm"]
    a = g1 + -(g1 * np.exp(r["post_logvar"] - lv2))
    d_kl = a + -((g1 * (d * d)) * np.exp(-lv2))
    dlv = np.where(r["t0"], d_nll, d_kl)
    if var == LEARNED_RANGE:
        dlv = (dlv * r["log_beta"] + -(dlv * r["post_logvar"])) / f32(2.0)
    out["grad"] = np.concatenate([dm, dlv.astype(f32)], axis=1)
    return out


def mse32(tg, o, g=None):
    """rho_gd_mse_per_sample (float64 mean of float32 squares, rounded) and, with g, rho_gd_mse_per_sample_bwd"""
    tg, o = N32.a(tg), N32.a(o)
    d = tg - o
    if g is None:
        return (d * d).astype(np.float64).mean(1)
    gn = (N32.a(g) / f32(tg.shape[1])).reshape(-1, 1)
    return -(gn * (f32(2.0) * d))


# ---------------------------------------------------------------------------------------------------------------- inputs
EDGE_X = np.array([-1.0, 1.0, f32(-0.999), f32(0.999), np.nextafter(f32(-0.999), f32(-2)), np.nextafter(f32(-0.999), f32(2)),
                   np.nextafter(f32(0.999), f32(-2)), np.nextafter(f32(0.999), f32(2))], dtype=f32)
_OFFSETS = np.array([0.0, 0.3, 1.0, 3.0, -0.3, -1.0, -3.0, 0.0, 0.3, -1.0, 3.0, -3.0, 1.0, -0.3, 16.0, -16.0])
_OFFSETS_BULK = np.array([0.0, 0.3, 1.0, 3.0, -0.3, -1.0, -3.0, 0.0, 0.3, -1.0, 3.0, -3.0, 1.0, -0.3, 0.0, -0.3])


def x_start_of(B, n, salt):
    """x_start in [-1, 1] with exactly +-1, +-0.999 and one ulp either side placed in every sample (as many as fit)"""
    xs = det_uniform((B, n), salt + "_xs", -1.0, 1.0).numpy().copy()
    for b in range(B):
        for k in range(min(8, n)):
            xs[b, (k * 5 + b) % n if n >= 40 else k] = EDGE_X[(k + b) % 8]
    return xs


def offsets_of(B, n, salt, saturated=True):
    """offsets in sigma by regime: 0, 0.3, 1, 3 (+ up to 0.05 jitter) and, where ``saturated``, 1 in 8 beyond +-14"""
    i = (np.arange(B * n) * 7 + 3).reshape(B, n) % 16
    base = (_OFFSETS if saturated else _OFFSETS_BULK)[i]
    jit = det_uniform((B, n), salt + "_jit", 0.0, 0.05).numpy().astype(np.float64)
    return base + np.sign(base) * jit * np.where(np.abs(base) > 10, 80.0, 1.0)


def metric_inputs(B, n, salt):
    """(x, means, log_scales) [B, n] float32 of the dgll metric: log_scales in [-6, 1], offsets by regime"""
    x = x_start_of(B, n, salt)
    ls = det_uniform((B, n), salt + "_ls", -6.0, 1.0).numpy()
    means = (x.astype(np.float64) - offsets_of(B, n, salt) * np.exp(ls.astype(np.float64))).astype(f32)
    return x, means, ls


def loss_inputs(tab32, t, B, n, salt, eps_mode, var, quant=False):
    """x_start, x_t, noise, model_out ([B, 2n]: mean half | variance half; [B, n] with a fixed variance) float32.  The variance
    values span log-scales of [-6, 1] (LEARNED: v in [-12, 2]; the float32 rounding of the model mean, which grows as 1/sigma in
    units of sigma, is what ``_propagated`` adds to the bounds) or v in [-1, 1] (LEARNED_RANGE).  The mean half
    puts the model mean at x_start + offset * sigma by regime.

    ``quant``: inputs for the dynamic threshold x0 -> clamp(x0, -s, s) / s, s = max(quantile(|x0|, 0.9), 1), which would scatter the
    offsets.  Samples at t > 0 take a wide x0 (s > 1) and solve x_t for the model mean of the thresholded x0; samples at t == 0
    (coef2 == 0: the model mean is the thresholded x0 itself) take x0 = clip(x_start + offset * sigma, -1, 1), |offset| <= 3, so s == 1
    and the clamp only shrinks offsets inside the bounded regime."""
    r = rows_at(T64, tab32, t)
    xs = x_start_of(B, n, salt)
    noise = det_normal((B, n), salt + "_noise").numpy()
    xs64 = T64.a(xs)
    xt = r["sqrt_abar"] * xs64 + torch.sqrt(r["1m_abar"]) * T64.a(noise)
    v = None
    if var is not None:
        v = det_uniform((B, n), salt + "_v", -12.0, 2.0).numpy() if var == LEARNED else det_uniform((B, n), salt + "_v", -1.0, 1.0).numpy()
    lv2 = _logvar(T64, r, None if v is None else T64.a(v), var)
    sigma = torch.exp(0.5 * lv2).expand(B, n)
    t0 = torch.from_numpy(r["t0"])
    if not quant:
        mm = xs64 + torch.from_numpy(offsets_of(B, n, salt)) * sigma
        x0 = (mm - r["coef2"] * xt) / r["coef1"]
    else:
        wide = 1.5 * T64.a(det_normal((B, n), salt + "_x0").numpy())
        s = torch.quantile(wide.abs(), 0.9, dim=1, keepdim=True).clamp(min=1.0)
        mm = xs64 + torch.from_numpy(offsets_of(B, n, salt)) * sigma
        xt_solved = (mm - r["coef1"] * (wide.clamp(-s, s) / s)) / torch.where(t0, 1.0, r["coef2"])
        xt = torch.where(t0, xt, xt_solved)
        mm0 = (xs64 + torch.from_numpy(offsets_of(B, n, salt, False)) * sigma).clamp(-1.0, 1.0)
        x0 = torch.where(t0, (mm0 - r["coef2"] * xt) / r["coef1"], wide)
    m = (r["sqrt_recip"] * xt - x0) / r["sqrt_recipm1"] if eps_mode else x0
    mo = m.numpy().astype(f32) if v is None else np.concatenate([m.numpy().astype(f32), v], axis=1)
    return xs, xt.numpy().astype(f32), noise, np.ascontiguousarray(mo)


def ratio(err, cond):
    """worst error / (u * condition term) over the elements with a nonzero condition term"""
    err, cond = np.abs(np.asarray(err, dtype=np.float64)).ravel(), np.asarray(cond, dtype=np.float64).ravel()
    ok = cond > 0
    return float((err[ok] / (U * cond[ok])).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- the cases
T = 20
MEANS, VARS = ("START_X", "EPSILON"), (LEARNED, LEARNED_RANGE)
# (per_sample, batch, t): per-sample sizes from gd_chunks and GD_THREADS = 256: one thread .. one element past a workgroup; 1023 V = 1
# with a ragged end; 1024 / 1028 V = 4, 1028's second chunk holding one float4; 65 795 = 257 * 256 + 3: 258 chunks, so
# gd_sum_partials makes a second trip (odd: V = 1); 263 172 = 4 * 65 793 the same for V = 4; 524 549 > 2048 * 256: a second
# grid-stride trip.  t mixes 0, a middle step and T - 1.
CASES = ((1, 5, (0, 10, 19, 0, 7)), (3, 3, (10, 0, 19)), (255, 1, (0,)), (256, 3, (0, 10, 19)), (257, 5, (19, 0, 7, 0, 10)),
         (1023, 3, (0, 10, 19)), (1024, 5, (0, 10, 19, 0, 7)), (1028, 3, (19, 0, 10)), (1028, 1, (10,)),
         (65795, 1, (0,)), (263172, 1, (0,)), (524549, 1, (10,)))
CASE_IDS = [f"n{n}_B{b}" for n, b, _ in CASES]
PRIOR_CASES = (1, 5, 8, 9, 11)                       # indices into CASES: the sizes the prior term runs at


def prior_inputs(ci):
    n, B, _ = CASES[ci]
    return x_start_of(B, n, f"gdl_prior_{n}")


def tables():
    """the pipeline's own packed float32 table, T = 20 (the learned kinds read the same rows; model_logvar is FIXED_LARGE's)"""
    from rho_diffusion_amd.diffusion.gaussian_diffusion import diffusion_tables, gd_table_rows_learned, get_named_beta_schedule
    return gd_table_rows_learned(diffusion_tables(get_named_beta_schedule("cosine", T)))


def case_inputs(ci, mean, var, quant=False):
    n, B, t = CASES[ci]
    t = np.asarray(t, dtype=np.int64)
    return (t,) + loss_inputs(tables(), t, B, n, f"gdl_{n}_{B}_{mean}_{var}", mean == "EPSILON", var, quant)


def upstream(B, which):
    """per-sample upstream gradients: g_loss alone (``which`` = 1) or g_loss, g_mse, g_vb (3), a different value per sample"""
    g = [(0.25 + 0.5 * np.arange(B)).astype(f32), (1.5 - 0.125 * np.arange(B)).astype(f32), (-0.75 + 0.375 * np.arange(B)).astype(f32)]
    return tuple(g[:which]) + (None,) * (3 - which)


# per_sample = 35: the i / n gather of a per-sample operand with a non-power of two; 3 * 349 551 = 1 048 653 elements: past 4096 * 256,
# so the flat kernels make a second grid-stride trip
METRIC_SHAPES = ((3, 35), (3, 349551))
DGLL_MODES = ((0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 0, 0), (2, 1, 0), (0, 1, 2))
KL_MODES = ((0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 2, 2), (1, 1, 0, 0), (2, 2, 1, 1), (0, 2, 1, 0))


def _operand(mode, full, b):
    """an operand in mode 0 (full [B, n]), 1 (per sample [B, 1]: column b of ``full``) or 2 (scalar: element b of row 0)"""
    return full if mode == 0 else (np.ascontiguousarray(full[:, b:b + 1]) if mode == 1 else full[0, b])


def metric_mode_operands(B, n, kind):
    """[(modes, operands)] of every operand mode of rho_discretized_gaussian_ll ('dgll': log-scales in [-1, 1] and means within
    0.3 of x, so every element is in the bounded regime whatever is broadcast) or rho_normal_kl ('kl')"""
    salt = f"gdm_modes_{B}_{n}"
    out = []
    if kind == "dgll":
        x = x_start_of(B, n, salt)
        ls = det_uniform((B, n), salt + "_ls", -1.0, 1.0).numpy()
        dm = det_uniform((B, n), salt + "_dm", -0.3, 0.3).numpy()
        for modes in DGLL_MODES:
            xo = _operand(modes[0], x, 2 if modes[0] == 1 else 4)              # x_start_of puts edge values in the first columns
            means = (xo + dm).astype(f32) if modes[0] else (x * f32(0.9)).astype(f32)
            out.append((modes, (xo, _operand(modes[1], means, 1), _operand(modes[2], ls, 3))))
        return out
    full = [det_uniform((B, n), f"{salt}_{k}", lo, hi).numpy() for k, (lo, hi) in enumerate(((-2, 2), (-6, 2), (-2, 2), (-6, 2)))]
    return [(modes, tuple(_operand(md, full[k], k) for k, md in enumerate(modes))) for modes in KL_MODES]


def cdf_inputs(n=1048653):
    """sorted float32 arguments over [-16, 16] (n of them: a second grid-stride trip), +-12 among them"""
    u = np.linspace(-16.0, 16.0, n).astype(f32)
    u[np.searchsorted(u, f32(-12.0))] = -12.0
    u[np.searchsorted(u, f32(12.0))] = 12.0
    assert np.all(np.diff(u) >= 0)
    return u
