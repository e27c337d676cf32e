"""The step side of csrc/gaussian.hip (k_gd_affine, k_gd_posterior, k_gd_ddim) and the two older step kernels of csrc/select.hip
(k_ddim_step, k_ddpm_sched_step) restated once and evaluated in three arithmetics (importable without a GPU; the sibling of
gd_loss_ref.py, whose T64, N32, rows_at, _x0, _logvar and tables() it uses):

  * ``N32``: numpy float32 in the kernels' own operation order, one rounding per operation, no contraction.  Its exp is the correctly
    rounded one (float64 exp, rounded once): what the device computes up to the ulps of its expf.
  * ``T64``: the same expression in torch float64 on the float32 inputs and the float32 table rows.
  * ``E64``: T64's value together with a bound on |float32 result - value| (running_error.py): every +, -, *, /, sqrt adds
    u = 2^-24 times the magnitude of its result to the first-order propagation of its operands' bounds; expf counts as 2 ulps, that is
    4 u relative (the allowance the attention bounds give exp2; the HIP math documentation lists expf at 1 ulp), plus exp(v) * expm1(e)
    for an argument known to within e.  min, max, clamp against exact limits and negation are exact.  No constant comes from the
    observed error of a kernel.

The t == 0 mask comes from the raw t, the table row from t clamped to [0, T): what gd_coef does.

What has no transcendental is compared bit for bit with N32 on the device: all of ``affine``, ``ddim``, ``ddim_uniform`` and
``sched_step``, ``pred_xstart``, ``log_variance`` (LEARNED: the input itself; LEARNED_RANGE: two products and a sum), and ``out`` of the
posterior step wherever no expf enters (no noise, and no grad with a learned variance).  The outputs behind expf (``out`` with the
noise term or with exp(logvar) * grad, ``variance``) are bounded against T64 by E64's bound.  For the bit-exact quantities E64's bound
is the operation-by-operation form of k u sum |terms| (k the rounding count): test_gd_step_ref_host.py holds N32 to it, and for the
bounded quantities to the bound taken with expf at 2 u (``expf_allowance``): the arithmetic part in full, half of the expf allowance.
Half of the whole bound is out of reach of any float32 evaluation where the rounding of a log-variance of magnitude ~10 dominates
it (the figures are in that module's docstring).

``fma=True`` (N32 only) is the contracted variant: every a*x +- b*y computed in float64 and rounded once.  ``mut`` names one wrong
kernel (MUTATIONS): the host twin shows that the inputs chosen here tell each from the right one."""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch

from detdata import det_normal, det_uniform
from gd_loss_ref import LEARNED, LEARNED_RANGE, N32, T, T64, U, _logvar, _x0, f32, rows_at, tables
from running_error import B, add, div, mul, sqrt as _sqrt_b, sub

GD_THREADS, GD_TARGET_WGS, FLAT_GRID = 256, 2048, 4096
FIXED_LARGE, FIXED_SMALL = "FIXED_LARGE", "FIXED_SMALL"
MEANS = ("START_X", "EPSILON")
VARS = (FIXED_LARGE, FIXED_SMALL, LEARNED, LEARNED_RANGE)
MUTATIONS = ("swap_abar", "swap_coef", "row_b1", "mask_clamped", "div_first", "var_stride_n", "grad_half")
_EXTRA_ROWS = ("model_var", "abar", "abar_prev", "abar_next")


# ---------------------------------------------------------------------------------------------------------------- the third arithmetic
class Bv(B):
    """a (value, bound) pair with operators, so the expressions below are written once for all three arithmetics"""

    def __add__(self, o):
        return _w(add(self, o))

    def __sub__(self, o):
        return _w(sub(self, o))

    def __mul__(self, o):
        return _w(mul(self, o))

    def __truediv__(self, o):
        return _w(div(self, o))

    def __neg__(self):
        return Bv(-self.v, self.e)


def _w(b):
    return Bv(b.v, b.e)


class E64:
    exp_u = 4.0                                                          # expf's allowance in units of u (2 ulps); see expf_allowance

    @staticmethod
    def a(v):
        return Bv(T64.a(v))

    @staticmethod
    def c(x):
        return Bv(float(x))

    k = c

    @staticmethod
    def clamp(v, lo, hi):                                                # the limits are exact here (s = max(q, 1), clip)
        assert not bool(lo.e.any()) and not bool(hi.e.any())
        return Bv(torch.minimum(torch.maximum(v.v, lo.v), hi.v), v.e)


def _exp(A, x):
    if A is E64:
        v = torch.exp(x.v)
        p = v * torch.expm1(x.e)
        return Bv(v, p + E64.exp_u * U * (v + p))
    if A is N32:
        return np.exp(x.astype(np.float64)).astype(f32)
    return torch.exp(x)


@contextlib.contextmanager
def expf_allowance(units):
    """E64 with expf counted at ``units`` * u: 4 for the device; the host twin holds N32, whose exp is correctly rounded (1 u), to 2"""
    keep, E64.exp_u = E64.exp_u, float(units)
    try:
        yield
    finally:
        E64.exp_u = keep


def _sqrt(A, x):
    return _w(_sqrt_b(x)) if A is E64 else (np.sqrt(x) if A is N32 else torch.sqrt(x))


def value(A, v, shape):
    """a result of arithmetic A as a contiguous array / tensor of ``shape`` (per-sample results broadcast): float32 numpy for N32,
    float64 torch for T64; (value, bound) float64 torch for E64"""
    if A is N32:
        return np.ascontiguousarray(np.broadcast_to(v, shape)).astype(f32, copy=False)
    if A is E64:
        return v.v.expand(shape).contiguous(), v.e.expand(shape).contiguous()
    return v.expand(shape).contiguous()


# ---------------------------------------------------------------------------------------------------------------- shared pieces
def _row(A, tab32, name, tc):
    from rho_diffusion_amd.engine.ops import GD_ROW
    return A.a(np.ascontiguousarray(tab32[GD_ROW[name]][tc].reshape(-1, 1)))


def step_rows(A, tab32, t, mut=None):
    """the float32 rows at t clamped to [0, T) as [B, 1] operands; ``t0`` and ``nmask`` = 1 - (t == 0) from the raw t"""
    t = np.asarray(t, dtype=np.int64)
    tc = np.clip(t, 0, tab32.shape[1] - 1)
    if mut == "row_b1":
        tc = np.roll(tc, -1)
    r = rows_at(A, tab32, tc)
    for k in _EXTRA_ROWS:
        r[k] = _row(A, tab32, k, tc)
    r["t0"] = ((np.clip(t, 0, tab32.shape[1] - 1) if mut == "mask_clamped" else t) == 0).reshape(-1, 1)
    r["nmask"] = A.a(np.where(r["t0"], 0.0, 1.0).astype(f32))
    return r


def _axpby(A, a, x, b, y, sign, fma):
    """a*x + sign * b*y: two products and a sum, or (``fma``, N32 only) evaluated in float64 and rounded once"""
    if fma:
        assert A is N32
        p0, p1 = np.asarray(a, np.float64) * np.asarray(x, np.float64), np.asarray(b, np.float64) * np.asarray(y, np.float64)
        return (p0 + p1 if sign > 0 else p0 - p1).astype(f32)
    p0, p1 = a * x, b * y
    return p0 + p1 if sign > 0 else p0 - p1


def _s(A, quant):
    """s = max(quantile[b], 1) as a [B, 1] operand (exact), or None"""
    return None if quant is None else A.a(np.maximum(np.asarray(quant, dtype=f32), f32(1.0)).reshape(-1, 1))


def _pred_x0(A, r, xt, m, eps_mode, s, fma=False, mut=None):
    if not fma and mut != "div_first":
        return _x0(A, r, xt, m, eps_mode, s)
    x0 = _axpby(A, r["sqrt_recip"], xt, r["sqrt_recipm1"], m, -1, fma) if eps_mode else m
    if s is not None:
        x0 = A.clamp(x0 / s, -s, s) if mut == "div_first" else A.clamp(x0, -s, s) / s
    return x0


# ---------------------------------------------------------------------------------------------------------------- the five kernels
AFFINE_OPS = ("ax", "ax+by", "ax-by", "(ax-y)/b")
AFFINE_ROWS = (("sqrt_abar", None), ("sqrt_abar", "1m_abar"), ("sqrt_recip", "sqrt_recipm1"), ("sqrt_recip", "sqrt_recipm1"))


def affine(A, tab32, t, x, y, row_a, row_b, op, fma=False, mut=None):
    """k_gd_affine: a[t]*x | a[t]*x + b[t]*y | a[t]*x - b[t]*y | (a[t]*x - y) / b[t]"""
    t = np.asarray(t, dtype=np.int64)
    tc = np.clip(t, 0, tab32.shape[1] - 1)
    if mut == "row_b1":
        tc = np.roll(tc, -1)
    a, x = _row(A, tab32, row_a, tc), A.a(x)
    if op == 0:
        return a * x
    b, y = _row(A, tab32, row_b, tc), A.a(y)
    if mut == "swap_coef":
        a, b = b, a
    if op == 3:
        return _axpby(A, a, x, A.c(1.0), y, -1, fma) / b if fma else (a * x - y) / b
    return _axpby(A, a, x, b, y, 1 if op == 1 else -1, fma)


def posterior(A, tab32, t, xt, m, eps_mode, var=None, v=None, quant=None, grad=None, noise=None, fma=False, mut=None):
    """k_gd_posterior: dict(out, pred_xstart) and, with a learned variance (``var`` LEARNED / LEARNED_RANGE, values ``v``), variance and
    log_variance.  A fixed variance reads the model_var / model_logvar rows of ``tab32``."""
    var = var if var in (LEARNED, LEARNED_RANGE) else None
    r = step_rows(A, tab32, t, mut)
    xt, m = A.a(xt), A.a(m)
    x0 = _pred_x0(A, r, xt, m, eps_mode, _s(A, quant), fma, mut)
    lv = _logvar(A, r, None if var is None else A.a(v), var)
    c1, c2 = (r["coef2"], r["coef1"]) if mut == "swap_coef" else (r["coef1"], r["coef2"])
    mean = _axpby(A, c1, x0, c2, xt, 1, fma)
    if grad is not None:
        sc = r["model_var"] if var is None else _exp(A, A.c(0.5) * lv if mut == "grad_half" else lv)
        mean = mean + sc * A.a(grad)
    if noise is not None:
        mean = mean + (r["nmask"] * _exp(A, A.c(0.5) * lv)) * A.a(noise)
    out = {"out": mean, "pred_xstart": x0}
    if var is not None:
        out.update(variance=_exp(A, lv), log_variance=lv)
    return out


def ddim(A, tab32, t, xt, m, eps_mode, quant=None, grad=None, noise=None, eta=0.0, reverse=False, fma=False, mut=None):
    """k_gd_ddim: dict(sample, pred_xstart)"""
    r = step_rows(A, tab32, t, mut)
    xt, m = A.a(xt), A.a(m)
    one, sr, srm1, ab = A.c(1.0), r["sqrt_recip"], r["sqrt_recipm1"], r["abar"]
    prev, nxt = ("abar_next", "abar_prev") if mut == "swap_abar" else ("abar_prev", "abar_next")
    sq1mab = _sqrt(A, one - ab)
    with np.errstate(divide="ignore", invalid="ignore"):                  # a mutated row may divide by abar_next[T - 1] = 0
        if reverse:
            abn = r[nxt]
            c_x0, c_eps, msig = _sqrt(A, abn), _sqrt(A, one - abn), None
        else:
            abp = r[prev]
            sigma = A.c(f32(eta)) * _sqrt(A, (one - abp) / (one - ab))
            sigma = sigma * _sqrt(A, one - ab / abp)
            c_x0, c_eps = _sqrt(A, abp), _sqrt(A, (one - abp) - sigma * sigma)
            msig = r["nmask"] * sigma
        x0 = _pred_x0(A, r, xt, m, eps_mode, _s(A, quant), fma, mut)
        ax = sr * xt
        if grad is not None:
            e = (ax - x0) / srm1
            e = e - sq1mab * A.a(grad)
            x0 = ax - srm1 * e
        eps = (ax - x0) / srm1
        v = _axpby(A, x0, c_x0, c_eps, eps, 1, fma)
        if noise is not None:
            v = v + msig * A.a(noise)
    return {"sample": v, "pred_xstart": x0}


def ddim_uniform(A, xt, m, quant, noise, coef, fma=False, mut=None):
    """k_ddim_step with the five host scalars of ddim_coefficients (c_recip, c_recipm1, sqrt_abar_prev, coef_eps, sigma_masked);
    the noise enters when sigma_masked != 0: dict(sample, pred_xstart)"""
    q = np.asarray(quant, dtype=f32)
    s = _s(A, np.roll(q, -1) if mut == "row_b1" else q)
    xt, m = A.a(xt), A.a(m)
    c = [A.c(f32(v)) for v in coef]
    x0 = A.clamp(m / s, -s, s) if mut == "div_first" else A.clamp(m, -s, s) / s
    ax = c[0] * xt
    eps = (ax - x0) / c[1]
    v = _axpby(A, x0, c[2], c[3], eps, 1, fma)
    if float(coef[4]) != 0.0:
        v = v + c[4] * A.a(noise)
    return {"sample": v, "pred_xstart": x0}


def sched_step(A, x, m, noise, eps_mode, sb, sa, clip, c0, c1, sigma, fma=False, mut=None):
    """k_ddpm_sched_step: dict(sample, pred_xstart).  sa == 0 (zero terminal SNR): +-inf, which the clamp maps to +-clip"""
    x, x0 = A.a(x), A.a(m)
    if mut == "swap_coef":
        c0, c1 = c1, c0
    if eps_mode:
        d = _axpby(A, A.c(1.0), x, A.c(f32(sb)), x0, -1, fma) if fma else x - A.c(f32(sb)) * x0
        if A is E64 and float(sa) == 0.0:
            assert clip > 0 and bool((d.v.abs() > d.e).all())             # the sign of the infinity is certain
            x0 = Bv(torch.where(d.v > 0, float(f32(clip)), -float(f32(clip))))
        else:
            with np.errstate(divide="ignore"):
                x0 = d / A.c(f32(sa))
    if clip > 0:
        lim = A.a(np.asarray(f32(clip)))
        x0 = A.clamp(x0, -lim, lim)
    v = _axpby(A, A.c(f32(c0)), x0, A.c(f32(c1)), x, 1, fma)
    if float(sigma) != 0.0:
        v = v + A.c(f32(sigma)) * A.a(noise)
    return {"sample": v, "pred_xstart": x0}


def exact_out(var, grad, noise) -> bool:
    """whether ``out`` of the posterior step has no expf in it: then it is compared bit for bit"""
    return noise is None and (grad is None or var in (None, FIXED_LARGE, FIXED_SMALL))


# ---------------------------------------------------------------------------------------------------------------- tables, inputs
@functools.lru_cache(maxsize=None)
def table(var=FIXED_LARGE) -> np.ndarray:
    """the packed float32 table, cosine, T = 20 (row T - 1 has the clipped beta, row 0 abar_prev = 1): gd_loss_ref.tables() (the
    learned kinds and FIXED_LARGE) or the FIXED_SMALL rows of the same schedule"""
    if var != FIXED_SMALL:
        return tables()
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType, diffusion_tables, gd_table_rows, get_named_beta_schedule
    return gd_table_rows(diffusion_tables(get_named_beta_schedule("cosine", T)), ModelVarType.FIXED_SMALL)


SCALES = (0.3, 2.5, 3.5)                                                  # per sample: quantiles below and above the threshold's 1


@functools.lru_cache(maxsize=8)
def step_inputs(B, n):
    """read-only float32 [B, n] arrays: x_t, the model's mean output (scaled per sample by 0.3, 2.5, 3.5), grad, noise, y, the
    variance values of LEARNED_RANGE in [-1.5, 1.5] (frac leaves [0, 1]) and of LEARNED in [-9, 1]"""
    salt = f"gds_{B}_{n}"
    sc = np.asarray(SCALES, dtype=f32)[np.arange(B) % 3].reshape(-1, 1)
    d = {"xt": det_normal((B, n), salt + "_xt").numpy(), "m": det_normal((B, n), salt + "_m").numpy() * sc,
         "grad": det_normal((B, n), salt + "_g").numpy() * f32(0.5), "noise": det_normal((B, n), salt + "_nz").numpy(),
         LEARNED_RANGE: det_uniform((B, n), salt + "_vr", -1.5, 1.5).numpy(), LEARNED: det_uniform((B, n), salt + "_vl", -9.0, 1.0).numpy()}
    for a in d.values():
        a.setflags(write=False)
    return d


def quantile_of(tab32, t, xt, m, eps_mode):
    """float32 [B]: torch.quantile(|x0|, 0.9) of the unthresholded x0, as the pipeline hands it to the step (rho_abs_quantile has its
    own tests; the step kernels take any value)"""
    x0 = np.broadcast_to(_x0(N32, step_rows(N32, tab32, t), xt, m, eps_mode), xt.shape)
    return torch.quantile(torch.from_numpy(np.array(x0)).abs(), 0.9, dim=1).numpy()


def merged(m, v):
    """[B, 2, n]: the mean half and the variance half of one learned-variance output"""
    return np.ascontiguousarray(np.stack([m, v], axis=1))


# ---------------------------------------------------------------------------------------------------------------- the cases
def gd_chunks(batch, per_sample):
    return max(1, min(-(-GD_TARGET_WGS // batch), -(-per_sample // GD_THREADS), 65535))


def flat_grid(total):
    return min(-(-total // GD_THREADS), FLAT_GRID)


def t_of(B, n=0, base=(0, 10, 19)):
    """t [B]: ``base`` for B = 3, its middle step for B = 1, else a cycle through all T rows"""
    if B == 1:                                                           # a middle row: at 0 and T - 1 one DDIM coefficient is exactly 0
        return np.asarray(base[1:2], dtype=np.int64)
    return np.asarray(base[:B] if B <= len(base) else np.arange(B) % T, dtype=np.int64)


SMALL_N = (1, 3, 255, 256, 257, 1029)
GRID_SMALL = tuple((3, n) for n in SMALL_N) + ((1, 1), (1, 257), (1, 1029))
GRID_TRIP2 = ((300, 1801), (2049, 700))                                   # 7 chunks then 9 elements; one chunk, three trips, ragged
GRID_LIMIT = (65535, 2)
FLAT_SMALL = tuple((3, n) for n in SMALL_N)
FLAT_TRIP2 = ((3, 349551),)                                               # 1 048 653 > 4096 * 256 elements
MODE_SHAPE = (3, 257)
STRIDE_SHAPE = (3, 1029)                                                  # odd n: every second row of [B, 2, n] is off 16 bytes
GRID_CASES = GRID_SMALL + GRID_TRIP2 + (GRID_LIMIT,)
FLAT_CASES = FLAT_SMALL + FLAT_TRIP2


def ids(cases):
    return [f"B{b}_n{n}" for b, n in cases]


def posterior_modes(B, n):
    """[(mean, quant, grad, noise, var)]: the full product at MODE_SHAPE, elsewhere four of them, one per variance kind, in which
    every value of every factor occurs; which four rotates with the size"""
    if (B, n) == MODE_SHAPE:
        return [(mean, q, g, z, var) for var in VARS for mean in MEANS for q in (False, True) for g in (False, True) for z in (False, True)]
    i = GRID_CASES.index((B, n))
    out = []
    for k in range(4):
        b0, b1 = k & 1, k >> 1
        out.append((MEANS[b0 ^ (i & 1)], bool(b1 ^ ((i >> 1) & 1)), bool(b0 ^ b1 ^ (i & 1)), bool(b0 ^ ((i >> 2) & 1)), VARS[(k + i) % 4]))
    return out


ETAS = ((0.0, False), (0.5, True), (1.0, True))                           # (eta, with noise)


def ddim_modes(B, n):
    """[(mean, quant, grad, eta, noise, reverse)]: the full product at MODE_SHAPE, elsewhere one per eta kind and one reverse"""
    if (B, n) == MODE_SHAPE:
        fw = [(mean, q, g, eta, z, False) for mean in MEANS for q in (False, True) for g in (False, True) for eta, z in ETAS]
        return fw + [(mean, q, False, 0.0, False, True) for mean in MEANS for q in (False, True)]
    i = GRID_CASES.index((B, n))
    out = [(MEANS[(k + i) & 1], bool(((k >> 1) + i) & 1), bool((((k + 1) >> 1) + i) & 1), ETAS[(k + i) % 3][0], ETAS[(k + i) % 3][1], False)
           for k in range(3)]
    return out + [(MEANS[(i >> 1) & 1], bool(i & 1), False, 0.0, False, True)]


def uniform_modes(B, n):
    """[(t, eta, with pred_xstart)] of rho_ddim_step: t = 0 (masked sigma), a middle step with and without noise, T - 1"""
    i = FLAT_CASES.index((B, n))
    return [(0, 0.5, True), (10, 0.0, bool(i & 1)), (10, 0.5, not (i & 1)), (19, 1.0, True)]


SCHED_T, SCHED_CLIP = 100, 0.5


@functools.lru_cache(maxsize=None)
def sched_coefficients(t, var="fixed_large"):
    """(sqrt_beta_prod, sqrt_alpha_prod, c0, c1, sigma) of a zero-terminal-SNR squaredcos_cap_v2 schedule, T = 100: at t = T - 1
    sqrt_alpha_prod == 0"""
    from rho_diffusion_amd.diffusion import DDPMScheduler
    sch = DDPMScheduler(num_train_timesteps=SCHED_T, beta_schedule="squaredcos_cap_v2", variance_type=var, rescale_betas_zero_snr=True)
    return sch.step_coefficients(t)


def sched_modes(B, n):
    """[(t, eps_mode, clip, with noise)]: eps / sample, clip > 0 / 0, t = T - 1 (division by 0, clamped; the sample form and clip = 0
    only where the quotient is finite), a middle step, t = 0 (sigma = 0)"""
    i = FLAT_CASES.index((B, n))
    return [(SCHED_T - 1, True, SCHED_CLIP, True), (57, True, 0.0, bool(i & 1)), (57, False, SCHED_CLIP, not (i & 1)), (0, False, 0.0, False),
            (SCHED_T - 1, False, 0.0, True), (0, True, SCHED_CLIP, False)]


def posterior_args(B, n, mode, t=None):
    """(table, t, eps_mode, keyword operands) of one posterior mode (mean, quant, grad, noise, var) on step_inputs(B, n)"""
    mean, q, g, z, var = mode
    d, t, tab, em = step_inputs(B, n), t_of(B, n) if t is None else np.asarray(t, dtype=np.int64), table(var), mean == "EPSILON"
    return tab, t, em, dict(var=var, v=d[var] if var in (LEARNED, LEARNED_RANGE) else None,
                            quant=quantile_of(tab, t, d["xt"], d["m"], em) if q else None, grad=d["grad"] if g else None,
                            noise=d["noise"] if z else None)


def ddim_args(B, n, mode, t=None):
    """the same of one DDIM mode (mean, quant, grad, eta, noise, reverse)"""
    mean, q, g, eta, z, rev = mode
    d, t, tab, em = step_inputs(B, n), t_of(B, n) if t is None else np.asarray(t, dtype=np.int64), table(), mean == "EPSILON"
    return tab, t, em, dict(quant=quantile_of(tab, t, d["xt"], d["m"], em) if q else None, grad=d["grad"] if g else None,
                            noise=d["noise"] if z else None, eta=eta, reverse=rev)


def uniform_args(B, n, mode):
    """(quantile [B], noise or None, the five scalars) of one rho_ddim_step mode (t, eta, with pred_xstart)"""
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ddim_coefficients, diffusion_tables, get_named_beta_schedule
    t, eta, _ = mode
    d = step_inputs(B, n)
    coef = ddim_coefficients(diffusion_tables(get_named_beta_schedule("cosine", T)), t, eta)
    quant = torch.quantile(torch.from_numpy(d["m"].copy()).abs(), 0.9, dim=1).numpy()
    return quant, d["noise"] if coef[4] != 0.0 else None, coef


def sched_args(B, n, mode):
    """(noise or None, eps_mode, sb, sa, clip, c0, c1, sigma) of one rho_ddpm_sched_step mode (t, eps_mode, clip, with noise): without
    noise sigma is passed as 0"""
    t, em, clip, z = mode
    sb, sa, c0, c1, sigma = sched_coefficients(t)
    z = z and sigma != 0.0
    return (step_inputs(B, n)["noise"] if z else None, em, sb, sa, clip, c0, c1, sigma if z else 0.0)


def err_ratio(got, ref, bound):
    """worst |got - ref| / bound; an element with a zero bound must agree exactly (else inf)"""
    err = (torch.as_tensor(np.asarray(got, dtype=np.float64)).reshape(-1) - ref.reshape(-1)).abs_()
    b = bound.reshape(-1)
    r = torch.where(b > 0, err / b, torch.where(err == 0, 0.0, float("inf")))
    return float(r.max()) if bool(np.isfinite(np.asarray(got)).all()) else float("inf")
