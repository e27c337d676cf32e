"""-m gpu: the streaming kernels of the DDPM loops at the sizes, tails and alignments where such kernels go wrong.

Every kernel here is a grid-stride loop under a grid capped at 2048 blocks x 256 threads (4096 blocks for rho_q_sample_coef), most
with a 16-byte vector body, a scalar tail and a scalar fallback chosen from the pointers' alignment.  The sizes: 1 ... 1029 (below,
at and past a vector, a wave, a block) and one size per kernel that needs a SECOND trip of the loop and ends ragged.  Reference: the
same expression in float64 on the CPU, evaluated on the float32 inputs.  Two bars each: the rel-L2 the kernel's existing test uses,
and a per-element bound |got - ref| <= k * 2^-24 * sum |terms| with k counted from the roundings of the kernel's expression (rel-L2
over two million elements would not show a handful of wrong ones).  Every output and in-place operand sits between 64 sentinel
elements that must survive the launch; the operands offset by 4 bytes must give the bits of the aligned run."""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import det_normal, rel_l2
from gpu_util import DEV, Guarded, bits, check_bound, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of float32: one correctly rounded operation errs by at most U * |result|
SMALL = [1, 3, 4, 5, 255, 257, 1029]
WRAP4 = 2_100_227                  # > 2048 * 256 * 4: second trip of a 4-wide kernel, 3-element tail
WRAP1 = 525_065                    # > 2048 * 256: second trip of a scalar kernel
POOL = 2_100_228


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=None)
def _pool(salt: str) -> torch.Tensor:
    """POOL deterministic ~N(0, 1) float32 values on the CPU; tests take prefixes and never write to them."""
    return det_normal((POOL,), "edges_" + salt)


def _data(salt: str, n: int) -> torch.Tensor:
    return _pool(salt)[:n]


def _shift_sets(names):
    """Alignment variants: each operand alone offset by one element, then all of them."""
    return [frozenset([n]) for n in names] + [frozenset(names)]


# ----------------------------------------------------------------------------- q_sample / q_sample_coef
T = 1000


@functools.lru_cache(maxsize=None)
def _tables():
    from oracle import ref_torch as R
    sched = R.linear_schedule(T, 1e-3, 0.02)
    ab32 = sched["alpha_bar_t"].contiguous()
    scale = 1000 / T
    ab64 = (1.0 - torch.linspace(scale * 1e-3, scale * 0.02, T, dtype=torch.float64)).cumprod(0)
    return ab32, ab64.sqrt().float().contiguous(), (1.0 - ab64).sqrt().float().contiguous()


def _timesteps(B):
    return torch.tensor([(331 * i + 7) % T for i in range(B)])            # a different t per sample


Q_SHAPES = [(3, s) for s in SMALL] + [
    (3, 700004),     # vector path, total4 = 525003 > 524288 threads: the batch index changes inside the second trip
    (3, 175023),     # per_sample % 4 != 0: the scalar kernel, second trip
]


def _q_run(hip, which, x0, eps, t, B, per, shifts=frozenset()):
    ab32, ca, cb = _tables()
    gx, ge = Guarded(x0, int("x0" in shifts)), Guarded(eps, int("eps" in shifts))
    out = Guarded(B * per, int("out" in shifts))
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    td = t.to(DEV)
    L = hip.lib()
    if which == "q_sample":
        tab = ab32.to(DEV)
        hip.check(L.rho_q_sample(gx.ptr, ge.ptr, out.ptr, tab.data_ptr(), td.data_ptr(), B, per, T, flag.data_ptr(), hip.stream()), which)
    else:
        a, b = ca.to(DEV), cb.to(DEV)
        hip.check(L.rho_q_sample_coef(gx.ptr, ge.ptr, out.ptr, a.data_ptr(), b.data_ptr(), td.data_ptr(), B, per, T, flag.data_ptr(),
                                      hip.stream()), which)
    res = out.cpu()
    assert int(flag.item()) == 0, which
    assert out.intact() and gx.intact() and ge.intact(), (which, B, per, sorted(shifts))
    assert torch.equal(gx.cpu(), x0) and torch.equal(ge.cpu(), eps)          # inputs are read only
    return res


def _q_ref(which, x0, eps, t, B, per):
    """(reference, per-element bound) in float64.
    q_sample:      sa = sqrtf(ab); sb = sqrtf(1 - ab); sa * x0 + sb * eps.  Longest chain of roundings into one element: 1 - ab,
                   sqrtf (correctly rounded; it halves the error it inherits, counted whole), the product, the sum: k = 4.
    q_sample_coef: ca * x0 + cb * eps from float32 tables: the product and the sum, k = 2."""
    ab32, ca, cb = _tables()
    x, e = x0.double().view(B, per), eps.double().view(B, per)
    if which == "q_sample":
        ab = ab32.double()[t].view(B, 1)
        a, b, k = ab.sqrt(), (1.0 - ab).sqrt(), 4
    else:
        a, b, k = ca.double()[t].view(B, 1), cb.double()[t].view(B, 1), 2
    return a * x + b * e, k * U * ((a * x).abs() + (b * e).abs())


@pytest.mark.parametrize("which", ["q_sample", "q_sample_coef"])
@pytest.mark.parametrize("B,per", Q_SHAPES)
def test_q_sample_sizes(hip, which, B, per):
    x0, eps, t = _data("qx0", B * per) * 0.5 + 0.5, _data("qeps", B * per), _timesteps(B)
    got = _q_run(hip, which, x0, eps, t, B, per)
    ref, bound = _q_ref(which, x0, eps, t, B, per)
    check_bound(got, ref, bound, (which, B, per), 1e-6)


# 1029 and 2100227 elements (odd: the scalar kernel either way); per_sample % 4 == 0 at 1032 elements and at the wrap shape, where
# the aligned run takes the 16-byte kernel and the offset runs the scalar one
@pytest.mark.parametrize("B,per", [(3, 343), (1, WRAP4), (3, 344), (3, 700004)])
def test_q_sample_alignment(hip, B, per):
    """rho_q_sample falls back to its scalar kernel when any pointer is not 16-byte aligned: same arithmetic, same bits (both
    kernels evaluate q_mix, fma(sa, x0, sb * eps); left to the compiler's contraction they differed in the last bit)."""
    x0, eps, t = _data("qx0", B * per) * 0.5 + 0.5, _data("qeps", B * per), _timesteps(B)
    base = _q_run(hip, "q_sample", x0, eps, t, B, per)
    ref, bound = _q_ref("q_sample", x0, eps, t, B, per)
    check_bound(base, ref, bound, ("aligned", B, per), 1e-6)
    for shifts in _shift_sets(["x0", "eps", "out"]):
        got = _q_run(hip, "q_sample", x0, eps, t, B, per, shifts)
        assert same_bits(got, base), (B, per, sorted(shifts))


# ----------------------------------------------------------------------------- p_sample_step
@functools.lru_cache(maxsize=None)
def _coef():
    from rho_diffusion_amd.diffusion.schedule import LinearSchedule
    return LinearSchedule(T, 1e-3, 0.02).device_tables("cpu")["coef"].clone()       # float32 [T, 3]


def _p_run(hip, x, eh, z, t, shifts=frozenset()):
    gx, ge = Guarded(x, int("x" in shifts)), Guarded(eh, int("eh" in shifts))
    gz = Guarded(z, int("z" in shifts)) if z is not None else None
    coef = _coef().to(DEV)
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    hip.check(hip.lib().rho_p_sample_step(gx.ptr, ge.ptr, gz.ptr if gz else None, coef.data_ptr(), t_dev.data_ptr(), x.numel(),
                                          hip.stream()), "rho_p_sample_step")
    res = gx.cpu()
    assert gx.intact() and ge.intact() and (gz is None or gz.intact()), (x.numel(), t, sorted(shifts))
    assert torch.equal(ge.cpu(), eh) and (gz is None or torch.equal(gz.cpu(), z))
    assert int(t_dev.item()) == t
    return res


def _p_ref(x, eh, z, t):
    """clamp(c0 * (x - c1 * eh) + c2 * z, -1, 1) with the float32 table row of t; z is dropped for t <= 1 or z = None.
    Longest chain of roundings: c1 * eh, the difference, its product with c0, the sum with c2 * z: k = 4 (the clamp is exact and
    1-Lipschitz)."""
    c0, c1, c2 = (float(v) for v in _coef()[t].double())
    x, e = x.double(), eh.double()
    zz = z.double() * c2 if (z is not None and t > 1) else torch.zeros_like(x)
    ref = (c0 * (x - c1 * e) + zz).clamp(-1.0, 1.0)
    return ref, 4 * U * (abs(c0) * (x.abs() + (c1 * e).abs()) + zz.abs())


@pytest.mark.parametrize("n", SMALL + [WRAP4])
def test_p_sample_step_sizes(hip, n):
    x, eh, z = _data("px", n) * 0.7, _data("pe", n), _data("pz", n)
    for t, zz in ((500, z), (1, z), (500, None), (2, z)):
        got = _p_run(hip, x, eh, zz, t)
        ref, bound = _p_ref(x, eh, zz, t)
        check_bound(got, ref, bound, ("p_sample_step", n, t, zz is not None), 2e-6)
        assert (got != x).any()
    assert same_bits(_p_run(hip, x, eh, z, 0), x)                            # t = 0: no update
    assert same_bits(_p_run(hip, x, eh, None, 0), x)


@pytest.mark.parametrize("n", [1029, WRAP4])
def test_p_sample_step_alignment(hip, n):
    """The 4-byte-aligned fallback against the 16-byte body + tail: the same bits (all are loops of step_walk over PSampleOp)."""
    x, eh, z = _data("px", n) * 0.7, _data("pe", n), _data("pz", n)
    base = _p_run(hip, x, eh, z, 500)
    ref, bound = _p_ref(x, eh, z, 500)
    check_bound(base, ref, bound, ("aligned", n), 2e-6)
    for shifts in _shift_sets(["x", "eh", "z"]):
        assert same_bits(_p_run(hip, x, eh, z, 500, shifts), base), (n, sorted(shifts))
        assert same_bits(_p_run(hip, x, eh, z, 0, shifts), x), (n, sorted(shifts))


# ----------------------------------------------------------------------------- mse (scratch of its own), mse_ws (caller's scratch)
def _mse_ref(a, b):
    """loss = mean((a - b)^2); grad = 2 (a - b) / n.  Roundings into one gradient element: the difference, 1.0f / n, the product
    with it (the factor 2 is exact): k = 3."""
    n = a.numel()
    d = a.double() - b.double()
    return float((d * d).mean()), 2.0 * d / n, 3 * U * 2.0 * (a.double().abs() + b.double().abs()) / n


def _mse_run(hip, form, a, b, shifts=frozenset(), want_grad=True):
    n = a.numel()
    ga, gb = Guarded(a, int("a" in shifts)), Guarded(b, int("b" in shifts))
    gg = Guarded(n, int("grad" in shifts)) if want_grad else None
    loss, part = Guarded(1), Guarded(1024)
    L = hip.lib()
    if form == "mse":
        hip.check(L.rho_mse(ga.ptr, gb.ptr, loss.ptr, gg.ptr if gg else None, n, hip.stream()), "rho_mse")
    else:
        hip.check(L.rho_mse_ws(ga.ptr, gb.ptr, loss.ptr, gg.ptr if gg else None, n, part.ptr, 1024, hip.stream()), "rho_mse_ws")
    res = float(loss.cpu().item()), (gg.cpu() if gg else None)
    assert ga.intact() and gb.intact() and loss.intact() and part.intact() and (gg is None or gg.intact()), (form, n, sorted(shifts))
    assert torch.equal(ga.cpu(), a) and torch.equal(gb.cpu(), b)
    return res


@pytest.mark.parametrize("form", ["mse", "mse_ws"])
@pytest.mark.parametrize("n", SMALL + [WRAP4])
def test_mse_sizes(hip, form, n):
    from rho_diffusion_amd.engine import ops
    a, b = _data("ma", n), _data("mb", n)
    ref_loss, ref_grad, bound = _mse_ref(a, b)
    loss, grad = _mse_run(hip, form, a, b)
    print(f"{form} n={n}: |loss - ref| = {abs(loss - ref_loss):.3e}")
    assert abs(loss - ref_loss) < 1e-6, (form, n, loss, ref_loss)
    check_bound(grad, ref_grad, bound, (form, n), 1e-6)
    loss2, none = _mse_run(hip, form, a, b, want_grad=False)                  # the loss alone
    assert none is None and abs(loss2 - ref_loss) < 1e-6
    if form == "mse_ws":
        assert loss2 == loss                                                  # ordered reduction: the same bits with and without grad
        l3, g3 = ops.mse(a.to(DEV), b.to(DEV), want_grad=True)                # the wrapper the pipelines call
        assert float(l3.item()) == loss and same_bits(g3, grad)


@pytest.mark.parametrize("n", [1029, WRAP4])
def test_mse_ws_alignment(hip, n):
    """rho_mse_ws takes its 16-byte path only when a, b and grad are all aligned: the gradient is the same bits either way, the
    loss may differ by summation order."""
    a, b = _data("ma", n), _data("mb", n)
    ref_loss, ref_grad, bound = _mse_ref(a, b)
    _, base = _mse_run(hip, "mse_ws", a, b)
    for shifts in _shift_sets(["a", "b", "grad"]):
        loss, grad = _mse_run(hip, "mse_ws", a, b, shifts)
        assert abs(loss - ref_loss) < 1e-6, (n, sorted(shifts), loss, ref_loss)
        assert same_bits(grad, base), (n, sorted(shifts))
    check_bound(base, ref_grad, bound, ("aligned", n), 1e-6)


# ----------------------------------------------------------------------------- mean_flat
@pytest.mark.parametrize("B,per", [(1, 1), (3, 255), (2, 257), (5, 100003)])
def test_mean_flat_sizes(hip, B, per):
    """One workgroup per sample: thread i adds elements i, i + 256, ... in float32, then a 6-level wave butterfly, the sum of the
    four waves in two levels, one division.  Additions on the longest path to the result: ceil(per / 256) - 1 + 6 + 2, plus the
    division: |got - ref| <= (ceil(per / 256) + 8) * 2^-24 * mean |x|."""
    x = _data("mf", B * per)
    gx, out = Guarded(x), Guarded(B)
    hip.check(hip.lib().rho_mean_flat(gx.ptr, out.ptr, B, per, hip.stream()), "rho_mean_flat")
    assert out.intact() and gx.intact() and torch.equal(gx.cpu(), x)
    xd = x.double().view(B, per)
    k = math.ceil(per / 256) + 8
    check_bound(out.cpu(), xd.mean(1), k * U * xd.abs().mean(1), ("mean_flat", B, per))
    from rho_diffusion_amd.engine import ops
    assert same_bits(ops.mean_flat(x.view(B, per).to(DEV)), out.cpu())       # fixed summation order: reproducible bits


# ----------------------------------------------------------------------------- adamw
@pytest.mark.parametrize("n", SMALL + [WRAP1])
def test_adamw_sizes(hip, n):
    """Three steps against float64 AdamW with the float32 hyperparameters the ABI receives.  Per step and element, roundings:
      m = b1 * m + (1 - b1) * g                 product, 1 - b1, product, sum: 4, on top of b1 times the error m carried in
      v = b2 * v + (1 - b2) * g * g             one more product: 5, likewise
      p = p * (1 - lr * wd) - (lr / bc1) * (m / (sqrtf(v) * rsqrt_bc2 + eps))
          decay: lr * wd, 1 - ., product: 3 on |p|;  update u: bc1 and rsqrt_bc2 are float32 casts (2), lr / bc1 (1), sqrtf (1, and
          half of v's <= 15), two more in the denominator (2), the quotient and the product (2), m's own <= 12: under 28 on |u| with
          m taken as the same recurrence over |g|;  the final difference: 1 on |p| + |u|."""
    lr, b1, b2, eps, wd = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 1e-2))
    p0 = _data("adam_p", n)
    gp, gm, gv = Guarded(p0), Guarded(torch.zeros(n)), Guarded(torch.zeros(n))
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    m_abs, em, ev, ep = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        g32 = _data(f"adam_g{step}", n)
        gg = Guarded(g32)
        hip.check(hip.lib().rho_adamw(gp.ptr, gg.ptr, gm.ptr, gv.ptr, n, lr, b1, b2, eps, wd, step, hip.stream()), "rho_adamw")
        assert gp.intact() and gm.intact() and gv.intact() and gg.intact() and torch.equal(gg.cpu(), g32), (n, step)
        g = g32.double()
        m = b1 * m + (1 - b1) * g
        m_abs = b1 * m_abs + (1 - b1) * g.abs()
        v = b2 * v + (1 - b2) * g * g
        em = b1 * em + 4 * U * m_abs
        ev = b2 * ev + 5 * U * v
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        denom = v.sqrt() / math.sqrt(bc2) + eps
        upd_abs = (lr / bc1) * m_abs / denom
        ep = ep + 4 * U * p.abs() + 29 * U * upd_abs
        p = p * (1 - lr * wd) - (lr / bc1) * m / denom
        check_bound(gm.cpu(), m, em, ("adamw m", n, step), 1e-6)
        check_bound(gv.cpu(), v, ev, ("adamw v", n, step), 1e-6)
        check_bound(gp.cpu(), p, ep, ("adamw p", n, step), 1e-6)
    assert rel_l2(gp.cpu(), p0) > 1e-4                                        # the parameters moved


# ----------------------------------------------------------------------------- ema_update
OMF = float(np.float32(1.0 - 0.999))


def _ema_run(hip, s, p, shifts=frozenset()):
    gs, gp = Guarded(s, int("shadow" in shifts)), Guarded(p, int("param" in shifts))
    hip.check(hip.lib().rho_ema_update(gs.ptr, gp.ptr, s.numel(), OMF, hip.stream()), "rho_ema_update")
    assert gs.intact() and gp.intact() and torch.equal(gp.cpu(), p), (s.numel(), sorted(shifts))
    return gs.cpu()


def _ema_ref(s, p):
    """float32, in the kernel's operation order: d = s - p; d = omf * d; s - d."""
    omf = torch.tensor(OMF, dtype=torch.float32)
    d = s - p
    d = omf * d
    return s - d


@pytest.mark.parametrize("n", SMALL + [WRAP4])
def test_ema_update_sizes(hip, n):
    s, p = _data("ema_s", n), _data("ema_p", n)
    got, ref = _ema_run(hip, s, p), _ema_ref(s, p)
    assert ref.dtype == torch.float32 and not torch.equal(ref, s)
    assert same_bits(got, ref), (n, int((bits(got) != bits(ref)).sum()))


@pytest.mark.parametrize("n", [1029, WRAP4])
def test_ema_update_alignment(hip, n):
    s, p = _data("ema_s", n), _data("ema_p", n)
    ref = _ema_ref(s, p)
    for shifts in [frozenset()] + _shift_sets(["shadow", "param"]):
        assert same_bits(_ema_run(hip, s, p, shifts), ref), (n, sorted(shifts))


# ----------------------------------------------------------------------------- add_inplace
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", SMALL + [WRAP4 + 1])
def test_add_inplace_sizes(hip, dtype, n):
    """dst += src in whole 16-byte pieces.  A ragged n is refused and nothing is written; the size rounded up to whole pieces (for
    the wrap size: 2100228 float32, 4200456 bfloat16 - a second trip of the piece loop) must be exact: float32 one rounding like
    torch's; bfloat16 the float32 sum of the operands rounded once to bfloat16."""
    from rho_diffusion_amd.hip import RHO_BF16, RHO_F32
    pe, code = (8, RHO_BF16) if dtype == torch.bfloat16 else (4, RHO_F32)
    if n > 1029:
        n = n * (pe // 4)
    L = hip.lib()
    if n % pe:
        dst, src = Guarded(_data("add_d", n).to(dtype)), Guarded(_data("add_s", n).to(dtype))
        before = dst.cpu()
        assert L.rho_add_inplace(dst.ptr, src.ptr, code, n, hip.stream()) == -1            # RHO_E_ARG
        assert same_bits(dst.cpu(), before) and dst.intact()
        n = (n + pe - 1) // pe * pe
    d0 = torch.cat([_data("add_d", min(n, POOL)), _data("add_d2", n - min(n, POOL))]).to(dtype)
    s0 = torch.cat([_data("add_s", min(n, POOL)), _data("add_s2", n - min(n, POOL))]).to(dtype)
    dst, src = Guarded(d0), Guarded(s0)
    hip.check(L.rho_add_inplace(dst.ptr, src.ptr, code, n, hip.stream()), "rho_add_inplace")
    assert dst.intact() and src.intact() and same_bits(src.cpu(), s0)
    ref = (d0.float() + s0.float()).to(dtype)
    assert same_bits(dst.cpu(), ref), (n, int((bits(dst.cpu()) != bits(ref)).sum()))
    assert not same_bits(ref, d0)


# ----------------------------------------------------------------------------- scale_by_device_scalar
@pytest.mark.parametrize("n", SMALL + [WRAP1])
def test_scale_by_device_scalar_sizes(hip, n):
    x = _data("scale_x", n)
    sc = torch.tensor([0.3721], dtype=torch.float32)
    gx, gs = Guarded(x), Guarded(sc)
    hip.check(hip.lib().rho_scale_by_device_scalar(gx.ptr, gs.ptr, n, hip.stream()), "rho_scale_by_device_scalar")
    assert gx.intact() and gs.intact() and torch.equal(gs.cpu(), sc)
    assert same_bits(gx.cpu(), x * sc)                                       # one float32 product per element
