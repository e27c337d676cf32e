"""-m gpu: the element-wise VisionTransformer kernels of csrc/vit.hip (``rho_bias_act``, ``rho_bias_act_bwd``, ``rho_pos_add``,
``rho_pos_add_bwd``) per element, at the edges of the activation expressions of csrc/common.h (``silu_f`` / ``dsilu_f`` with the
hardware exp2 and reciprocal, ``act_other_f`` / ``dact_other_f``: 1 + erff cancelling for u << 0, u phi(u) underflowing, saturated
tanh / sigmoid / expm1).

``rho_bias_act`` / ``rho_bias_act_bwd``: all six activations, with and without a bias that differs in every column, float32 and bf16.
* index checks at (rows, cols) = (1, 8), (5, 24), (37, 96), (3, 1024) with u = x + bias uniform in [-5, 5];
* range buckets [-100, -20], [-20, -5], [-5, 5], [5, 20], [20, 100]: 64 x 64 uniform draws of u each;
* one hand-written row: +-0, +-2^-140, +-1e-30, +-0.75, +-1.2785, +-87, +-89, +-104.
Reference: float64 torch on the same inputs (for bf16 the bf16-rounded ones), f' and f'' by autograd.  Error scale per element, the
mixed forward-backward criterion (an evaluation that is exact at an input a few ulps away is no error):
    forward  s = |f(u)| + |u f'(u)|            backward  s = |dy| (|f'(u)| + |u f''(u)|)
and the bound  (K rho + 16 * 2^-24) s + 2^-126 max(1, |u|)  with K = 4, where rho = max over the tensor of |o - f64| / s and o is
torch's float32 CPU evaluation of the same function on the same inputs (it only sizes the bound); the last term admits one flushed
denormal (dy is drawn from [-1, 1] so that this absolute term means the same in the backward: |dy| sigma(u) |1 + u| stays below
2^-126 |u| wherever sigma(u) is a denormal).  bf16 adds 2^-8 |f64| for the one output rounding.  ReLU forward and backward are
bit-exact.  This covers the kernels' own mechanisms, which are no defects: the rounding of the argument in exp2(-1.4427 u) (a
relative error of 2^-24 |u| in sigmoid(u), inside |u f'(u)|), and 1 + erff(u / sqrt 2) losing everything below 2^-24 (torch's float32
GELU does the same, so rho carries it).

``rho_pos_add`` at (B, N, E) = (1, 1, 8), (3, 7, 32), (2, 133, 96): float32 bit-equal to x + pos, bf16 to (x.float() + pos).bfloat16();
``rho_pos_add_bwd`` bit-equal to a float32 loop over the batch in ascending order, both dtypes.

NOT ASKED FOR HERE: the second trip of the grid-stride loops.  The grid is capped at 262144 workgroups of 256 threads, so a thread
takes a second 16-byte vector only beyond 262144 * 256 vectors - more than 1 GiB per operand.

MEASURED on an MI355X: worst err / bound as "forward / backward", over with and without bias; columns: the four index shapes,
the five buckets from [-100, -20] to [20, 100], the hand-written row.  Nothing needed a fix in common.h or a bound of its own.
    float32   shapes      [-100,-20]  [-20,-5]    [-5,5]      [5,20]      [20,100]    hand
    SiLU      0.12/0.18   0.97/0.80   0.09/0.09   0.12/0.17   0.07/0.20   0.03/0.04   0.19/0.06
    GELU      0.17/0.18   0.00/0.00   0.25/0.01   0.08/0.14   0.05/0.08   0.03/0.00   0.13/0.05
    Tanh      0.06/0.25   0.00/0.00   0.03/0.25   0.07/0.25   0.03/0.25   0.00/0.00   0.03/0.06
    Sigmoid   0.08/0.22   0.05/0.05   0.05/0.05   0.07/0.22   0.07/0.25   0.00/0.25   0.03/0.05
    ELU       0.04/0.06   0.00/0.05   0.04/0.05   0.04/0.05   0.03/0.00   0.03/0.00   0.02/0.05
    bf16
    SiLU      0.99/0.99   0.99/0.97   0.99/0.97   0.98/0.99   0.98/0.94   0.96/0.00   0.79/0.70
    GELU      0.84/0.91   0.00/0.00   0.25/0.01   0.09/0.84   0.97/0.00   0.96/0.00   0.84/0.39
    Tanh      0.99/0.95   0.00/0.00   0.02/0.25   0.95/0.95   0.02/0.25   0.00/0.00   0.76/0.91
    Sigmoid   0.98/0.98   0.98/0.96   0.98/0.99   0.98/0.97   0.50/0.25   0.00/0.25   0.77/0.71
    ELU       0.98/0.98   0.00/0.96   0.50/0.98   0.99/0.98   0.97/0.00   0.96/0.00   0.71/0.55
The 0.97 of SiLU on [-100, -20] is the flushed denormal: for u below -87.3 sigmoid(u) < 2^-126, the hardware reciprocal returns 0
and the kernel's u * 0 stands against |u| sigmoid(u) just under 2^-126 |u|, the bound's last term.  A 0.25 is err = rho s against K rho s: at the
worst element the kernel errs exactly as torch's float32 evaluation does (tanh / sigmoid saturated, 1 - t^2 and s (1 - s)
cancelling in both, where rho is up to 6e-2).  bf16 sits at 0.95 - 0.99 wherever the output is no constant: the bound there IS
the one bf16 rounding, 2^-8 |f| at the bottom of a binade, and 4096 draws come close to it.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from detdata import det_uniform
from gpu_util import DEV

pytestmark = pytest.mark.gpu

K = 4.0
U = 2.0 ** -24
TINY = 2.0 ** -126
ACTS = {"SiLU": F.silu, "ReLU": F.relu, "GELU": F.gelu, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "ELU": F.elu}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [(1, 8), (5, 24), (37, 96), (3, 1024)]
BUCKETS = [(-100.0, -20.0), (-20.0, -5.0), (-5.0, 5.0), (5.0, 20.0), (20.0, 100.0)]
HAND = [0.0, 2.0 ** -140, 1e-30, 0.75, 1.2785, 87.0, 89.0, 104.0]


@functools.lru_cache(maxsize=None)
def _inputs(name: str, dtype_name: str, with_bias: bool):
    """(x in the kernel's dtype, bias float32 or None, dy in the kernel's dtype), on the CPU: u = x + bias lies in the set's range."""
    dtype = DTYPES[dtype_name]
    if name == "hand":
        u = torch.tensor([[s * v for v in HAND for s in (1.0, -1.0)]], dtype=torch.float32)
    elif name.startswith("shape"):
        u = det_uniform(SHAPES[int(name[5:])], f"ew_{name}", -5.0, 5.0)
    else:
        lo, hi = BUCKETS[int(name[6:])]
        u = det_uniform((64, 64), f"ew_{name}", lo, hi)
    cols = u.shape[1]
    bias = 0.75 * det_uniform((cols,), f"ew_bias{cols}") if with_bias else None        # distinct per column
    x = (u - bias if with_bias else u).to(dtype)
    dy = det_uniform(tuple(u.shape), f"ew_dy_{name}").to(dtype)
    return x, bias, dy


def _references(fn, x, bias, dy):
    """float64 f, f', f'' at u = x + bias and torch's float32 evaluations of f(u) and dy f'(u)."""
    u64 = x.double() + bias.double() if bias is not None else x.double().clone()
    u64.requires_grad_(True)
    f = fn(u64)
    (f1,) = torch.autograd.grad(f.sum(), u64, create_graph=True)
    f2 = torch.autograd.grad(f1.sum(), u64, allow_unused=True)[0] if f1.requires_grad else None
    f2 = torch.zeros_like(u64) if f2 is None else f2
    u32 = (x.float() + bias if bias is not None else x.float().clone()).requires_grad_(True)
    o = fn(u32)
    (od,) = torch.autograd.grad(o, u32, dy.float())
    return u64.detach(), f.detach(), f1.detach(), f2.detach(), o.detach().double(), od.detach().double()


def _worst(got, want, o, s, u, bf16: bool):
    """max over elements of err / bound, and rho."""
    live = s > 2.0 ** -100
    rho = float(((o - want).abs()[live] / s[live]).max()) if bool(live.any()) else 0.0
    bound = (K * rho + 16 * U) * s + TINY * u.abs().clamp(min=1.0)
    if bf16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got.double().cpu() - want).abs()
    r = err / bound
    i = int(r.argmax())
    return float(r.max()), rho, (float(u.flatten()[i]), float(got.flatten()[i]), float(want.flatten()[i]))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("act", list(ACTS))
def test_bias_act_forward_and_backward_per_element(act, dtype_name):
    from rho_diffusion_amd.engine import ops
    fn, dtype, code = ACTS[act], DTYPES[dtype_name], ops.ACT_CODES[act]
    sets = [f"shape{i}" for i in range(len(SHAPES))] + [f"bucket{i}" for i in range(len(BUCKETS))] + ["hand"]
    bad = []
    for name in sets:
        for with_bias in (False, True):
            x, bias, dy = _inputs(name, dtype_name, with_bias)
            bd = bias.to(DEV) if with_bias else None
            y = ops.bias_act(x.to(DEV), code, bias=bd)
            dx = ops.bias_act_bwd(x.to(DEV), dy.to(DEV), code, bias=bd)
            assert y.dtype == dtype and dx.dtype == dtype and y.shape == x.shape and dx.shape == x.shape
            assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
            if act == "ReLU":
                u32 = x.float() + bias if with_bias else x.float()
                assert torch.equal(y.cpu(), F.relu(u32).to(dtype)), (name, with_bias)
                assert torch.equal(dx.cpu(), (dy.float() * (u32 > 0).float()).to(dtype)), (name, with_bias)
                continue
            u, f, f1, f2, o, od = _references(fn, x, bias, dy)
            d64 = dy.double()
            rf, rho_f, at_f = _worst(y, f, o, f.abs() + (u * f1).abs(), u, dtype == torch.bfloat16)
            rb, rho_b, at_b = _worst(dx, d64 * f1, od, d64.abs() * (f1.abs() + (u * f2).abs()), u, dtype == torch.bfloat16)
            print(f"bias_act {act} {dtype_name} {name} bias={int(with_bias)}: fwd err/bound {rf:.3f} (rho {rho_f:.2e}), "
                  f"bwd err/bound {rb:.3f} (rho {rho_b:.2e})")
            if rf > 1.0:
                bad.append((name, with_bias, "fwd", rf, at_f))
            if rb > 1.0:
                bad.append((name, with_bias, "bwd", rb, at_b))
    assert not bad, bad[:8]


POS_SHAPES = [(1, 1, 8), (3, 7, 32), (2, 133, 96)]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_pos_add_and_its_backward_bit_exact(dtype_name):
    from rho_diffusion_amd.engine import ops
    dtype = DTYPES[dtype_name]
    for shape in POS_SHAPES:
        B, N, E = shape
        x = det_uniform(shape, f"pa_x{shape}", -3.0, 3.0).to(dtype)
        pos = det_uniform((N, E), f"pa_p{shape}", -3.0, 3.0)
        got = ops.pos_add(x.to(DEV).clone(), pos.to(DEV))
        assert got.dtype == dtype and torch.equal(got.cpu(), (x.float() + pos).to(dtype)), shape
        dpos = ops.pos_add_bwd(x.to(DEV))
        acc = torch.zeros(N, E, dtype=torch.float32)
        for b in range(B):
            acc = acc + x[b].float()
        assert dpos.dtype == torch.float32 and tuple(dpos.shape) == (N, E) and torch.equal(dpos.cpu(), acc), shape
