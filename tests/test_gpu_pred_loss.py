"""-m gpu: rho_pred_loss_ws, the training loss of an eps- / v- / x0-predicting backbone with optional min-SNR weights, at the sizes,
sample boundaries and alignments where a streaming reduction goes wrong (the manner of test_gpu_spaced_step.py).

Operands sit between 64 sentinel elements and must come back unchanged.  Shapes (B, P): (1, 1), (3, 5), (3, 255), (5, 257), (2, 1028)
and (3, 700 003): P % 4 != 0 makes 16-byte pieces straddle sample boundaries, P < 4 takes the scalar form, and the last is past
twice 1024 blocks x 256 threads x 4 elements (the Python binding passes n_partials = 1024): every thread takes a second trip, the
first blocks a third.
alpha_bar: LinearSchedule(1000) as float32; w: min_snr_weights(alpha_bar, type, 5) or NULL; t spreads over the table, both ends included.

Reference: float64 on the float32 inputs and tables.  U = 2^-24.  The kernel's written-out contraction, per sample b and element i:
    ab = alpha_bar[t_b]     o = 1 - ab  (1)     sa = sqrtf(ab)  (2)     sb = sqrtf(o)  (3)                      v only
    m  = sb * x0  (4)       g = fma(sa, eps, -m)  (5)                    epsilon: g = eps, sample: g = x0, exact
    d  = pred - g  (6)
    inv = 1.0f / (float)n  (7, 8: the conversion rounds from n = 2^24 on)       k2 = 2 * inv, exact      kw = w_b * k2  (9)
    grad = kw * d  (10)         wd = w_b * d  (11)         sum = fma(wd, d, sum)  (12)
sqrtf is granted one ulp, 2 U, so sa carries 2 U and sb 2.5 U (half of (1), then its own).  First order, one term per rounding:
    Eg   = 2 |sa eps| + 3.5 |m| + |g|   (v; 0 otherwise)       the error of g in units of U      [(2) |sa eps|, (3)+(4) |m|, (5) |g|]
    Ed   = Eg + |d|                                            the error of d
    grad:  |grad - ref| <= U [ (2 w_b / n) Ed + 4 |ref| ]                         [(7), (8), (9), (10) are relative to the result]
    term w_b d^2 of the loss:  <= U [ 2 w_b |d| Ed + w_b d^2 ]                    [d enters twice; (11)]
The reduction tree (that of rho_mse_ws; every term is >= 0, so every intermediate sum is at most the total S):
    thread: a sequential fma sum of its m_t elements, m_t <= 4 ceil(ceil(n / 4) / (256 G)) + 1 with G = min(1024, ceil(n / 2048))
            blocks - at most m_t U S summed over the threads
    wave_sum: 6 levels, 6 U S;   the block's four waves (r0 + r1) + (r2 + r3): 2 U S;   times inv: 3 U S  [(7), (8) and its own]
    k_mse_final: each of 64 lanes adds ceil(G / 64) partials in index order, ceil(G / 64) U S;  wave_sum: 6 U S
    |loss - ref| <= U [ sum of the term bounds / n + (m_t + ceil(G / 64) + 17) ref ]
Both bounds carry the factor 1.001 for the second-order terms.  grad must have the same bits in every form (16-byte body, tail,
scalar); the loss of a misaligned run only stays within its bound, since other threads add other elements.  With w == 1 and type
epsilon, grad = k2 * (pred - eps) is what rho_mse_ws writes for (pred, eps): bit-equal."""
import functools
import math

import pytest
import torch

from helpers import det_normal
from gpu_util import DEV, Guarded, check_bound, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
T = 1000
EPSILON, V, SAMPLE = 0, 1, 2
KINDS = {EPSILON: "epsilon", V: "v", SAMPLE: "sample"}
SHAPES = [(1, 1), (3, 5), (3, 255), (5, 257), (2, 1028)]
BIG = (3, 700_003)                 # n = 2 100 009 > 1024 * 256 * 4 * 2: a second trip, a third for some; P % 4 == 3: pieces straddle both boundaries
POOL = BIG[0] * BIG[1]
NPART = 1024


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=None)
def _pool(salt: str) -> torch.Tensor:
    return det_normal((POOL,), "predloss_" + salt)


@functools.lru_cache(maxsize=None)
def _alpha_bar() -> torch.Tensor:
    from rho_diffusion_amd.diffusion import LinearSchedule
    return LinearSchedule(T, 1e-3, 0.02)["alpha_bar_t"].float().contiguous()


@functools.lru_cache(maxsize=None)
def _weights(kind: int) -> torch.Tensor:
    from rho_diffusion_amd.diffusion.prediction import min_snr_weights
    return min_snr_weights(_alpha_bar(), KINDS[kind], 5.0).contiguous()


def _timesteps(B: int) -> torch.Tensor:
    return torch.tensor([(0, T - 1, 500, 7, 333)[b % 5] for b in range(B)], dtype=torch.int64)


def _inputs(B, P, kind):
    """(pred, x0, eps) float32 [B * P]: x0 = 0.7 N, eps = N, pred = half the true target of the middle timestep plus 0.5 N."""
    n = B * P
    x0, eps = (0.7 * _pool("x0")[:n].double()).float(), _pool("eps")[:n]
    true = {EPSILON: eps.double(), SAMPLE: x0.double(), V: 0.7 * eps.double() - 0.7 * x0.double()}[kind]
    pred = (0.5 * true + 0.5 * _pool("pred")[:n].double()).float()
    return pred, x0, eps


def _run(hip, B, P, kind, pred, x0, eps, t, w, want_grad, shifts=frozenset(), flag=True, expect=0):
    """Launch on guarded copies; returns (loss float32 [1] on the CPU, grad float32 [n] on the CPU or None, the flag's value)."""
    n = B * P
    gp, gx, ge = Guarded(pred, int("pred" in shifts)), Guarded(x0, int("x0" in shifts)), Guarded(eps, int("eps" in shifts))
    gg = Guarded(torch.full((n,), 123.0), int("grad" in shifts)) if want_grad else None
    out = Guarded(torch.full((1 + NPART,), 321.0))                 # loss, then the block partials
    ab_d, t_d = _alpha_bar().to(DEV), t.to(DEV)
    w_d = w.to(DEV) if w is not None else None
    flag_d = torch.zeros(1, dtype=torch.int32, device=DEV) if flag else None
    rc = hip.lib().rho_pred_loss_ws(gp.ptr, gx.ptr, ge.ptr, ab_d.data_ptr(), w_d.data_ptr() if w is not None else None, t_d.data_ptr(),
                                    B, P, T, kind, out.ptr, gg.ptr if gg else None, out.ptr + 4, NPART,
                                    flag_d.data_ptr() if flag else None, hip.stream())
    assert rc == expect, (rc, expect)
    what = (B, P, KINDS.get(kind), w is not None, want_grad, sorted(shifts))
    assert gp.intact() and gx.intact() and ge.intact() and out.intact() and (gg is None or gg.intact()), what
    assert same_bits(gp.cpu(), pred) and same_bits(gx.cpu(), x0) and same_bits(ge.cpu(), eps), what
    assert torch.equal(ab_d.cpu(), _alpha_bar()) and torch.equal(t_d.cpu(), t) and (w is None or torch.equal(w_d.cpu(), w)), what
    return out.cpu()[:1].clone(), (gg.cpu() if gg else None), (int(flag_d.item()) if flag else None)


def _ref(B, P, kind, pred, x0, eps, t, w):
    """float64 (loss, its bound, grad [n], its bound [n]) - module docstring.  ``t`` already clamped to the table."""
    n = B * P
    ab = _alpha_bar().double()[t]
    wb = (w.double()[t] if w is not None else torch.ones(B, dtype=torch.float64)).view(B, 1)
    p, x, e = (v.double().view(B, P) for v in (pred, x0, eps))
    if kind == V:
        sa, sb = ab.sqrt().view(B, 1), (1.0 - ab).sqrt().view(B, 1)
        m = sb * x
        g = sa * e - m
        Eg = 2.0 * (sa * e).abs() + 3.5 * m.abs() + g.abs()
    else:
        g = e if kind == EPSILON else x
        Eg = torch.zeros_like(p)
    d = p - g
    Ed = Eg + d.abs()
    grad = 2.0 * wb * d / n
    grad_bound = 1.001 * U * ((2.0 * wb / n) * Ed + 4.0 * grad.abs())
    loss = float((wb * d * d).sum() / n)
    term_bound = float((2.0 * wb * d.abs() * Ed + wb * d * d).sum() / n)
    G = min(NPART, max(1, -(-n // 2048)))
    m_t = 4 * -(-(-(-n // 4)) // (256 * G)) + 1
    loss_bound = 1.001 * U * (term_bound + (m_t + -(-G // 64) + 17) * loss)
    return loss, loss_bound, grad.flatten(), grad_bound.flatten()


@functools.lru_cache(maxsize=None)
def _case(B, P, kind, weighted):
    """Inputs and reference of one case, computed once and shared (never written to)."""
    pred, x0, eps = _inputs(B, P, kind)
    t = _timesteps(B)
    w = _weights(kind) if weighted else None
    return pred, x0, eps, t, w, _ref(B, P, kind, pred, x0, eps, t, w)


def _check_loss(got, ref, bound, what):
    got = float(got.double())
    print(what, "loss", got, "ref", ref, "err", abs(got - ref), "bound", bound)
    assert math.isfinite(got) and abs(got - ref) <= bound, (what, got, ref, abs(got - ref), bound)


def _one(hip, B, P, kind, weighted, want_grad, shifts=frozenset()):
    pred, x0, eps, t, w, (loss_ref, loss_bound, grad_ref, grad_bound) = _case(B, P, kind, weighted)
    loss, grad, flag = _run(hip, B, P, kind, pred, x0, eps, t, w, want_grad, shifts)
    what = ("pred_loss", B, P, KINDS[kind], weighted, want_grad, sorted(shifts))
    assert flag == 0, what
    _check_loss(loss, loss_ref, loss_bound, what)
    if want_grad:
        check_bound(grad, grad_ref, grad_bound, what)
    return loss, grad


@pytest.mark.parametrize("kind", [EPSILON, V, SAMPLE], ids=["epsilon", "v", "sample"])
@pytest.mark.parametrize("B,P", SHAPES + [BIG])
def test_loss_and_grad(hip, B, P, kind):
    for weighted in (False, True):
        with_grad = _one(hip, B, P, kind, weighted, True)
        without = _one(hip, B, P, kind, weighted, False)
        assert same_bits(with_grad[0], without[0]), (B, P, kind, weighted)       # grad == NULL changes nothing about the sum
        again = _one(hip, B, P, kind, weighted, True)
        assert same_bits(again[0], with_grad[0]) and same_bits(again[1], with_grad[1]), (B, P, kind, weighted)   # run to run


def test_weights_matter(hip):
    """The weighted and the unweighted loss differ (the table is read), and a table of ones gives the bits of w == NULL."""
    B, P = 5, 257
    for kind in (EPSILON, V, SAMPLE):
        pred, x0, eps, t, w, _ = _case(B, P, kind, True)
        lw, gw, _ = _run(hip, B, P, kind, pred, x0, eps, t, w, True)
        l1, g1, _ = _run(hip, B, P, kind, pred, x0, eps, t, None, True)
        lo, go, _ = _run(hip, B, P, kind, pred, x0, eps, t, torch.ones(T), True)
        assert not same_bits(lw, l1) and not same_bits(gw, g1), kind
        assert same_bits(lo, l1) and same_bits(go, g1), kind


@pytest.mark.parametrize("B,P", SHAPES + [BIG])
def test_epsilon_with_unit_weight_has_the_gradient_of_rho_mse_ws(hip, B, P):
    pred, x0, eps, t, _, _ = _case(B, P, EPSILON, False)
    n = B * P
    a, b = Guarded(pred), Guarded(eps)
    g = Guarded(torch.zeros(n))
    out = torch.zeros(1 + NPART, dtype=torch.float32, device=DEV)
    hip.check(hip.lib().rho_mse_ws(a.ptr, b.ptr, out.data_ptr(), g.ptr, n, out.data_ptr() + 4, NPART, hip.stream()), "rho_mse_ws")
    for w in (None, torch.ones(T)):
        loss, grad, _ = _run(hip, B, P, EPSILON, pred, x0, eps, t, w, True)
        assert same_bits(grad, g.cpu()), (B, P, w is not None)
        # the two losses are sums of the same terms in the same tree; rho_mse_ws leaves the contraction of d * d + sum to the
        # compiler, so only the bound is claimed
        _, (loss_ref, loss_bound, _, _) = _case(B, P, EPSILON, False)[4:]
        assert abs(float(out[0].double()) - loss_ref) <= loss_bound and abs(float(loss.double()) - loss_ref) <= loss_bound


@pytest.mark.parametrize("kind", [EPSILON, V, SAMPLE], ids=["epsilon", "v", "sample"])
@pytest.mark.parametrize("B,P", [(3, 255), (2, 1028), (5, 257)])
def test_alignment(hip, B, P, kind):
    """Each operand offset by 4 bytes, singly and together, takes the scalar form: grad has the bits of the aligned run, the loss
    stays within its bound."""
    base = _one(hip, B, P, kind, True, True)
    for shifts in [frozenset([s]) for s in ("pred", "x0", "eps", "grad")] + [frozenset(("pred", "x0", "eps", "grad"))]:
        loss, grad = _one(hip, B, P, kind, True, True, shifts)
        assert same_bits(grad, base[1]), (B, P, kind, sorted(shifts))


def test_alignment_at_the_large_size(hip):
    B, P = BIG
    base = _one(hip, B, P, V, True, True)
    loss, grad = _one(hip, B, P, V, True, True, frozenset(["x0"]))
    assert same_bits(grad, base[1])


@pytest.mark.parametrize("B,P", [(3, 5), (5, 257)])
def test_timestep_outside_the_table_sets_bit_2_and_reads_the_clamped_row(hip, B, P):
    for kind in (EPSILON, V, SAMPLE):
        pred, x0, eps, t, w, _ = _case(B, P, kind, True)
        bad = t.clone()
        bad[0], bad[-1] = -3, T + 5
        clamped = t.clone()
        clamped[0], clamped[-1] = 0, T - 1
        loss, grad, flag = _run(hip, B, P, kind, pred, x0, eps, bad, w, True)
        assert flag == 4, (kind, flag)
        want_loss, want_grad, flag = _run(hip, B, P, kind, pred, x0, eps, clamped, w, True)
        assert flag == 0 and same_bits(loss, want_loss) and same_bits(grad, want_grad), kind
        loss_ref, loss_bound, grad_ref, grad_bound = _ref(B, P, kind, pred, x0, eps, clamped, w)
        check_bound(grad, grad_ref, grad_bound, ("clamped", B, P, kind))
        _check_loss(loss, loss_ref, loss_bound, ("clamped", B, P, kind))
        loss2, grad2, none = _run(hip, B, P, kind, pred, x0, eps, bad, w, True, flag=False)      # the flag is optional
        assert none is None and same_bits(loss2, loss) and same_bits(grad2, grad)


def test_bad_arguments_are_refused(hip):
    B, P = 3, 5
    pred, x0, eps, t, w, _ = _case(B, P, V, True)
    for kind in (-1, 3):
        _run(hip, B, P, kind, pred, x0, eps, t, w, True, expect=-1)
    lib = hip.lib()
    g = Guarded(pred)
    out = torch.zeros(1 + NPART, dtype=torch.float32, device=DEV)
    ab, td = _alpha_bar().to(DEV), t.to(DEV)
    ok = [g.ptr, g.ptr, g.ptr, ab.data_ptr(), None, td.data_ptr(), B, P, T, V, out.data_ptr(), None, out.data_ptr() + 4, NPART, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (5, None), (6, 0), (7, 0), (8, 0), (10, None), (12, None), (13, 0)):
        args = list(ok)
        args[i] = v
        assert lib.rho_pred_loss_ws(*args, hip.stream()) == -1, i
    assert float(out.abs().max()) == 0.0 and same_bits(g.cpu(), pred)


def test_wrapper_and_autograd(hip):
    from rho_diffusion_amd.autograd import pred_loss
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    B, P = 2, 1028
    pred, x0, eps, t, w, (loss_ref, loss_bound, grad_ref, grad_bound) = _case(B, P, V, True)
    shape = (B, 1, 4, 257)
    pd, xd, ed, td = pred.view(shape).to(DEV), x0.view(shape).to(DEV), eps.view(shape).to(DEV), t.to(DEV)
    ab, wd = _alpha_bar().to(DEV), w.to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, grad = ops.pred_loss(pd, xd, ed, td, ab, wd, V, want_grad=True, err_flag=flag)
    raw_loss, raw_grad, _ = _run(hip, B, P, V, pred, x0, eps, t, w, True)
    assert loss.shape == (1,) and grad.shape == shape and same_bits(loss, raw_loss) and same_bits(grad.flatten(), raw_grad)
    assert ops.pred_loss(pd, xd, ed, td, ab, None, V)[1] is None and int(flag.item()) == 0
    leaf = pd.clone().requires_grad_(True)
    out = pred_loss(leaf, xd, ed, td, ab, wd, V, flag)
    assert out.shape == () and same_bits(out.detach().reshape(1), raw_loss)
    (3.0 * out).backward()                                       # the upstream gradient is applied on the device
    check_bound(leaf.grad.cpu() / 3.0, grad_ref, grad_bound + 2.0 * U * grad_ref.abs(), "autograd")
    for bad in (lambda: ops.pred_loss(pd.double(), xd, ed, td, ab, wd, V),
                lambda: ops.pred_loss(pd, xd[:1].contiguous(), ed, td, ab, wd, V),
                lambda: ops.pred_loss(pd, xd, ed, td.int(), ab, wd, V),
                lambda: ops.pred_loss(pd, xd, ed, td.cpu(), ab, wd, V),
                lambda: ops.pred_loss(pd, xd, ed, td[:1], ab, wd, V),
                lambda: ops.pred_loss(pd, xd, ed, td, ab, wd[:5].contiguous(), V),
                lambda: ops.pred_loss(pd, xd, ed, td, ab, wd, 3),
                lambda: ops.pred_loss(pd, xd, ed, td, ab, wd, V, err_flag=flag.long())):
        with pytest.raises(RhoHipError):
            bad()
