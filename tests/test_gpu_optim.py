"""-m gpu: the fused optimizer kernel (rho_optim_step), the gradient-norm reduction (rho_sumsq_partial / rho_clip_coef) and the
optimizer classes of rho_diffusion_amd/optim.py built on them.

Reference: ``torch.optim.X(foreach=False)`` on float64 CPU copies, fed the same float32 gradients, with the hyperparameters rounded to
float32 first (the ABI receives float32).  Two bars, as in test_gpu_streaming_edges.py: rel-L2 < 1e-6 on the parameters and on every
state after every step, and a per-element bound  |got - ref| <= 2^-24 * sum over the kernel's operations of |that operation's result|,
propagated through the expression.

How the per-element bound is counted.  The kernel's update (csrc/optim.hip: opt_update, contraction off, so every product, sum,
quotient and square root rounds once; hipcc's default is correctly rounded division and sqrtf) is written out once more in ``_shadow``
over pairs (value, error bound) in float64 - a running error analysis: each operation adds U = 2^-24 times the magnitude of its result
(one rounding: k grows by one on that term) to the first-order propagation of its operands' bounds
    a + b: ea + eb      a * b: |a| eb + |b| ea + ea eb      a / b: (ea + |a / b| eb) / (|b| - eb)
    sqrt(a): sqrt(a) - sqrt(max(a - ea, 0))   (the larger of the two one-sided deviations; this is what carries the cancellation of
             centred RMSprop's square_avg - grad_avg^2 into the bound)         max, |.|, negation: exact.
A scalar the launcher computes in double and casts to float32 (1 - beta1, lr / bc1, 1 / sqrt(bc2), clr, NAdam's two factors, RAdam's
rectified factor, 1 - lr * weight_decay) carries one rounding; a hyperparameter passed through unchanged carries none.  States carry
their bound from step to step.  For SGD with momentum, say, this gives per step  buf: 3 roundings (two products, one sum) on top of
momentum times the carried bound;  p: lr * buf (1) and the difference (1) - the same count test_adamw_sizes writes out by hand.
The shadow's VALUE is the kernel's expression in exact-ish arithmetic; it must agree with torch's float64 result to 1e-12 (it is the
same mathematics in a different association), and that difference is added to the bound.  No constant here comes from the observed
error of the kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, det_normal, det_state_dict, det_uniform, golden_template, load_golden, rel_l2
from gpu_util import DEV, Guarded, check_bound, same_bits
from running_error import B, _r, add, div, maxf, mul, neg, sqrt, sub          # noqa: F401  (the analysis of the docstring below)
from test_gpu_streaming_edges import SMALL, U, WRAP4, _data, _shift_sets

pytestmark = pytest.mark.gpu

KINDS = {"Adam": 0, "AdamW": 1, "SGD": 2, "RMSprop": 3, "Adagrad": 4, "Adamax": 5, "NAdam": 6, "RAdam": 7, "Adadelta": 8}
MAXIMIZE, AMSGRAD, DECOUPLED, NESTEROV, CENTERED = 1, 2, 4, 8, 16


def r32(x):
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, tuple):
        return tuple(r32(v) for v in x)
    return float(np.float32(x))


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


# every kind x option set of the issue's table (each with maximize / weight_decay somewhere); "*" marks the one per kind that also runs
# at the wrap-around size and in the alignment test: the option set with the most state arenas and branches
CASES = {
    "adam": ("Adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)),
    "adam_wd_max": ("Adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, maximize=True)),
    "adam_amsgrad*": ("Adam", dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, amsgrad=True)),
    "adam_decoupled": ("Adam", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True)),
    "adamw": ("AdamW", dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)),
    "adamw_amsgrad_max*": ("AdamW", dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, amsgrad=True, maximize=True)),
    "sgd": ("SGD", dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0)),
    "sgd_wd_max": ("SGD", dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=1e-2, maximize=True)),
    "sgd_momentum": ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=0.0)),
    "sgd_dampening*": ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.25, weight_decay=1e-2)),
    "sgd_nesterov": ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.0, weight_decay=1e-2, nesterov=True)),
    "rmsprop": ("RMSprop", dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0)),
    "rmsprop_momentum_max": ("RMSprop", dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=1e-2, momentum=0.9, maximize=True)),
    "rmsprop_centered": ("RMSprop", dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=True)),
    "rmsprop_centered_momentum*": ("RMSprop", dict(lr=1e-2, alpha=0.9, eps=1e-8, weight_decay=1e-2, momentum=0.9, centered=True)),
    "adagrad": ("Adagrad", dict(lr=1e-2, lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10)),
    "adagrad_decay_init_max*": ("Adagrad", dict(lr=1e-2, lr_decay=0.1, weight_decay=1e-2, initial_accumulator_value=0.5, eps=1e-10,
                                                maximize=True)),
    "adamax": ("Adamax", dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)),
    "adamax_wd_max*": ("Adamax", dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, maximize=True)),
    "nadam": ("NAdam", dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3)),
    "nadam_wd_max": ("NAdam", dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, momentum_decay=4e-3, maximize=True)),
    "nadam_decoupled*": ("NAdam", dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, momentum_decay=1e-2,
                                       decoupled_weight_decay=True)),
    "radam": ("RAdam", dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8, weight_decay=0.0)),
    "radam_wd_max": ("RAdam", dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8, weight_decay=1e-2, maximize=True)),
    "radam_decoupled*": ("RAdam", dict(lr=1e-3, betas=(0.9, 0.9), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True)),
    "adadelta": ("Adadelta", dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0)),
    "adadelta_wd_max*": ("Adadelta", dict(lr=0.5, rho=0.95, eps=1e-6, weight_decay=1e-2, maximize=True)),
}
CASES = {k: (kind, {key: r32(v) for key, v in o.items()}) for k, (kind, o) in CASES.items()}
STARRED = [k for k in CASES if k.endswith("*")]
assert sorted(CASES[k][0] for k in STARRED) == sorted(KINDS)


def radam_rho_t(beta2, step):
    """radam.py: the length of the approximated SMA; > 5 takes the rectified branch."""
    return (2 / (1 - beta2) - 1) - 2 * step * beta2 ** step / (1 - beta2 ** step)


def n_steps(kind):
    # SGD: step 1 seeds the buffer, steps 2 and 3 run the recurrence.  RAdam with beta2 = 0.9: rho_t = 1.0, 1.9, 2.9, 3.7, 4.6, 5.4, 6.1 -
    # the unrectified branch for steps 1 .. 5, the rectified one from step 6 (test_radam_takes_both_branches pins this on the CPU)
    return 7 if kind == "RAdam" else 3


def test_radam_takes_both_branches():
    b2 = r32(0.9)
    taken = [radam_rho_t(b2, s) > 5.0 for s in range(1, n_steps("RAdam") + 1)]
    assert taken == [False] * 5 + [True] * 2


# ----------------------------------------------------------------------------- the ABI as the test drives it
def abi_of(kind, o, step, mu_product):
    """(flags, hp[3:], torch names of the state slots) - written from include/rho_hip.h, not taken from optim.py."""
    flags = MAXIMIZE if o.get("maximize") else 0
    if kind in ("Adam", "AdamW"):
        flags |= (AMSGRAD if o.get("amsgrad") else 0) | (DECOUPLED if kind == "Adam" and o.get("decoupled_weight_decay") else 0)
        return flags, o["betas"], ["exp_avg", "exp_avg_sq", "max_exp_avg_sq" if o.get("amsgrad") else None]
    if kind == "SGD":
        return flags | (NESTEROV if o.get("nesterov") else 0), (o["momentum"], o["dampening"]), \
            ["momentum_buffer" if o["momentum"] != 0 else None, None, None]
    if kind == "RMSprop":
        return flags | (CENTERED if o.get("centered") else 0), (o["alpha"], o["momentum"]), \
            ["square_avg", "grad_avg" if o.get("centered") else None, "momentum_buffer" if o["momentum"] > 0 else None]
    if kind == "Adagrad":
        return flags, (o["lr_decay"],), ["sum", None, None]
    if kind == "Adamax":
        return flags, o["betas"], ["exp_avg", "exp_inf", None]
    if kind == "NAdam":
        return flags | (DECOUPLED if o.get("decoupled_weight_decay") else 0), (*o["betas"], o["momentum_decay"], mu_product), \
            ["exp_avg", "exp_avg_sq", None]
    if kind == "RAdam":
        return flags | (DECOUPLED if o.get("decoupled_weight_decay") else 0), o["betas"], ["exp_avg", "exp_avg_sq", None]
    return flags, (o["rho"],), ["square_avg", "acc_delta", None]


def nadam_mu(o, step):
    return o["betas"][0] * (1.0 - 0.5 * (0.96 ** (step * o["momentum_decay"])))


class KernelRun:
    """The arenas of one rho_optim_step sequence, each between sentinels, each optionally one element off 16-byte alignment."""

    def __init__(self, hip, kind, o, p0, shifts=frozenset()):
        self.hip, self.kind, self.o, self.shifts, self.n = hip, kind, o, shifts, p0.numel()
        self.p = Guarded(p0, int("p" in shifts))
        _, _, names = abi_of(kind, o, 1, 1.0)
        init = o.get("initial_accumulator_value", 0.0)
        self.names = names
        self.s = {nm: Guarded(torch.full((self.n,), init if nm == "sum" else 0.0), int(nm in shifts)) for nm in names if nm}
        self.mu_product = torch.ones((), dtype=torch.float32)          # torch keeps it as a float32 scalar (nadam.py)

    def step(self, step, g32, gscale=None):
        if self.kind == "NAdam":
            self.mu_product *= nadam_mu(self.o, step)
        flags, extra, names = abi_of(self.kind, self.o, step, float(self.mu_product))
        hp = [self.o["lr"], self.o.get("weight_decay", 0.0), self.o.get("eps", 0.0), *extra]
        arr = (ctypes.c_float * 8)(*(hp + [0.0] * (8 - len(hp))))
        g = Guarded(g32, int("g" in self.shifts))
        ptrs = [self.s[nm].ptr if nm else None for nm in names]
        rc = self.hip.lib().rho_optim_step(KINDS[self.kind], flags, self.p.ptr, g.ptr, *ptrs, self.n, ctypes.addressof(arr), step,
                                           gscale.data_ptr() if gscale is not None else None, self.hip.stream())
        self.hip.check(rc, "rho_optim_step")
        what = (self.kind, self.n, step, sorted(self.shifts))
        assert self.p.intact() and g.intact() and all(s.intact() for s in self.s.values()), what
        assert torch.equal(g.cpu(), g32), what                                       # the gradient comes back unchanged


# ----------------------------------------------------------------------------- running error analysis (module docstring)
def cast(x, kernel_x=None):
    """A double the launcher casts to float32.  ``kernel_x``: the launcher's double where it is known to differ from the reference's
    ``x`` (NAdam's factors once mu_product has been through a float64 state_dict)."""
    kx = x if kernel_x is None else kernel_x
    return B(torch.tensor(float(x), dtype=torch.float64), torch.tensor(abs(float(kx) - float(x)) + U * abs(float(kx)), dtype=torch.float64))


def lerp(s, g, w):                                   # s + w * (g - s)
    return add(s, mul(w, sub(g, s)))


def ema_sq(s, g, b, w):                              # s * b + (w * g) * g
    return add(mul(s, b), mul(mul(w, g), g))


def _shadow(kind, o, step, p, g, s, mu_product=None, gs=None, mu_product_kernel=None):
    """One step of csrc/optim.hip's opt_update over (value, bound) pairs.  p, g: B; s: {torch state name: B}.  Returns the new p.
    mu_product: the reference's (after this step's factor); mu_product_kernel: the launcher's, where it differs."""
    x = B                                            # a float32 value passed through unchanged
    lr, wd, eps = o["lr"], o.get("weight_decay", 0.0), o.get("eps", 0.0)
    if gs is not None:
        g = mul(g, gs)
    if o.get("maximize"):
        g = neg(g)
    decoupled = kind == "AdamW" or o.get("decoupled_weight_decay", False)
    if wd != 0:
        if decoupled:
            p = mul(p, cast(1.0 - lr * wd))
        else:
            g = add(g, mul(x(wd), p))
    if kind in ("Adam", "AdamW"):
        b1, b2 = o["betas"]
        s["exp_avg"] = lerp(s["exp_avg"], g, cast(1.0 - b1))
        s["exp_avg_sq"] = ema_sq(s["exp_avg_sq"], g, x(b2), cast(1.0 - b2))
        v = s["exp_avg_sq"]
        if o.get("amsgrad"):
            v = s["max_exp_avg_sq"] = maxf(s["max_exp_avg_sq"], v)
        denom = add(mul(sqrt(v), cast(1.0 / math.sqrt(1.0 - b2 ** step))), x(eps))
        return sub(p, mul(cast(lr / (1.0 - b1 ** step)), div(s["exp_avg"], denom)))
    if kind == "SGD":
        mom = o["momentum"]
        if mom != 0:
            s["momentum_buffer"] = g if step == 1 else add(mul(s["momentum_buffer"], x(mom)), mul(cast(1.0 - o["dampening"]), g))
            g = add(g, mul(x(mom), s["momentum_buffer"])) if o.get("nesterov") else s["momentum_buffer"]
        return sub(p, mul(x(lr), g))
    if kind == "RMSprop":
        al = o["alpha"]
        s["square_avg"] = ema_sq(s["square_avg"], g, x(al), cast(1.0 - al))
        if o.get("centered"):
            s["grad_avg"] = lerp(s["grad_avg"], g, cast(1.0 - al))
            avg = sqrt(sub(s["square_avg"], mul(s["grad_avg"], s["grad_avg"])))
        else:
            avg = sqrt(s["square_avg"])
        avg = add(avg, x(eps))
        if o["momentum"] > 0:
            s["momentum_buffer"] = add(mul(s["momentum_buffer"], x(o["momentum"])), div(g, avg))
            return sub(p, mul(x(lr), s["momentum_buffer"]))
        return sub(p, mul(x(lr), div(g, avg)))
    if kind == "Adagrad":
        s["sum"] = add(s["sum"], mul(g, g))
        return sub(p, mul(cast(lr / (1.0 + (step - 1) * o["lr_decay"])), div(g, add(sqrt(s["sum"]), x(eps)))))
    if kind == "Adamax":
        b1, b2 = o["betas"]
        s["exp_avg"] = lerp(s["exp_avg"], g, cast(1.0 - b1))
        s["exp_inf"] = maxf(mul(s["exp_inf"], x(b2)), add(B(g.v.abs(), g.e), x(eps)))
        return sub(p, mul(cast(lr / (1.0 - b1 ** step)), div(s["exp_avg"], s["exp_inf"])))
    if kind == "NAdam":
        b1, b2 = o["betas"]
        mu_next = b1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * o["momentum_decay"])))
        s["exp_avg"] = lerp(s["exp_avg"], g, cast(1.0 - b1))
        s["exp_avg_sq"] = ema_sq(s["exp_avg_sq"], g, x(b2), cast(1.0 - b2))
        denom = add(sqrt(mul(s["exp_avg_sq"], cast(1.0 / (1.0 - b2 ** step)))), x(eps))
        mpk = mu_product if mu_product_kernel is None else mu_product_kernel
        c1 = lambda mp: lr * (1.0 - nadam_mu(o, step)) / (1.0 - mp)                                 # noqa: E731
        c2 = lambda mp: lr * mu_next / (1.0 - mp * mu_next)                                         # noqa: E731
        p = sub(p, mul(cast(c1(mu_product), c1(mpk)), div(g, denom)))
        return sub(p, mul(cast(c2(mu_product), c2(mpk)), div(s["exp_avg"], denom)))
    if kind == "RAdam":
        b1, b2 = o["betas"]
        s["exp_avg"] = lerp(s["exp_avg"], g, cast(1.0 - b1))
        s["exp_avg_sq"] = ema_sq(s["exp_avg_sq"], g, x(b2), cast(1.0 - b2))
        bc1, bc2, rho_inf, rho_t = 1.0 - b1 ** step, 1.0 - b2 ** step, 2 / (1 - b2) - 1, radam_rho_t(b2, step)
        if rho_t > 5.0:
            rect = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t))
            return sub(p, mul(cast(lr * math.sqrt(bc2) * rect / bc1), div(s["exp_avg"], add(sqrt(s["exp_avg_sq"]), x(eps)))))
        return sub(p, mul(cast(lr / bc1), s["exp_avg"]))
    assert kind == "Adadelta"
    rho = o["rho"]
    s["square_avg"] = ema_sq(s["square_avg"], g, x(rho), cast(1.0 - rho))
    delta = mul(div(sqrt(add(s["acc_delta"], x(eps))), sqrt(add(s["square_avg"], x(eps)))), g)
    s["acc_delta"] = ema_sq(s["acc_delta"], delta, x(rho), cast(1.0 - rho))
    return sub(p, mul(x(lr), delta))


def shadow_states(kind, o, n):
    _, _, names = abi_of(kind, o, 1, 1.0)
    init = o.get("initial_accumulator_value", 0.0)
    return {nm: B(torch.full((n,), init if nm == "sum" else 0.0, dtype=torch.float64)) for nm in names if nm}


def torch_reference(kind, o, p0):
    p = nn.Parameter(p0.double().clone())
    return p, getattr(torch.optim, kind)([p], foreach=False, **o)


def check_against(got, ref, sh, what):
    """rel-L2 < 1e-6 and the per-element bound: the shadow's bound plus the shadow's own (tiny, asserted) distance to torch."""
    ref = ref.detach().double().flatten()
    gap = (sh.v - ref).abs()
    assert float(gap.norm()) <= 1e-12 * float(ref.norm()) + 1e-300, (what, "the shadow expression is not torch's", float(gap.max()))
    check_bound(got, ref, sh.e + gap, what, 1e-6 if float(ref.norm()) > 0 else None)


def compare_with_torch(hip, case, n):
    kind, o = CASES[case]
    p0 = _data("opt_p", n)
    run = KernelRun(hip, kind, o, p0)
    pref, opt = torch_reference(kind, o, p0)
    p, s = B(p0.double()), shadow_states(kind, o, n)
    for step in range(1, n_steps(kind) + 1):
        g32 = _data(f"opt_g{step}", n)
        run.step(step, g32)
        pref.grad = g32.double()
        opt.step()
        p = _shadow(kind, o, step, p, B(g32.double()), s, mu_product=float(run.mu_product))
        check_against(run.p.cpu(), pref, p, (case, "p", n, step))
        for nm, guarded in run.s.items():
            ref = opt.state[pref][nm]
            check_against(guarded.cpu(), ref, s[nm], (case, nm, n, step))
        if kind == "NAdam":
            assert float(opt.state[pref]["mu_product"]) == float(run.mu_product)
    assert rel_l2(run.p.cpu(), p0) > 1e-5, case                               # the parameters moved


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_torch(hip, case, n):
    compare_with_torch(hip, case, n)


@pytest.mark.parametrize("case", STARRED)
def test_kernel_second_trip_and_ragged_end(hip, case):
    """2 100 227 elements: 525 056 vectors for 524 288 threads - a second trip of the 16-byte loop - and a 3-element scalar tail."""
    compare_with_torch(hip, case, WRAP4)


@pytest.mark.parametrize("case", STARRED)
def test_alignment_variants_give_the_aligned_bits(hip, case):
    """Each operand alone one element off 16-byte alignment (the scalar fallback), and all of them, against the aligned run (16-byte
    body plus tail) over two steps - SGD's second step is the first that reads its buffer."""
    kind, o = CASES[case]
    n = 1029
    p0 = _data("opt_p", n)

    def run(shifts):
        r = KernelRun(hip, kind, o, p0, shifts)
        for step in (1, 2):
            r.step(step, _data(f"opt_g{step}", n))
        return [r.p.cpu()] + [g.cpu() for g in r.s.values()]

    base = run(frozenset())
    operands = ["p", "g"] + [nm for nm in abi_of(kind, o, 1, 1.0)[2] if nm]
    for shifts in _shift_sets(operands):
        for a, b in zip(run(shifts), base):
            assert same_bits(a, b), (case, sorted(shifts))


def test_argument_checks(hip):
    lib, st = hip.lib(), hip.stream()
    t = [torch.zeros(8, device=DEV) for _ in range(5)]
    p, g, s0, s1, s2 = (x.data_ptr() for x in t)
    arr = (ctypes.c_float * 8)(1e-3, 0.0, 1e-8, 0.9, 0.999, 0, 0, 0)
    hp = ctypes.addressof(arr)
    ok = lambda *a: lib.rho_optim_step(*a, st)                                                       # noqa: E731
    assert ok(0, 0, p, g, s0, s1, None, 8, hp, 1, None) == 0
    assert ok(0, 0, None, g, s0, s1, None, 8, hp, 1, None) == -1
    assert ok(0, 0, p, None, s0, s1, None, 8, hp, 1, None) == -1
    assert ok(0, 0, p, g, s0, s1, None, 8, None, 1, None) == -1
    assert ok(0, 0, p, g, s0, None, None, 8, hp, 1, None) == -1          # Adam needs exp_avg_sq
    assert ok(0, AMSGRAD, p, g, s0, s1, None, 8, hp, 1, None) == -1      # amsgrad needs the third arena
    assert ok(0, 0, p, g, s0, s1, None, 0, hp, 1, None) == -1
    assert ok(0, 0, p, g, s0, s1, None, 8, hp, 0, None) == -1
    assert ok(9, 0, p, g, s0, s1, None, 8, hp, 1, None) == -1
    assert ok(-1, 0, p, g, s0, s1, None, 8, hp, 1, None) == -1
    assert ok(0, 32, p, g, s0, s1, None, 8, hp, 1, None) == -1           # unknown flag
    assert ok(2, 0, p, g, None, None, None, 8, hp, 1, None) == -1        # hp[3] = 0.9 is SGD's momentum: the buffer is needed
    assert lib.rho_sumsq_partial(None, 8, s0, st) == -1 and lib.rho_sumsq_partial(g, 0, s0, st) == -1
    assert lib.rho_clip_coef(None, 1, 1.0, s0, st) == -1 and lib.rho_clip_coef(g, 0, 1.0, s0, st) == -1
    assert lib.rho_sumsq_blocks(0) == -1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- gradient norm
def sumsq_chain(n, n_partials):
    """L: the longest chain of additions a term passes through in the reduction as written (csrc/optim.hip).  First launch: a thread
    adds one quad per trip into four per-lane sums with an fma (the square is not rounded on its own) - trips additions; the four
    lanes pairwise: 2; the 64-lane butterfly: 6; the four waves pairwise: 2.  Second launch: thread t adds partials t, t + 256, ...:
    ceil(P / 256); butterfly and waves: 6 + 2.  The norm is the square root of that sum; squared back in float64 its one rounding
    counts double: 2."""
    from rho_diffusion_amd.engine import ops
    blocks = ops.sumsq_blocks(n)
    trips = math.ceil(math.ceil(n / 4) / (blocks * 256))
    return trips + 2 + 6 + 2 + math.ceil(n_partials / 256) + 6 + 2 + 2


@pytest.mark.parametrize("n", SMALL + [WRAP4])
def test_sumsq_against_float64(hip, n):
    from rho_diffusion_amd.engine import ops
    x = _data("opt_norm", n)
    ref = float((x.double() ** 2).sum())
    blocks = ops.sumsq_blocks(n)
    assert blocks == min(2048, math.ceil(math.ceil(n / 4) / 256))
    outs = []
    for shift in (0, 0, 1):                                   # twice aligned (same bits run to run), once 4 bytes off (same bits again)
        gx, part, out = Guarded(x, shift), Guarded(blocks), Guarded(2)
        hip.check(hip.lib().rho_sumsq_partial(gx.ptr, n, part.ptr, hip.stream()), "rho_sumsq_partial")
        hip.check(hip.lib().rho_clip_coef(part.ptr, blocks, 1.5, out.ptr, hip.stream()), "rho_clip_coef")
        assert gx.intact() and part.intact() and out.intact() and torch.equal(gx.cpu(), x)
        outs.append((part.cpu(), out.cpu()))
    for part, out in outs[1:]:
        assert same_bits(part, outs[0][0]) and same_bits(out, outs[0][1])
    part, out = outs[0]
    L = sumsq_chain(n, blocks)
    bound = min((L + 1) * U, 1e-5)
    got = float(out[0].double() ** 2)
    print(f"sumsq n={n} L={L} rel={abs(got - ref) / ref:.3e} bound={bound:.3e}")
    assert abs(got - ref) <= bound * ref, (n, got, ref)
    assert abs(float(part.double().sum()) - ref) <= bound * ref
    # coef from the float32 norm the kernel wrote: a sum and a quotient, one rounding each
    norm = float(out[0])
    coef = min(1.0, 1.5 / (norm + float(np.float32(1e-6))))
    assert abs(float(out[1]) - coef) <= 2 * U * (1 + U) * coef, (n, float(out[1]), coef)


def test_sumsq_partials_of_several_arenas_side_by_side(hip):
    """Two arenas' partials in one buffer, one rho_clip_coef over both: the global norm; a max_norm above it gives coef exactly 1."""
    from rho_diffusion_amd.engine import ops
    a, b = _data("opt_norm", 300_001).to(DEV), det_normal((1029,), "opt_norm_b").to(DEV)
    ka, kb = ops.sumsq_blocks(a.numel()), ops.sumsq_blocks(b.numel())
    part, out = torch.full((ka + kb,), float("nan"), device=DEV), torch.empty(2, device=DEV)
    ops.sumsq_partial(a, part[:ka])
    ops.sumsq_partial(b, part[ka:])
    ops.clip_coef(part, 1e9, out)
    ref = math.sqrt(float((a.double() ** 2).sum() + (b.double() ** 2).sum()))
    assert abs(float(out[0]) - ref) <= 1e-5 * ref and float(out[1]) == 1.0


# ----------------------------------------------------------------------------- the optimizer classes
def two_group_params(salt):
    """Two param groups of odd sizes (3 + 1 tensors, 3 601 + 1 102 elements) as device parameters and float64 CPU copies."""
    shapes = [[(37, 53), (1029,), (611,)], [(19, 29, 2)]]
    dev, cpu = [], []
    for gi, group in enumerate(shapes):
        ts = [det_normal(s, f"{salt}_p{gi}_{i}") for i, s in enumerate(group)]
        dev.append([nn.Parameter(t.clone().to(DEV)) for t in ts])
        cpu.append([nn.Parameter(t.double().clone()) for t in ts])
    return dev, cpu


def set_grads(dev, cpu, salt, step):
    for gi, (gd, gc) in enumerate(zip(dev, cpu)):
        for i, (pd, pc) in enumerate(zip(gd, gc)):
            g = det_normal(tuple(pd.shape), f"{salt}_g{step}_{gi}_{i}")
            pd.grad = g.to(DEV) if pd.grad is None else pd.grad.copy_(g.to(DEV))
            pc.grad = g.double()


CLIP_CASES = {"Adam": ("adam_amsgrad*", "HipAdam"), "SGD": ("sgd_dampening*", "HipSGD"), "AdamW": ("adamw", "HipAdamW")}


@pytest.mark.parametrize("name", list(CLIP_CASES))
def test_clipping_two_groups_one_global_norm(hip, name):
    """Norm above max_grad_norm: three steps against clip_grad_norm_ + torch.optim.X on float64 copies, both bars, over two param
    groups with different lr clipped by ONE norm; the gradient arenas are not rewritten; last_grad_norm is the pre-clip norm.
    The coefficient the kernel multiplies by is float32: min(1, max / (norm + 1e-6)) from a norm within ((L + 1) / 2 + 1) U of the
    true one (sumsq_chain; the square root halves the relative error and rounds once), then a sum and a quotient: the shadow takes
    the float64 coefficient with a bound of ((L + 1) / 2 + 3) U on it."""
    from rho_diffusion_amd import optim as O
    from rho_diffusion_amd.engine import ops
    case, cls = CLIP_CASES[name]
    kind, o = CASES[case]
    dev, cpu = two_group_params("clip")
    lrs = [o["lr"], r32(o["lr"] * 0.5)]
    hip_opt = getattr(O, cls)([dict(params=g, lr=lr) for g, lr in zip(dev, lrs)], max_grad_norm=1.0,
                              **{k: v for k, v in o.items() if k != "lr"})
    ref_opt = getattr(torch.optim, kind)([dict(params=g, lr=lr) for g, lr in zip(cpu, lrs)], foreach=False,
                                         **{k: v for k, v in o.items() if k != "lr"})
    opts = [dict(o, lr=lr) for lr in lrs]
    sh_p = [B(torch.cat([p.detach().reshape(-1) for p in g])) for g in cpu]
    sh_s = [shadow_states(kind, o, int(p.v.numel())) for p in sh_p]
    arena = hip_opt.build_arena()
    n_part = sum(ops.sumsq_blocks(a["grad"].numel()) for a in arena)
    L = max(sumsq_chain(a["grad"].numel(), n_part) for a in arena)
    for step in (1, 2, 3):
        set_grads(dev, cpu, "clip", step)
        grads_before = [a["grad"].clone() for a in arena]
        hip_opt.step()
        norm64 = float(torch.nn.utils.clip_grad_norm_([p for g in cpu for p in g], 1.0, foreach=False))
        assert norm64 > 10.0                                                           # well above max_grad_norm: clipping is active
        coef64 = 1.0 / (norm64 + 1e-6)                                                 # what clip_grad_norm_ just multiplied by
        ref_opt.step()
        assert hip_opt.last_grad_norm.shape == (1,) and hip_opt.last_grad_norm.device == hip_opt.build_arena()[0]["grad"].device
        assert abs(float(hip_opt.last_grad_norm) - norm64) <= ((L + 1) / 2 + 1) * U * norm64
        gs = B(coef64, ((L + 1) / 2 + 3) * U * coef64)
        for gi, a in enumerate(arena):
            assert torch.equal(a["grad"], grads_before[gi])                            # the gradient arena is not rewritten
            g_unclipped = B(grads_before[gi].double().cpu())                           # the kernel scales as it loads
            sh_p[gi] = _shadow(kind, opts[gi], step, sh_p[gi], g_unclipped, sh_s[gi], gs=gs)
            ref = torch.cat([p.detach().reshape(-1) for p in cpu[gi]])
            check_against(a["flat"].cpu(), ref, sh_p[gi], (name, "p", gi, step))


@pytest.mark.parametrize("name", ["Adam", "SGD"])
def test_clipping_below_the_norm_is_the_unclipped_step(hip, name):
    """coef is exactly 1.0 and g * 1.0 is g: parameters and states bit-equal to those of the optimizer without max_grad_norm, which
    makes no extra launch.  (HipAdamW is not in this list: unclipped it runs rho_adamw, clipped the AdamW kind of rho_optim_step,
    and those two kernels associate differently.)"""
    from rho_diffusion_amd import optim as O
    case, cls = CLIP_CASES[name]
    kind, o = CASES[case]
    flats = []
    for max_norm in (None, 1e6):
        dev, cpu = two_group_params("clipb")
        opt = getattr(O, cls)([dict(params=g) for g in dev], max_grad_norm=max_norm, **o)
        for step in (1, 2):
            set_grads(dev, cpu, "clipb", step)
            opt.step()
        if max_norm is None:
            assert opt.last_grad_norm is None and opt._clip_ws is None                  # no extra launch, no workspace
        else:
            assert 10.0 < float(opt.last_grad_norm) < 1e6
        flats.append([{k: v.clone() for k, v in a.items() if isinstance(v, torch.Tensor)} for a in opt.build_arena()])
    for a, b in zip(*flats):
        assert a.keys() == b.keys()
        for k in a:
            assert same_bits(a[k], b[k]), (name, k)


def test_hip_adamw_default_path_still_calls_rho_adamw(hip, monkeypatch):
    """amsgrad = maximize = False and no clipping: rho_adamw, as before; any of the three: rho_optim_step."""
    from rho_diffusion_amd import optim as O
    from rho_diffusion_amd.engine import ops
    calls = []
    monkeypatch.setattr(ops, "adamw", lambda *a, _f=ops.adamw: (calls.append("adamw"), _f(*a))[1])
    monkeypatch.setattr(ops, "optim_step", lambda *a, _f=ops.optim_step: (calls.append("optim_step"), _f(*a))[1])
    for kw, want in (({}, "adamw"), ({"amsgrad": True}, "optim_step"), ({"maximize": True}, "optim_step"),
                     ({"max_grad_norm": 1.0}, "optim_step")):
        dev, cpu = two_group_params("dflt")
        opt = O.HipAdamW([p for g in dev for p in g], **kw)
        set_grads(dev, cpu, "dflt", 1)
        del calls[:]
        opt.step()
        assert calls == [want], (kw, calls)


@pytest.mark.parametrize("name", ["HipAdamW", "HipAdam", "HipSGD"])
def test_checkpoint_resume_is_bit_equal(hip, name):
    """Two steps, state_dict(), a fresh optimizer over fresh parameters loads it (plus the parameters): its third step is bit-equal
    to the uninterrupted run's - parameters and every state arena."""
    from rho_diffusion_amd import optim as O
    kw = {"HipAdamW": dict(lr=1e-3), "HipAdam": dict(lr=1e-3, amsgrad=True, weight_decay=1e-2),
          "HipSGD": dict(lr=1e-2, momentum=0.9, weight_decay=1e-2)}[name]
    dev, cpu = two_group_params("ckpt")
    opt = getattr(O, name)([dict(params=g) for g in dev], **kw)
    for step in (1, 2):
        set_grads(dev, cpu, "ckpt", step)
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3]
    sd = {"state": {k: {kk: (vv.clone() if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()}
                    for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
    weights = [[p.detach().clone() for p in g] for g in dev]
    dev2, cpu2 = two_group_params("ckpt_other")                     # other values: everything must come from the checkpoint
    with torch.no_grad():
        for g2, gw in zip(dev2, weights):
            for p2, w in zip(g2, gw):
                p2.copy_(w)
    opt2 = getattr(O, name)([dict(params=g) for g in dev2], **kw)
    opt2.load_state_dict(sd)
    for o_, d_ in ((opt, dev), (opt2, dev2)):
        set_grads(d_, cpu, "ckpt", 3)
        o_.step()
    for a, b in zip(opt.build_arena(), opt2.build_arena()):
        assert name == "HipSGD" or a["step"] == b["step"] == 3       # torch's SGD state has no step: a loaded buffer means "past step 1"
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert same_bits(a[k], b[k]), (name, k)
    for g, g2 in zip(dev, dev2):
        for p, p2 in zip(g, g2):
            assert same_bits(p.detach(), p2.detach())


@pytest.mark.parametrize("case", STARRED)
def test_state_dict_loads_into_torch_with_a_permuted_arena(hip, case):
    """arena_order reversed: the arena is laid out last parameter first, the state_dict is still indexed in param_groups order.
    After two fused steps it loads into torch.optim.X over float64 copies of the parameters; that optimizer's third step agrees with
    the fused third step at both bars (the float64 optimizer starts from float32 state: the shadow starts there too, with no carried
    bound).  And back: torch's dict loads into a fresh fused optimizer, whose third step is bit-equal."""
    from rho_diffusion_amd import optim as O
    kind, o = CASES[case]
    dev, cpu = two_group_params("perm")
    ps = [p for g in dev for p in g]
    opt = O.fused_optimizer_class(getattr(torch.optim, kind))(ps, arena_order=ps[::-1], **o)
    for step in (1, 2):
        set_grads(dev, cpu, "perm", step)
        opt.step()
    a = opt.build_arena()[0]
    assert [id(p) for p in a["params"]] == [id(p) for p in ps[::-1]]
    ref_ps = [nn.Parameter(p.detach().double().cpu()) for p in ps]
    ref_opt = getattr(torch.optim, kind)(ref_ps, foreach=False, **o)
    ref_opt.load_state_dict(opt.state_dict())
    back = ref_opt.state_dict()
    # shadow from the float32 state, per parameter
    names = [nm for nm in abi_of(kind, o, 1, 1.0)[2] if nm]
    sh = []
    for i, rp in enumerate(ref_ps):
        st = ref_opt.state[rp]
        assert all(st[nm].dtype == torch.float64 and st[nm].shape == rp.shape for nm in names), (case, i)
        if kind != "SGD":
            assert float(st["step"]) == 2.0
        sh.append((B(rp.detach().reshape(-1).clone()), {nm: B(st[nm].reshape(-1).clone()) for nm in names}))
    mu_product = mu_product_kernel = None
    if kind == "NAdam":            # torch's load casts mu_product to the parameters' float64 and goes on in float64; the arena stays float32
        loaded = float(ref_opt.state[ref_ps[0]]["mu_product"])
        mu_product = loaded * nadam_mu(o, 3)
        mu_product_kernel = float(torch.tensor(loaded, dtype=torch.float32) * nadam_mu(o, 3))
    # a second fused optimizer restored from torch's dict
    dev2, _ = two_group_params("perm")
    ps2 = [p for g in dev2 for p in g]
    with torch.no_grad():
        for p2, p in zip(ps2, ps):
            p2.copy_(p)
    opt2 = O.fused_optimizer_class(getattr(torch.optim, kind))(ps2, arena_order=ps2[::-1], **o)
    opt2.load_state_dict(back)
    set_grads(dev, cpu, "perm", 3)
    for p2, p in zip(ps2, ps):
        p2.grad = p.grad.clone()
    for rp, p in zip(ref_ps, ps):
        rp.grad = p.grad.detach().double().cpu()
    opt.step()
    opt2.step()
    ref_opt.step()
    for i, (p, p2, rp) in enumerate(zip(ps, ps2, ref_ps)):
        assert same_bits(p.detach(), p2.detach()), (case, i)
        shp, shs = sh[i]
        shp = _shadow(kind, o, 3, shp, B(rp.grad.reshape(-1)), shs, mu_product=mu_product, mu_product_kernel=mu_product_kernel)
        check_against(p.detach().cpu(), rp, shp, (case, "p", i))
    sd3, ref3 = opt.state_dict()["state"], ref_opt.state_dict()["state"]
    for i in range(len(ps)):
        for nm in names:
            assert rel_l2(sd3[i][nm].cpu(), ref3[i][nm]) < 1e-6, (case, i, nm)


# ----------------------------------------------------------------------------- pipeline
def _tiny_ddpm(optimizer, opt_kwargs):
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    g4 = load_golden("g4_unet.npz")
    kw, xshape, _ = UNET_CASES["tiny2d"]
    ddpm = DDPM(UNet, dict(kw, compute_dtype="fp32"), LinearSchedule(1000, 1e-3, 0.02), nn.MSELoss, optimizer=optimizer,
                opt_kwargs=opt_kwargs)
    ddpm.backbone.load_state_dict(det_state_dict(golden_template(g4, "tiny2d"), "tiny2d"))
    ddpm = ddpm.to(DEV).train()
    eps = det_normal(xshape, "eps").to(DEV)
    tq = torch.tensor([300, 700])
    ddpm.noise = lambda data: eps
    ddpm.random_timesteps = lambda bs: tq
    return ddpm, det_uniform(xshape, "x0", 0.0, 1.0).to(DEV)


# learning rates: small enough that four steps on one fixed batch descend whatever the curvature (RMSprop's first step is
# lr / sqrt(1 - alpha) = 10 lr per weight, so its lr is a tenth of Adam's)
PIPE = {"Adam": ("HipAdam", {"lr": 2e-4}), "SGD": ("HipSGD", {"lr": 1e-3, "momentum": 0.9}), "RMSprop": ("HipRMSprop", {"lr": 2e-5})}


@pytest.mark.parametrize("name", list(PIPE))
def test_pipeline_builds_and_trains_with_the_fused_class(name):
    from rho_diffusion_amd import optim as O
    from rho_diffusion_amd.optim import optimizer_kwargs
    cls, user = PIPE[name]
    ddpm, x0 = _tiny_ddpm(name, user)
    opt = ddpm.configure_optimizers()["optimizer"]
    assert type(opt) is getattr(O, cls)
    ref_params = [p.detach().clone().requires_grad_(True) for p in ddpm.parameters()]
    ref_opt = getattr(torch.optim, name)(ref_params, **optimizer_kwargs(getattr(torch.optim, name), user))
    losses = []
    for step in range(4):
        opt.zero_grad()
        loss = ddpm.training_step(x0)
        loss.backward()
        if step == 0:
            for rp, p in zip(ref_params, ddpm.parameters()):
                rp.grad = p.grad.detach().clone()
            ref_opt.step()
        opt.step()
        if step == 0:
            for rp, p in zip(ref_params, ddpm.parameters()):
                assert rel_l2(p, rp) < 1e-6
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def test_dp_trainer_builds_the_configured_optimizer_and_clips():
    from rho_diffusion_amd import optim as O
    from rho_diffusion_amd.trainer import DPTrainer
    ddpm, x0 = _tiny_ddpm("SGD", {"lr": 1e-3, "momentum": 0.9})
    trainer = DPTrainer(ddpm, max_grad_norm=0.5)
    assert type(trainer.opt) is O.HipSGD and trainer.opt.max_grad_norm == 0.5
    g = trainer.opt.param_groups[0]
    assert g["momentum"] == 0.9 and g["lr"] == 1e-3 and g["weight_decay"] == 1e-2
    before = trainer.opt.build_arena()[0]["flat"].clone()
    loss = trainer.step(x0)
    norm = trainer.opt.last_grad_norm
    assert norm.shape == (1,) and norm.is_cuda and norm.device == trainer.opt.flat_grads[0].device
    assert math.isfinite(float(norm)) and float(norm) > 0
    ref = float(trainer.opt.flat_grads[0].double().norm())
    assert abs(float(norm) - ref) <= 1e-5 * ref
    assert torch.isfinite(loss) and not torch.equal(before, trainer.opt.build_arena()[0]["flat"])
    ddpm2, _ = _tiny_ddpm("AdamW", {"lr": 2e-4})
    default = DPTrainer(ddpm2).opt
    assert type(default) is O.HipAdamW and default.max_grad_norm is None and default.param_groups[0]["lr"] == 2e-4
