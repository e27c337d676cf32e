"""Running error analysis over pairs (value, error bound) in float64, shared by test_gpu_optim.py (whose docstring explains the count)
and gd_step_ref.py: each float32 operation adds U = 2^-24 times the magnitude of its result to the first-order propagation of its
operands' bounds
    a + b: ea + eb      a * b: |a| eb + |b| ea + ea eb      a / b: (ea + |a / b| eb) / (|b| - eb)
    sqrt(a): sqrt(a) - sqrt(max(a - ea, 0))      max, |.|, negation: exact.
Importable without a GPU."""
import torch

U = 2.0 ** -24


class B:
    """value and a bound on |float32 result - value|, float64 tensors"""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=torch.float64)


def _r(v, e):
    return B(v, e + U * (v.abs() + e))               # one rounding of a result that is itself within e of v


def add(a, b):
    return _r(a.v + b.v, a.e + b.e)


def sub(a, b):
    return _r(a.v - b.v, a.e + b.e)


def mul(a, b):
    return _r(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)


def div(a, b):
    assert bool((b.v.abs() > b.e).all())
    q = a.v / b.v
    return _r(q, (a.e + q.abs() * b.e) / (b.v.abs() - b.e))


def sqrt(a):
    assert bool((a.v >= 0).all())
    v = a.v.sqrt()
    return _r(v, v - (a.v - a.e).clamp_min(0.0).sqrt())


def maxf(a, b):
    return B(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))


def neg(a):
    return B(-a.v, a.e)
