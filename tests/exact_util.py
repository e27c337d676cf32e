"""Helpers of the integer-operand tests (test_exact_cases_host.py, test_gpu_exact_*.py).

Small-integer operands make every product, every fp32 partial sum (in any order: split-K slabs, atomics) and every stored result
exact, so a kernel must equal the fp64 reference bit for bit: one wrong, missing or doubled contribution fails and is named.
Nothing here touches the GPU at import."""
from __future__ import annotations

import math

import torch

from detdata import det_normal

GUARD = 4096           # guard elements on either side of an output
GUARD_VALUE = 1.5


def int_tensor(shape, tag: str, scale: float, clamp: float) -> torch.Tensor:
    """Deterministic integer-valued float32 tensor: round(scale * z) clamped to +-clamp."""
    return det_normal(tuple(shape), tag).mul(scale).round().clamp(-clamp, clamp)


def int_choice(shape, tag: str, values) -> torch.Tensor:
    """Deterministic float32 tensor drawing from `values` (about uniformly)."""
    v = torch.tensor(list(values), dtype=torch.float32)
    idx = det_normal(tuple(shape), tag).mul(997.0).abs().floor().long() % len(values)
    return v[idx]


def _axis_lines(idx: torch.Tensor, shape) -> list:
    """Per axis, the indices that hold a failing element (idx: the [k, dim] result of nonzero())."""
    out = []
    for ax in range(len(shape)):
        u = torch.unique(idx[:, ax]).tolist()
        out.append(f"  axis {ax} (extent {shape[ax]}): {len(u)} indices with a mismatch: {u[:16]}{' ...' if len(u) > 16 else ''}")
    return out


def mismatch_report(got: torch.Tensor, want: torch.Tensor, what: str) -> str:
    bad = ~(got == want)                      # NaN in either counts as a mismatch
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements differ; first at {first}: got {got[first].item()!r}, "
             f"want {want[first].item()!r}"]
    return "\n".join(lines + _axis_lines(idx, got.shape))


def assert_bit_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """got == want element for element (so -0 equals +0, NaN equals nothing); the failure names the first index and, per axis,
    the indices that hold a mismatch - a face, a tile or a channel block."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    got, want = got.double(), want.double()
    if bool((got == want).all()):
        return
    raise AssertionError(mismatch_report(got, want, what))


def f32_ulp(v: torch.Tensor) -> torch.Tensor:
    """float64: the spacing of fp32 numbers at |v| (2^-149 below the smallest normal)."""
    _, e = torch.frexp(v.double().abs())                      # |v| = m * 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - 24).clamp_min(-149))


def assert_within_ulps(got: torch.Tensor, want64: torch.Tensor, ulps: float, what: str, mag: torch.Tensor = None) -> float:
    """|got - want| <= ulps * ulp32(want) for EVERY element (fp32 spacing at the fp64 reference value; NaN fails; ulps = 0 is
    bit equality).  `mag` (same shape, optional) replaces want as the magnitude whose spacing counts - for a sum of terms that may
    cancel, the sum of the terms' magnitudes.  The failure report has the shape of mismatch_report; returns the largest error met,
    in those units."""
    got, want = got.detach().cpu().double(), want64.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    unit = f32_ulp(want if mag is None else mag.detach().cpu().double().expand_as(want))
    err = (got - want).abs() / unit
    ok = err <= ulps
    if bool(ok.all()):
        return float(err.max()) if err.numel() else 0.0
    idx = (~ok).nonzero()
    first = tuple(int(i) for i in idx[0])
    worst = float(torch.where(ok | torch.isnan(err), torch.zeros_like(err), err).max())
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements are more than {ulps} fp32 ulp(s) off (worst {worst:.3g}); first at {first}: "
             f"got {got[first].item()!r}, want {want[first].item()!r}"]
    raise AssertionError("\n".join(lines + _axis_lines(idx, got.shape)))


def assert_within_abs(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """|got - want| <= bound for EVERY element (bound: a number or a tensor of want's shape); reports like assert_within_ulps and
    returns the largest |got - want| met."""
    got, want = got.detach().cpu().double(), want64.detach().cpu().double()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    err = (got - want).abs()
    ok = err <= (bound.detach().cpu().double() if torch.is_tensor(bound) else float(bound))
    if bool(ok.all()):
        return float(err.max()) if err.numel() else 0.0
    idx = (~ok).nonzero()
    first = tuple(int(i) for i in idx[0])
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements are outside their bound; first at {first}: got {got[first].item()!r}, "
             f"want {want[first].item()!r}"]
    raise AssertionError("\n".join(lines + _axis_lines(idx, got.shape)))


# The tie rule for a bf16 result.  A kernel computes the value in fp32 within a derived bound and rounds it to bf16 once.  If the
# fp64 reference r is farther than a margin from every bf16 rounding tie (the midpoint of two neighbouring bf16 numbers), every fp32
# value inside the bound rounds to the same bf16 number, and the kernel must store bf16(r) exactly.  Closer than the margin, either
# neighbour passes.  The margin is four times the derived fp32 bound of the value.  The share of elements allowed "either neighbour"
# is a property of the inputs: the host twins assert it stays at or below TIE_SHARE_MAX per tensor.
TIE_MARGIN_FACTOR = 4
TIE_SHARE_MAX = 0.01


def tie_margin(ulps, mag64: torch.Tensor) -> torch.Tensor:
    """TIE_MARGIN_FACTOR times the fp32 bound `ulps` * ulp32(mag) of a value whose terms have the magnitude sum `mag`; 0 where
    mag = 0 (every term is an exact zero)."""
    m = mag64.detach().cpu().double()
    return torch.where(m == 0, torch.zeros_like(m), TIE_MARGIN_FACTOR * ulps * f32_ulp(m))


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """float64: the spacing of bf16 numbers at |v| (8 significant bits; normal range)."""
    return f32_ulp(v) * 65536.0


def bf16_store_bound(ref64: torch.Tensor, f32_bound: torch.Tensor) -> torch.Tensor:
    """|bf16(v) - r| for an fp32 value v with |v - r| <= f32_bound rounded once to bf16: the fp32 bound plus half a bf16 ulp at the
    largest magnitude v can have."""
    return f32_bound + 0.5 * bf16_ulp(ref64.double().abs() + f32_bound)


def bf16_round(v64: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bf16 number (ties to even), in one rounding (through fp32 it would be two).  Normal range only."""
    v = v64.double()
    a = v.abs()
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, -125), e)
    ulp = torch.ldexp(torch.ones_like(a), e - 8)
    return torch.sign(v) * torch.round(a / ulp) * ulp          # torch.round: halves to even


def tie_share(ref64: torch.Tensor, margin: torch.Tensor) -> float:
    """Fraction of elements whose reference is within `margin` (absolute, per element or a number) of a bf16 rounding tie, i.e. for
    which bf16(r - margin) and bf16(r + margin) differ."""
    r = ref64.detach().cpu().double()
    m = margin.detach().cpu().double() if torch.is_tensor(margin) else float(margin)
    return float((bf16_round(r - m) != bf16_round(r + m)).double().mean()) if r.numel() else 0.0


def assert_bf16_tie_rule(got: torch.Tensor, ref64: torch.Tensor, margin: torch.Tensor, what: str) -> float:
    """The tie rule above for EVERY element of a bf16 tensor: bf16(r - margin) <= got <= bf16(r + margin).  Away from a tie both ends
    are bf16(r) and the element must equal it; within the margin of a tie they are its two neighbours (more than two bf16 numbers
    only where the value cancels so far that the margin exceeds a bf16 ulp).  Returns the share of elements that had a choice."""
    got, r = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert tuple(got.shape) == tuple(r.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(r.shape)}"
    m = (margin.detach().cpu().double() if torch.is_tensor(margin) else torch.tensor(float(margin), dtype=torch.float64)).expand_as(r)
    lo, hi = bf16_round(r - m), bf16_round(r + m)
    ok = (got >= lo) & (got <= hi)
    if bool(ok.all()):
        return float((lo != hi).double().mean()) if r.numel() else 0.0
    idx = (~ok).nonzero()
    first = tuple(int(i) for i in idx[0])
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} bf16 elements break the tie rule; first at {first}: got {got[first].item()!r}, "
             f"reference {r[first].item()!r}, allowed [{lo[first].item()!r}, {hi[first].item()!r}]"]
    raise AssertionError("\n".join(lines + _axis_lines(idx, got.shape)))


def guarded(shape, dtype, device="cuda"):
    """(flat, view): a NaN-filled tensor of `shape` inside a larger allocation whose margins hold 1.5."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD,), GUARD_VALUE, dtype=dtype, device=device)
    flat[GUARD:GUARD + n] = float("nan")
    return flat, flat[GUARD:GUARD + n].view(*shape)


def guards_intact(flat: torch.Tensor) -> bool:
    return bool((flat[:GUARD] == GUARD_VALUE).all()) and bool((flat[-GUARD:] == GUARD_VALUE).all())


def guarded_copy(src: torch.Tensor, dtype, device="cuda"):
    """As `guarded`, prefilled with `src` instead of NaN (an output that a launch accumulates onto)."""
    flat, view = guarded(tuple(src.shape), dtype, device)
    view.copy_(src.to(device).to(dtype))
    return flat, view


# Representability of the REFERENCE (conditions on the inputs of a case, never on a kernel's output): a case that violates one gets
# sparser inputs, not a tolerance.
def check_bf16_exact(ref: torch.Tensor, what: str = "reference") -> None:
    """Integers up to 256 are exact in bf16 (8 significant bits)."""
    m = float(ref.abs().max()) if ref.numel() else 0.0
    assert m <= 256, f"{what}: max |value| {m} is not exactly representable in bf16"
    assert bool((ref == ref.round()).all()), f"{what}: not integer-valued"


def check_f32_exact(ref: torch.Tensor, what: str = "reference") -> None:
    """Integers below 2^24 are exact in fp32, and so is every partial sum of such terms of one sign pattern bounded by it."""
    m = float(ref.abs().max()) if ref.numel() else 0.0
    assert m < 2 ** 24, f"{what}: max |value| {m} is not exactly representable in fp32"
    assert bool((ref == ref.round()).all()), f"{what}: not integer-valued"


def check_f32_grid(ref: torch.Tensor, step: float, what: str = "reference") -> None:
    """Multiples of a power of two `step` with fewer than 2^24 steps are exact in fp32 (halves arise where rstd = 0.5)."""
    k = ref.double() / step
    m = float(k.abs().max()) if k.numel() else 0.0
    assert m < 2 ** 24, f"{what}: max |value| {m * step} is not exactly representable in fp32 on a grid of {step}"
    assert bool((k == k.round()).all()), f"{what}: not a multiple of {step}"
