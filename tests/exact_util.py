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


def mismatch_report(got: torch.Tensor, want: torch.Tensor, what: str) -> str:
    bad = ~(got == want)                      # NaN in either counts as a mismatch
    idx = bad.nonzero()
    first = tuple(int(i) for i in idx[0])
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements differ; first at {first}: got {got[first].item()!r}, "
             f"want {want[first].item()!r}"]
    for ax in range(got.dim()):
        u = torch.unique(idx[:, ax]).tolist()
        lines.append(f"  axis {ax} (extent {got.shape[ax]}): {len(u)} indices with a mismatch: {u[:16]}{' ...' if len(u) > 16 else ''}")
    return "\n".join(lines)


def assert_bit_equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """got == want element for element (so -0 equals +0, NaN equals nothing); the failure names the first index and, per axis,
    the indices that hold a mismatch - a face, a tile or a channel block."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    got, want = got.double(), want.double()
    if bool((got == want).all()):
        return
    raise AssertionError(mismatch_report(got, want, what))


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
