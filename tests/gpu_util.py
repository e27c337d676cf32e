"""Helpers for the -m gpu parity tests (HIP path vs CPU oracle on the same seeded inputs)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from helpers import rel_l2

DEV = "cuda"


def to_cl(x: torch.Tensor, dtype) -> torch.Tensor:
    """[N, C, *S] -> channels-last [N, D, H, W, C] on the GPU (test-side plumbing)."""
    n, c = x.shape[:2]
    s = list(x.shape[2:])
    while len(s) < 3:
        s.insert(0, 1)
    y = x.reshape(n, c, *s).permute(0, 2, 3, 4, 1).contiguous()
    return y.to(DEV).to(dtype)


def from_cl(y: torch.Tensor, dims: int) -> torch.Tensor:
    """channels-last [N, D, H, W, C] -> [N, C, *S] float32 on the CPU."""
    n, d, h, w, c = y.shape
    out = y.float().cpu().permute(0, 4, 1, 2, 3)
    spatial = [d, h, w][3 - dims:]
    return out.reshape(n, c, *spatial).contiguous()


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


def rnd(x: torch.Tensor, dtype) -> torch.Tensor:
    return bf16_round(x) if dtype == torch.bfloat16 else x


def tol(dtype, f32=2e-5, bf16=6e-3):
    return bf16 if dtype == torch.bfloat16 else f32


# ----------------------------------------------------------------------------- the streaming-kernel edge tests
PAD = 64
SENT = -776.0                      # exact in float32 and bfloat16; no kernel under these tests produces it from their inputs


class Guarded:
    """A device copy of a 1-D CPU tensor (or n NaNs) placed ``shift`` elements past a 256-byte aligned address, with at least PAD
    sentinel elements on either side."""

    def __init__(self, src, shift: int = 0, dtype=torch.float32):
        n = src if isinstance(src, int) else src.numel()
        dtype = dtype if isinstance(src, int) else src.dtype
        self.n, self.shift = n, shift
        self.buf = torch.full((PAD + shift + n + PAD,), SENT, dtype=dtype, device=DEV)
        self.v = self.buf[PAD + shift: PAD + shift + n]
        if isinstance(src, int):
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(src)
        assert self.v.data_ptr() % 16 == (shift * self.buf.element_size()) % 16

    @property
    def ptr(self) -> int:
        return self.v.data_ptr()

    def cpu(self) -> torch.Tensor:
        return self.v.cpu()

    def intact(self) -> bool:
        lo, hi = self.buf[:PAD + self.shift], self.buf[PAD + self.shift + self.n:]
        return hi.numel() == PAD and bool((lo == SENT).all()) and bool((hi == SENT).all())


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(bits(a), bits(b))


def check_bound(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what, rel_bar=None):
    """Per-element |got - ref| <= bound (float64 tensors), then rel-L2 < rel_bar where one is given."""
    got = got.double().cpu().flatten()
    ref, bound = ref.flatten(), bound.flatten()
    assert torch.isfinite(got).all(), what
    excess = (got - ref).abs() - bound
    i = int(excess.argmax())
    assert float(excess[i]) <= 0.0, (what, "element", i, float(got[i]), float(ref[i]), "bound", float(bound[i]))
    if rel_bar is not None:
        assert rel_l2(got, ref) < rel_bar, what
