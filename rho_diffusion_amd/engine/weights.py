"""Conv parameters prepared for the kernels.  ``_ConvW.layouts`` is the one list of a convolution's layouts and ``_ConvW._walk`` the
one walk over it: into the one-launch ``ops.PrepTable`` (``prep_into``) or, for parameters that are not contiguous, into
``ops.EagerPrep`` (``refresh``)."""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import torch
from torch import nn

from .. import hip
from . import ops

Tensor = torch.Tensor


class _ConvW:
    """A conv weight prepared for the kernels: forward [taps, coutp, cinp] and (training) data-gradient
    [taps, ceil32(cin), coutp] layouts in the engine dtype + padded fp32 bias."""

    def __init__(self, weight: nn.Parameter, bias: nn.Parameter, dtype, row_src: Optional[Tensor] = None):
        self.weight, self.bias_param, self.dtype = weight, bias, dtype
        self.cout, self.cin = weight.shape[0], weight.shape[1]
        self.kernel = k = ops.kernel3(weight)
        self.taps = int(k[0] * k[1] * k[2])
        self._geometry()
        _, self.coutp, self.cinp = ops.prepared_shape(hip.PREP_FWD, (self.cout, self.cin), dtype)
        self.row_src = row_src
        dev = weight.device
        self.w = torch.empty(self.taps, self.coutp, self.cinp, dtype=dtype, device=dev)
        self.b = torch.zeros(self.coutp, dtype=torch.float32, device=dev)
        self.wd: Optional[Tensor] = None     # dgrad weights, allocated with the first training plan
        self.zero_bias: Optional[Tensor] = None
        self.wph: Optional[list] = None      # sub-pixel phase weights [(phase_hw, tensor)] of a conv behind a nearest x2 upsample
        self.wphd: Optional[list] = None     # ... and their data-gradient layouts (training plans)
        self.ws2: Optional[list] = None      # parity split of a stride-2 conv: forward taps per input parity
        self.ws2d: Optional[list] = None     # ... data-gradient taps per parity of dX
        self.refresh()

    def _geometry(self) -> None:          # subclasses re-interpret the parameter (see _StemAsGemm / _HeadAsGemm)
        pass

    def _source(self) -> Tensor:
        w = self.weight.detach()
        return w if w.is_contiguous() else w.contiguous()

    def _bias_source(self) -> Tensor:
        return self.bias_param.detach()

    def _dgrad_rows(self) -> int:
        return ops.prepared_shape(hip.PREP_DGRAD, (self.cout, self.cin), self.dtype)[1]

    def _want_zero_bias(self) -> None:          # the bias of every data-gradient launch: one zero per row of the dgrad weights
        if self.zero_bias is None:
            self.zero_bias = torch.zeros(self._dgrad_rows(), dtype=torch.float32, device=self.w.device)

    def enable_dgrad(self) -> None:
        if self.wd is None:
            self.wd = torch.empty(self.taps, self._dgrad_rows(), self.coutp, dtype=self.dtype, device=self.w.device)
            self._want_zero_bias()
            ops.EagerPrep().add_dgrad(self._source(), self.wd, self.row_src, cout=self.cout, cin=self.cin, k=self.kernel)

    def enable_phases(self, up_hw, dgrad: bool = False) -> None:
        """The conv sits behind a nearest x2 upsample of the axes flagged in up_hw: one 2-tap weight set per output parity
        (and, for training plans, its data-gradient layout)."""
        hs = (1, 2) if up_hw[0] else (0,)
        ws = (1, 2) if up_hw[1] else (0,)
        if self.wph is None:
            self.wph = [((a, b), ops.prep_conv_weight_phase(self._source(), self.dtype, (a, b))) for a in hs for b in ws]
        if dgrad and self.wphd is None:
            self.wphd = [((a, b), ops.prep_conv_weight_phase(self._source(), self.dtype, (a, b), dgrad=True)) for a in hs for b in ws]
            self._want_zero_bias()

    def phase_kernel(self, ph) -> Tuple[int, int, int]:
        """Kernel shape of the sub-pixel phase ``ph`` = (phase_h, phase_w): 2 taps along every upsampled axis."""
        return (self.kernel[0], 2 if ph[0] else self.kernel[1], 2 if ph[1] else self.kernel[2])

    S2_FWD = {0: (1,), 1: (0, 2)}        # taps of the stride-2 forward on the even / odd input rows of a strided axis
    S2_BWD = {0: (1,), 1: (2, 0)}        # taps of its data gradient on the even / odd rows of dX

    def _s2_args(self, ab, dgrad: bool) -> dict:
        """Arguments of rho_prep_conv_weight_sel for the parity ``ab`` = (parity_h, parity_w) of the forward / data-gradient split."""
        if dgrad:
            return dict(sel_hw=(self.S2_BWD[ab[0]], self.S2_BWD[ab[1]]), flip_d=True, dgrad=True)
        return dict(sel_hw=(self.S2_FWD[ab[0]], self.S2_FWD[ab[1]]))

    def enable_s2(self, dgrad: bool = False) -> None:
        """3-D stride-(1, 2, 2) conv as stride-1 launches per parity (rho_prep_conv_weight_sel)."""
        par = [(a, b) for a in (0, 1) for b in (0, 1)]
        if self.ws2 is None:
            self.ws2 = [(ab, ops.prep_conv_weight_sel(self._source(), self.dtype, **self._s2_args(ab, False))) for ab in par]
            self.zero_b = torch.zeros(self.coutp, dtype=torch.float32, device=self.w.device)
        if dgrad and self.ws2d is None:
            self.ws2d = [(ab, ops.prep_conv_weight_sel(self._source(), self.dtype, **self._s2_args(ab, True))) for ab in par]
            self._want_zero_bias()

    # batchable: every layout is a gather out of the parameter's own storage (rho_prep_batch reads the parameter directly)
    batchable = True

    def layout_signature(self) -> tuple:
        return (id(self), self.weight.data_ptr(), self.bias_param.data_ptr(), self.wd is not None, self.wph is not None,
                self.wphd is not None, self.ws2 is not None, self.ws2d is not None, self.weight.is_contiguous())

    def layouts(self) -> Iterator[Tuple[str, Tensor, dict]]:
        """(kind, buffer, arguments) of every prepared layout this conv has now - the ONE enumeration ``prep_into`` and ``refresh``
        walk: a new layout is listed here."""
        yield "fwd", self.w, dict(row_src=self.row_src)
        yield "bias", self.b, {}
        if self.wd is not None:
            yield "dgrad", self.wd, dict(col_src=self.row_src)
        for lst, dg in ((self.wph, False), (self.wphd, True)):
            for ph, t in (lst or []):
                yield "phase", t, dict(phase_hw=ph, dgrad=dg)
        for lst, dg in ((self.ws2, False), (self.ws2d, True)):
            for ab, t in (lst or []):
                yield "sel", t, self._s2_args(ab, dg)

    def _walk(self, sink, w: Tensor, bsrc: Tensor) -> None:
        """Every layout of ``layouts()`` into ``sink`` (ops.PrepTable or ops.EagerPrep), read from the source ``w`` under this object's
        geometry - which the sink checks against what ``w`` holds."""
        geo = dict(cout=self.cout, cin=self.cin, k=self.kernel)
        for kind, t, kw in self.layouts():
            if kind == "bias":
                sink.add_vec(bsrc, t, perm=self.row_src, n=(self.row_src.numel() if self.row_src is not None else bsrc.numel()))
            else:
                getattr(sink, "add_" + kind)(w, t, **kw, **geo)

    def prep_into(self, table: "ops.PrepTable") -> bool:
        """Append this conv's prepared layouts (what ``refresh`` writes) to a rho_prep_batch table; False if it cannot be batched."""
        if not self.batchable or not self.weight.is_contiguous() or not self.bias_param.is_contiguous():
            return False
        w = self._source()                      # a view of the parameter (reshape of a contiguous tensor)
        if w.data_ptr() != self.weight.data_ptr():
            return False
        self._walk(table, w, self._bias_source())
        return True

    def refresh(self) -> None:
        self._walk(ops.EagerPrep(), self._source(), self._bias_source())


class _StemAsGemm(_ConvW):
    """Stem conv with cin * taps <= 32 viewed as a 1x1x1 conv over the im2col operand (rho_im2col_taps): weight
    [cout, cin * taps] in the (ci, kd, kh, kw) order of ``weight.reshape``."""

    def _geometry(self):
        self.kernel3, self.taps3 = self.kernel, self.taps           # the parameter's own extents
        self.kernel, self.taps = (1, 1, 1), 1
        self.cin = self.weight.shape[1] * self.taps3

    def _source(self) -> Tensor:
        return self.weight.detach().reshape(self.cout, self.cin, 1, 1, 1).contiguous()

    def enable_dgrad(self) -> None:
        """A forward-only re-reading of the parameter: no data-gradient layout (the stem has no data gradient at all)."""


class _HeadAsGemm(_ConvW):
    """Head conv with cout == 1 viewed as a 1x1x1 conv cin -> taps (rows = taps, padded to 32 output channels) whose
    result rho_tap_gather_sum folds over the taps; the bias is added there."""

    def _geometry(self):
        self.kernel3, self.taps3 = self.kernel, self.taps           # the parameter's own extents
        self.kernel, self.taps = (1, 1, 1), 1
        self.cout = 32

    def _source(self) -> Tensor:
        w = self.weight.detach()[0].reshape(self.cin, self.taps3).t()          # [taps, cin]
        full = torch.zeros(32, self.cin, 1, 1, 1, dtype=w.dtype, device=w.device)
        full[: self.taps3, :, 0, 0, 0] = w
        return full

    def _bias_source(self) -> Tensor:
        return torch.zeros(32, dtype=torch.float32, device=self.weight.device)

    # its source is a transposed, zero-padded copy of the parameter, not a view: batched as a gather (RHO_PREP_VEC) through an
    # index table built once - w[0][r = tap][c] = weight[0][c][r]
    def prep_into(self, table: "ops.PrepTable") -> bool:
        if not self.weight.is_contiguous():
            return False
        if getattr(self, "_perm", None) is None:
            r = torch.arange(self.w.shape[1]).view(-1, 1)
            c = torch.arange(self.w.shape[2]).view(1, -1)
            idx = torch.where((r < self.taps3) & (c < self.cin), c * self.taps3 + r, torch.full_like(r + c, -1))
            self._perm = idx.reshape(-1).to(torch.int32).to(self.w.device)
        table.add_vec(self.weight.detach().reshape(-1), self.w, perm=self._perm, n=self.w.numel())
        return True                                  # (b stays zero: the bias is added by the kernel that folds the taps)

    def enable_dgrad(self) -> None:
        """A forward-only re-reading of the parameter ([1, C, taps] read as 32 rows x C): the generic data-gradient preparation
        would index the parameter with this geometry - 32 * C elements of a tensor that holds 27 * C (an out-of-bounds read that
        faulted once the parameter sat at the end of its allocation, round 4).  The head's data gradient has weights of its own
        (_HeadDgradW) or runs on the plain 3x3x3 form."""


class _HeadDgradW:
    """Data-gradient weights of a one-output-channel 3x3x3 head conv in the layout rho_stem_conv3d reads ([1][C][32], taps as the
    contraction): dact[pos][c] = sum_tap W[0][c][tap] dpred[pos - (tap - 1)] is that kernel run on dpred with the taps mirrored,
    w[0][c][t] = weight[0][c][26 - t]  (training plans of the bf16 engine, round 4)."""

    batchable = True

    def __init__(self, weight: nn.Parameter, dtype):
        self.weight = weight
        C_ = weight.shape[1]
        self.taps3 = int(weight[0, 0].numel())
        dev = weight.device
        self.w = torch.zeros(1, C_, 32, dtype=dtype, device=dev)
        self.zero_bias = torch.zeros(C_, dtype=torch.float32, device=dev)
        c = torch.arange(C_).view(-1, 1)
        t = torch.arange(32).view(1, -1)
        idx = torch.where(t < self.taps3, c * self.taps3 + (self.taps3 - 1 - t), torch.full_like(c + t, -1))
        self._perm = idx.reshape(-1).to(torch.int32).to(dev)
        self.refresh()

    def layout_signature(self) -> tuple:
        return (id(self), self.weight.data_ptr())

    def prep_into(self, table: "ops.PrepTable") -> bool:
        if not self.weight.is_contiguous():
            return False
        table.add_vec(self.weight.detach().reshape(-1), self.w, perm=self._perm, n=self.w.numel())
        return True

    def refresh(self) -> None:
        src = self.weight.detach().reshape(-1).float()
        g = torch.where(self._perm >= 0, src[self._perm.clamp(min=0).long()], torch.zeros((), device=src.device))   # (data movement only)
        self.w.copy_(g.view_as(self.w))
