"""Backward half of a training plan: walks the forward plan's nodes in reverse and appends the launches of the bias / weight /
data gradients and of the GroupNorm + FiLM + SiLU backward to ``plan.bwd`` (see the module docstring of unet_engine for what is
kept, recomputed and aliased).  Built once per plan by ``BackwardBuilder(plan).build()``; the launches are closures over the
builder, so what is allocated after they are created (the weight-gradient arena, the deterministic workspace) and what an
optimizer may re-home (``p.grad``) is read when they run.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional

import torch
from torch import nn

from .. import hip
from ..hip import ptr
from . import ops

Tensor = torch.Tensor

# A finalize batch closes at 32 MiB of parameters, or a sixteenth of the model where that is smaller, so that data-parallel buckets
# still become final - and their all-reduce still starts - well inside the backward
FIN_BATCH_BYTES = 32 * 2 ** 20


class _Pool:
    """Exact-size buffer pool for backward temporaries (emission order == stream order)."""

    def __init__(self, device):
        self.device = device
        self.free: Dict[tuple, List[Tensor]] = {}
        self.all: List[Tensor] = []

    def get(self, shape, dtype) -> Tensor:
        key = (int(torch.Size(shape).numel()), dtype)
        lst = self.free.get(key)
        if lst:
            return lst.pop().view(*shape)
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        self.all.append(t)
        return t

    def put(self, t: Tensor) -> None:
        self.free.setdefault((t.numel(), t.dtype), []).append(t)


def key(t: Tensor) -> int:
    return t.data_ptr()


def pgrad(p: nn.Parameter) -> int:
    return p.grad.data_ptr()       # resolved at launch time: optimizers may re-home .grad


class BackwardBuilder:
    """State of the backward construction of one ``_Plan``.  Everything runs on ONE stream: weight gradients on a side stream
    beside the HBM-bound GroupNorm backward passes were measured slower and removed."""

    def __init__(self, plan):
        self.plan = plan
        self.eng = eng = plan.eng
        self.sw = plan.sw
        self.L = plan.L
        self.dt = eng.dtype
        self.dtc = hip.dtype_code(eng.dtype)
        self.dev = eng.device
        self.esz = 2 if eng.dtype == torch.bfloat16 else 4
        self.pool = _Pool(self.dev)
        self.G: Dict[int, Tensor] = {}        # activation data_ptr -> gradient buffer
        self.written = set()
        # Residual adds folded into the next GroupNorm-backward apply pass: `G[res] += dY` of a residual connection whose target
        # already holds a gradient is NOT launched; the addend waits here until the apply pass that accumulates into G[res] anyway
        # takes it as `add1` (one read instead of read + read + write).  Any other access to G[res] flushes it as the plain
        # rho_add_inplace first.
        self.pending_add: Dict[int, Tensor] = {}
        self.skip_partner: Dict[int, int] = {}          # id(1x1x1 skip node) -> id(the block's in-conv node), see fuse_skip_dgrad
        self.held_skips: Dict[int, tuple] = {}          # id(in-conv node) -> (skip node, dY, width) waiting for its GroupNorm backward
        self.film_stride = plan.film.shape[1]
        # Deterministic training (rho_set_deterministic / RHO_DETERMINISTIC=1): the weight gradient flushes through ordered slabs
        # (rho_conv_nd_wgrad_ws) instead of fp32 atomics; one workspace per plan, sized for its largest launch after all are known
        self.deterministic = ops.deterministic()
        self.det_ws: Optional[Tensor] = None
        self.det_ws_bytes = 0
        # ---- weight-gradient accumulation ARENA: every weight-gradient launch accumulates into a region of its own
        # ([taps][coutp][cinp] fp32 + the channel sums), the whole arena is cleared by ONE memset at the head of the backward, and the
        # regions are moved into the parameter gradients by ONE table-driven launch per finalize batch (rho_wgrad_finalize_batch) -
        # instead of a memset + finalize + bias-gradient launch per convolution (~250 launches of a few microseconds each per step).
        # Parameters are reported final (bwd_marks) after their batch.
        self.arena: Optional[Tensor] = None             # allocated once every region is known
        self.arena_floats = 0
        self.fin_batch_bytes = min(FIN_BATCH_BYTES, max(1, sum(4 * cw.weight.numel() for cw in eng._convs) // 16))
        self.fin_entries: List[dict] = []               # the pending finalize batch
        self.fin_params: List[nn.Parameter] = []
        self.fin_bytes = 0

    # ------------------------------------------------------------------ bookkeeping
    def emit(self, fn, kind, flops=0.0, nbytes=0.0, **shape):
        self.plan.bwd.append(fn)
        self.plan.bwd_info.append(dict(kind=kind, flops=flops, bytes=nbytes, **shape))

    def mark(self, params: List[nn.Parameter]) -> None:
        """After the launches emitted so far these parameters' gradients are final."""
        self.plan.bwd_marks.append((len(self.plan.bwd), params))

    def flush_add(self, k: int):
        src = self.pending_add.pop(k, None)
        if src is not None:
            L = self.L
            a = (ptr(self.G[k]), ptr(src), self.dtc, src.numel())
            self.emit(lambda s, a=a: L.rho_add_inplace(*a, s), "add", nbytes=3.0 * self.esz * src.numel())
            if src.data_ptr() not in {g_.data_ptr() for g_ in self.G.values()}:
                self.pool.put(src)

    def gradbuf(self, t: Tensor, fold_ok: bool = False):
        """(buffer, accumulate?) for a write into the gradient of activation t."""
        k = key(t)
        if not fold_ok:
            self.flush_add(k)
        if k in self.G:
            return self.G[k], (k in self.written)
        self.G[k] = self.pool.get(tuple(t.shape), t.dtype)
        return self.G[k], False

    def take_grad(self, t: Tensor, what: str) -> Tensor:
        """The finished gradient of activation t, removed from G."""
        self.flush_add(key(t))
        g = self.G.pop(key(t), None)
        if g is None:
            raise hip.RhoHipError(f"internal: missing gradient of {what} in the backward plan")
        return g

    # ------------------------------------------------------------------ weight-gradient arena
    def region(self, nfloats: int) -> int:
        off = self.arena_floats
        self.arena_floats = off + ((int(nfloats) + 63) // 64) * 64
        return off

    def aptr(self, off: int) -> Callable[[], int]:
        return lambda: self.arena.data_ptr() + 4 * off

    def fin_add(self, **e):
        self.fin_entries.append(e)

    def fin_params_add(self, cw) -> None:
        """The conv's weight and bias become final with the pending batch."""
        self.fin_params += [cw.weight, cw.bias_param]
        self.fin_bytes += 4 * cw.weight.numel()

    def fin_close(self, force: bool = False):
        """Emit the batched finalize of the pending regions (and report their parameters final) once enough bytes are pending."""
        if not self.fin_entries or (not force and self.fin_bytes < self.fin_batch_bytes):
            return
        entries, params = self.fin_entries, self.fin_params
        self.fin_entries, self.fin_params, self.fin_bytes = [], [], 0
        table = ops.WfinTable(self.dev)
        for e in entries:
            table.add(**e)
        state = {"sig": None}

        def run(s):
            # (pointers resolved at launch time: the arena is allocated after the plan is built, optimizers may re-home .grad)
            sig = (self.arena.data_ptr(),) + tuple(pgrad(e["param"]) for e in entries)
            if sig != state["sig"]:
                table.build(sig[0], sig[1:])
                state["sig"] = sig
            return table.launch(s)
        self.emit(run, "wgrad_finalize", nbytes=12.0 * sum(e["cout"] * e["cin"] * e["k"][0] * e["k"][1] * e["k"][2] for e in entries))
        self.plan.keep.append(table)
        self.mark(params)

    def wgrad_call(self, d, dy_ptr: int, w_: int, dw_ptr: Callable[[], int], db_ptr: Callable[[], int]):
        L = self.L
        if not self.deterministic:
            return lambda s: L.rho_conv_nd_wgrad(C.byref(d), dy_ptr, w_, dw_ptr(), db_ptr(), s)
        self.det_ws_bytes = max(self.det_ws_bytes, int(L.rho_conv_wgrad_workspace_bytes(C.byref(d), w_)))
        return lambda s: L.rho_conv_nd_wgrad_ws(C.byref(d), dy_ptr, w_, dw_ptr(), db_ptr(), ptr(self.det_ws), self.det_ws_bytes, s)

    # ------------------------------------------------------------------ per-conv gradients
    def bias_and_wgrad(self, node, dY: Tensor, dyw: int):
        plan, pool, L, esz, dtc = self.plan, self.pool, self.L, self.esz, self.dtc
        cw = node["cw"]
        N, Do, Ho, Wo = node["out_dims"]
        S = Do * Ho * Wo
        nblk = ops.gn_nblk(S)
        part = pool.get((N * nblk * (dyw // 8) * 16,), torch.float32)
        rs = ptr(cw.row_src)
        # bias gradient = channel sums of dY: accumulated by the weight-gradient kernel itself (below)
        if node["res_add_off"] is not None:        # additive timestep embedding (unet_v2.py:291)
            dst = plan.dfilm.data_ptr() + 4 * node["res_add_off"]
            a = (ptr(dY), dtc, N, S, dyw, ptr(part), dst, self.film_stride, 0, None, 0)
            self.emit(lambda s, a=a: L.rho_chan_sum(*a, s), "chan_sum", nbytes=float(esz) * N * S * dyw)
        pool.put(part)
        if node.get("phased") and node["pre"] is None and node["x2"] is None and self.sw.phase_upsample_bwd:
            # Upsample + conv ran as sub-pixel phases: per phase a 2-tap weight gradient on the SOURCE tensor against that parity
            # of dY (12 / 27 of the multiply-adds, no upsampled copy), routed back to the 3-tap parameter gradient
            x1 = node["x1"]
            nwp = max(kk[0] * kk[1] * kk[2] for kk in [cw.phase_kernel(ph_) for ph_, _ in cw.wph]) * cw.coutp * cw.cinp
            stride_ = ((nwp + 63) // 64) * 64
            off_b, off0 = self.region(max(dyw, cw.coutp)), self.region(stride_ * len(cw.wph))
            for idx, (ph, wt) in enumerate(cw.wph):
                d = ops.make_conv_desc(x1, None, wt, cw.b, kernel=cw.phase_kernel(ph), cout=cw.cout, split=cw.cout, y=dY, y2=None,
                                       phase_hw=ph)
                plan.keep.append(d)
                plan.wgrad_descs.append((d, dyw))
                self.emit(self.wgrad_call(d, ptr(dY), dyw, self.aptr(off0 + idx * stride_), self.aptr(off_b)), "wgrad",
                          flops=2.0 * N * S * cw.cout * cw.cin * cw.taps / len(cw.wph),
                          nbytes=float(esz) * (x1.numel() + dY.numel() / len(cw.wph)),
                          cin=cw.cin, cout=cw.cout, taps=cw.taps, positions=N * S // len(cw.wph))
            up_h_, up_w_ = int(any(ph[0] for ph, _ in cw.wph)), int(any(ph[1] for ph, _ in cw.wph))
            self.fin_add(kind=1, off=off0, param=cw.weight, rs=None, cout=cw.cout, cin=cw.cin, coutp=cw.coutp, cinb=cw.cinp,
                         k=cw.kernel, up_h=up_h_, up_w=up_w_, stride=stride_)
            self.fin_add(kind=0, off=off_b, param=cw.bias_param, rs=rs, cout=cw.cout, cin=1, coutp=dyw, cinb=1, k=(1, 1, 1))
            self.fin_params_add(cw)
            return
        # weight gradient (forward descriptor; upsampled input materialised)
        x1 = node["x1"]
        tmp_up = None
        if node["up_hw"] != (0, 0):
            uh, uw = node["up_hw"]
            tmp_up = pool.get((x1.shape[0], x1.shape[1], x1.shape[2] * (2 if uh else 1), x1.shape[3] * (2 if uw else 1),
                               x1.shape[4]), self.dt)
            a = (ptr(x1), ptr(tmp_up), dtc, x1.shape[0] * x1.shape[1], x1.shape[2], x1.shape[3], x1.shape[4], int(uh), int(uw))
            self.emit(lambda s, a=a: L.rho_upsample2x(*a, s), "upsample", nbytes=5.0 * esz * x1.numel())
            x1 = tmp_up
        pre = node["pre"]
        x2 = node["x2"]
        xact = None
        if node.get("xact") is not None:
            x1, x2 = node["xact"], None              # materialised by the forward plan
        elif pre is not None:
            # materialise act(a*x+b) once (HBM-rate) instead of redoing it in every (cout tile, cin chunk) workgroup
            # (dropout: the same mask as the forward - same key, same counter)
            xact = pool.get(tuple(x1.shape[:4]) + (x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0),), self.dt)
            self.emit(ops.gn_apply_launch(x1, x2, pre, node["pre_silu"], xact, node.get("drop"), plan.drop_ctr), "gn_apply",
                      nbytes=2.0 * esz * xact.numel())
            x1, x2 = xact, None
        d = ops.make_conv_desc(x1, x2, cw.w, cw.b, kernel=cw.kernel, cout=cw.cout, split=cw.cout, y=dY, y2=None,
                               stride_hw=node["stride_hw"], pre_silu=False)
        plan.keep.append(d)
        plan.wgrad_descs.append((d, dyw))
        off_w, off_b = self.region(cw.taps * cw.coutp * cw.cinp), self.region(max(dyw, cw.coutp))
        self.emit(self.wgrad_call(d, ptr(dY), dyw, self.aptr(off_w), self.aptr(off_b)), "wgrad",
                  flops=2.0 * N * S * cw.cout * cw.cin * cw.taps, nbytes=float(esz) * (x1.numel() + dY.numel()),
                  cin=cw.cin, cout=cw.cout, taps=cw.taps, positions=N * S)
        self.fin_add(kind=0, off=off_w, param=cw.weight, rs=rs, cout=cw.cout, cin=cw.cin, coutp=cw.coutp, cinb=cw.cinp, k=cw.kernel)
        self.fin_add(kind=0, off=off_b, param=cw.bias_param, rs=rs, cout=cw.cout, cin=1, coutp=dyw, cinb=1, k=(1, 1, 1))
        self.fin_params_add(cw)
        if tmp_up is not None:
            pool.put(tmp_up)
        if xact is not None:
            pool.put(xact)

    def gn_backward(self, pre, pre_silu, x1, x2, dact, fused=None, drop=None, skip=None):
        """dact = gradient of act(GroupNorm(x) * (1 + scale) + shift): reduce / finalize / apply into the gradients of x1 (, x2),
        the norm's parameters and the FiLM rows.  ``fused`` = (tile sums, tiles per sample) when the dgrad launch that produced
        dact already reduced dz and dz * x in its epilogue (rho_conv_desc.gnb_*): the reduce pass is skipped.  ``skip`` = (node,
        dY, width) of the block's 1x1x1 skip convolution whose data gradient was held back: it runs here, with the apply pass in
        its epilogue (rho_conv_desc.gna_*), or - where that launch does not exist - on its own in front of the apply pass."""
        plan, pool, L, esz, dtc, G, written = self.plan, self.pool, self.L, self.esz, self.dtc, self.G, self.written
        film_stride = self.film_stride
        c1 = x1.shape[-1]
        c2 = x2.shape[-1] if x2 is not None else 0
        norm = pre["norm"]
        Cc, N_, S_ = pre["C"], pre["N"], pre["S"]
        skip_fused = None
        if skip is not None:
            sk_node, sk_dY, sk_w = skip
            can = (drop is None and int(pre_silu) <= 1 and key(x1) not in written and key(x1) not in self.pending_add
                   and (x2 is None or key(x2) not in written) and S_ % 256 == 0 and Cc % 32 == 0
                   and (x2 is None or c2 % (8 if self.dt == torch.bfloat16 else 4) == 0))
            if can:
                skip_fused = skip
            else:
                self.dgrad(sk_node, sk_dY, sk_w, hold_skip=False)          # the two-pass form: data gradient first, apply accumulates
                pool.put(sk_dY)
        g1, acc1 = self.gradbuf(x1, fold_ok=True)
        add1 = self.pending_add.pop(key(x1), None)         # a residual's gradient waiting to join G[x1]: folded into this pass
        g2, acc2 = self.gradbuf(x2) if x2 is not None else (None, False)
        cA = pool.get((N_, Cc), torch.float32)
        cP = pool.get((N_, 32), torch.float32)
        cQ = pool.get((N_, 32), torch.float32)
        work = pool.get((2 * N_ * Cc,), torch.float32)
        dargs = () if drop is None else (float(drop[0]), int(drop[1]), ptr(plan.drop_ctr))     # (Philox mask: p, key, counter)
        scale = dscale = dshift = None
        fstride = 0
        if pre["film_off"] is not None:
            scale = plan.film.data_ptr() + 4 * pre["film_off"]
            fstride = film_stride
            dscale = plan.dfilm.data_ptr() + 4 * pre["film_off"]
            dshift = plan.dfilm.data_ptr() + 4 * (pre["film_off"] + Cc)
        if fused is None:
            a1 = (ptr(dact), ptr(x1), c1, ptr(x2), c2, dtc, N_, S_, ptr(pre["a"]), ptr(pre["b"]), ptr(pre["st"]),
                  int(pre_silu), ptr(pre["part"]))
            reduce = L.rho_gn_bwd_reduce if drop is None else L.rho_gn_bwd_reduce_drop
            self.emit(lambda s, a=a1 + dargs: reduce(*a, s), "gn_bwd_reduce", nbytes=2.0 * esz * N_ * S_ * Cc)
            part_ptr, part_n, fmt = ptr(pre["part"]), pre["nblk"], 0
        else:
            part_ptr, part_n, fmt = ptr(fused[0]), fused[1], 1
        self.emit(lambda s: L.rho_gn_bwd_finalize(
            part_ptr, N_, Cc, S_, part_n, fmt, ptr(norm.weight), ptr(norm.bias), scale, fstride, ptr(pre["st"]),
            ptr(work), pgrad(norm.weight), pgrad(norm.bias), 1, dscale, dshift, film_stride, ptr(cA), ptr(cP),
            ptr(cQ), s), "gn_bwd_finalize")
        a3 = (ptr(dact), ptr(x1), c1, ptr(x2), c2, dtc, N_, S_, ptr(pre["a"]), ptr(pre["b"]), int(pre_silu),
              ptr(cA), ptr(cP), ptr(cQ), ptr(g1), ptr(g2), int(acc1), int(acc2), ptr(add1))
        nb3 = esz * N_ * S_ * (3.0 * Cc + (c1 if acc1 else 0) + (c2 if acc2 else 0) + (c1 if add1 is not None else 0))
        if skip_fused is not None:
            # dX = skip^T(dY) + [cA * (dact * act'(a x + b)) + cQ * x + cP] in the 1x1x1 data-gradient launch's epilogue
            sk_node, sk_dY, sk_w = skip_fused
            scw = sk_node["cw"]
            if acc1 or acc2 or add1 is not None:
                raise hip.RhoHipError("internal: fused skip data gradient on a gradient that already has a writer (backward plan)")
            d = ops.make_conv_desc(sk_dY, None, scw.wd, scw.zero_bias, kernel=scw.kernel, cout=Cc, split=c1, y=g1, y2=g2,
                                   y2_cl=x2 is not None)
            d.gnb_x1, d.gnb_x2, d.gnb_c1, d.gnb_silu = ptr(x1), ptr(x2), c1, int(pre_silu)
            d.gnb_a, d.gnb_b = ptr(pre["a"]), ptr(pre["b"])
            d.gna_g, d.gna_cA, d.gna_cP, d.gna_cQ = ptr(dact), ptr(cA), ptr(cP), ptr(cQ)
            self.conv_launch(d, flops=2.0 * N_ * S_ * Cc * scw.cout, nbytes=float(esz) * (sk_dY.numel() + 3.0 * N_ * S_ * Cc))
            pool.put(sk_dY)
        else:
            apply = L.rho_gn_bwd_apply if drop is None else L.rho_gn_bwd_apply_drop
            self.emit(lambda s, a=a3 + dargs: apply(*a, s), "gn_bwd_apply", nbytes=nb3)
        if add1 is not None and add1.data_ptr() not in {g_.data_ptr() for g_ in G.values()}:
            pool.put(add1)                                 # (stream order: recycled buffers are written by later launches only)
        written.add(key(x1))
        if x2 is not None:
            written.add(key(x2))
        for t in (cA, cP, cQ, work):
            pool.put(t)

    def conv_launch(self, d, flops: float, nbytes: float) -> None:
        """Emit one data-gradient launch: the forward kernel on dY with the descriptor's flipped / transposed weights."""
        L = self.L
        self.plan.keep.append(d)
        self.plan.fwd_descs.append(d)
        self.emit(lambda s: L.rho_conv_nd_fwd(C.byref(d), s), "dgrad", flops=flops, nbytes=nbytes)

    def dgrad(self, node, dY: Tensor, dyw: int, hold_skip: bool = True):
        """Data gradient of a conv node.  Returns True when the launch was held back: the 1x1x1 skip convolution of a ResBlock
        whose in-conv path ends in a GroupNorm backward of the same inputs - it runs inside that pass (gn_backward's ``skip``)."""
        plan, pool, L, esz, dtc, written = self.plan, self.pool, self.L, self.esz, self.dtc, self.written
        cw = node["cw"]
        if hold_skip and id(node) in self.skip_partner:
            self.held_skips[self.skip_partner[id(node)]] = (node, dY, dyw)
            return True
        x1, x2, pre = node["x1"], node["x2"], node["pre"]
        c1 = x1.shape[-1]
        c2 = x2.shape[-1] if x2 is not None else 0
        cin = c1 + c2
        if dyw != cw.wd.shape[2] or cw.wd.shape[1] != cin:
            raise hip.RhoHipError("internal: dgrad weight shape does not match the gradient tensors")
        common = dict(kernel=cw.kernel, cout=cin)
        if node.get("phased") and pre is None and x2 is None and self.sw.phase_upsample_bwd:
            # Upsample + conv ran as sub-pixel phases: each phase's share of dX is a 2-tap conv of that parity of dY with the
            # phase's flipped weights, accumulated in place - 12 / 27 of the multiply-adds, no full-resolution intermediate
            g1, acc1 = self.gradbuf(x1)
            for i, (ph, wt) in enumerate(cw.wphd):
                d = ops.make_conv_desc(dY, None, wt, cw.zero_bias, kernel=cw.phase_kernel(ph), cout=cin, split=cin, y=g1, y2=None,
                                       res=g1 if (acc1 or i > 0) else None, phase_dgrad_hw=ph)
                self.conv_launch(d, flops=2.0 * (dY.numel() // dyw) * cin * cw.cout * cw.taps / len(cw.wphd),
                                 nbytes=float(esz) * (dY.numel() / len(cw.wphd) + x1.numel() * (2 if (acc1 or i > 0) else 1)))
            written.add(key(x1))
        elif pre is not None or node["up_hw"] != (0, 0):
            N, Do, Ho, Wo = node["out_dims"]
            tshape = (N, Do, Ho, Wo, cin) if node["up_hw"] != (0, 0) else tuple(x1.shape[:4]) + (cin,)
            dact = pool.get(tshape, self.dt)       # gradient of the activated / upsampled tensor
            d = ops.make_conv_desc(dY, None, cw.wd, cw.zero_bias, split=cin, y=dact, y2=None, **common)
            fused = None
            if (pre is not None and self.sw.fuse_gn_bwd > 0 and cin >= self.sw.fuse_gn_bwd and int(node["pre_silu"]) <= 1
                    and node.get("drop") is None):
                # the norm's backward reductions ride in this launch's epilogue where a tile lies in one sample
                tiles = int(L.rho_conv_stats_tiles(C.byref(d)))
                if tiles > 0:
                    sbuf = pool.get((x1.shape[0] * tiles * 2 * cin,), torch.float32)
                    d.stats = sbuf.data_ptr()
                    d.gnb_x1, d.gnb_x2, d.gnb_c1 = ptr(x1), ptr(x2), c1
                    d.gnb_a, d.gnb_b, d.gnb_silu = ptr(pre["a"]), ptr(pre["b"]), int(node["pre_silu"])
                    fused = (sbuf, tiles)
            self.conv_launch(d, flops=2.0 * (dact.numel() // cin) * cin * cw.cout * cw.taps,
                             nbytes=float(esz) * (dY.numel() + dact.numel()))
            if pre is not None:
                self.gn_backward(pre, node["pre_silu"], x1, x2, dact, fused, drop=node.get("drop"),
                                 skip=self.held_skips.pop(id(node), None))
                if fused is not None:
                    pool.put(fused[0])
            else:   # upsample: sum the 2x2 (1x2) children
                g1, acc1 = self.gradbuf(x1)
                a = (ptr(dact), ptr(g1), dtc, x1.shape[0] * x1.shape[1], x1.shape[2], x1.shape[3], x1.shape[4],
                     int(node["up_hw"][0]), int(node["up_hw"][1]), int(acc1))
                self.emit(lambda s, a=a: L.rho_pool2x_sum(*a, s), "pool2x", nbytes=5.0 * esz * x1.numel())
                written.add(key(x1))
            pool.put(dact)
        elif node.get("s2") and self.sw.s2_split_bwd:
            # stride-2 conv: one launch per parity of dX (dx[2m] = w1 dy[m]; dx[2m+1] = w2 dy[m] + w0 dy[m+1]) instead of a 27-tap
            # conv over a zero-stuffed dY (three of four multiply-adds on zeros)
            g1, acc1 = self.gradbuf(x1)
            for (a, b), wt in cw.ws2d:
                kern = (3, len(cw.S2_BWD[a]), len(cw.S2_BWD[b]))
                d = ops.make_conv_desc(dY, None, wt, cw.zero_bias, kernel=kern, cout=cin, split=cin, y=g1, y2=None,
                                       res=g1 if acc1 else None, phase_hw=(a + 1, b + 1))
                self.conv_launch(d, flops=2.0 * (dY.numel() // dyw) * cin * cw.cout * kern[0] * kern[1] * kern[2],
                                 nbytes=float(esz) * (dY.numel() + x1.numel() / 4 * (2 if acc1 else 1)))
            written.add(key(x1))
        else:
            g1, acc1 = self.gradbuf(x1)
            g2, acc2 = self.gradbuf(x2) if x2 is not None else (None, False)
            st = node["stride_hw"]
            zs = (int(st[0] == 2), int(st[1] == 2))
            d = ops.make_conv_desc(dY, None, cw.wd, cw.zero_bias, split=c1, y=g1, y2=g2, y2_cl=x2 is not None,
                                   res=g1 if acc1 else None, res2=g2 if (x2 is not None and acc2) else None,
                                   zs_hw=zs, out_hw=(x1.shape[2], x1.shape[3]) if zs != (0, 0) else (0, 0), **common)
            self.conv_launch(d, flops=2.0 * (x1.numel() // c1) * cin * cw.cout * cw.taps,
                             nbytes=float(esz) * (dY.numel() + x1.numel()))
            written.add(key(x1))
            if x2 is not None:
                written.add(key(x2))
        return False

    # ------------------------------------------------------------------ GEMM forms of the one-channel ends
    def im2col_of(self, src_f32: Tensor, dims4):
        """[N, 1, D, H, W] float32 -> channels-last [N, D, H, W, 32] (27 taps + zero pad), the K = 32 operand of the GEMM forms."""
        L = self.L
        N_, D_, H_, W_ = dims4
        im = self.pool.get((N_, D_, H_, W_, 32), self.dt)
        a_ = (ptr(src_f32), ptr(im), self.dtc, N_, 1, D_, H_, W_, 3, 3, 3, 32)
        self.emit(lambda s, a=a_: L.rho_im2col_taps(*a, s), "pack", nbytes=4.0 * src_f32.numel() + float(self.esz) * im.numel())
        return im

    def gemm_wgrad(self, x_t: Tensor, dy_t: Tensor, rows: int):
        """dw[rows][cin] (+ channel sums of dy_t) = sum_pos dy_t[pos][:rows] x_t[pos][:] on the GEMM-shaped k_wgrad1; returns the
        arena offsets (weights, channel sums)."""
        plan = self.plan
        cin_ = x_t.shape[-1]
        dummy_w = torch.empty(1, rows, cin_, dtype=self.dt, device=self.dev)
        dummy_b = torch.zeros(rows, dtype=torch.float32, device=self.dev)
        plan.keep.extend([dummy_w, dummy_b])
        d = ops.make_conv_desc(x_t, None, dummy_w, dummy_b, kernel=(1, 1, 1), cout=rows, split=rows, y=dy_t, y2=None)
        plan.keep.append(d)
        plan.wgrad_descs.append((d, dy_t.shape[-1]))
        off_w, off_b = self.region(rows * cin_), self.region(max(rows, dy_t.shape[-1]))
        npos_ = x_t.numel() // cin_
        self.emit(self.wgrad_call(d, ptr(dy_t), dy_t.shape[-1], self.aptr(off_w), self.aptr(off_b)), "wgrad",
                  flops=2.0 * npos_ * 27 * max(rows, cin_), nbytes=float(self.esz) * (x_t.numel() + dy_t.numel()),
                  cin=cin_, cout=rows, taps=1, positions=npos_)
        return off_w, off_b

    # ------------------------------------------------------------------ node kinds
    def head_direct(self, head):
        """One-output-channel head conv (unet_v2.py:679-683): data gradient = rho_stem_conv3d on dpred with mirrored taps; weight
        gradient = GEMM of the kept activated input against the im2col of dpred (rows = taps, mirrored back by finalize kind 2);
        bias gradient = the im2col's centre column sum (tap 13 never touches the padding) = sum of dpred."""
        plan, pool, L = self.plan, self.pool, self.L
        hcw = head["cw"]
        N, Do, Ho, Wo = head["out_dims"]
        Ch = head["x"].shape[-1]
        hdw = self.eng._head_dgrad(self.eng.model.out[2])
        dact = pool.get((N, Do, Ho, Wo, Ch), self.dt)
        a = (ptr(plan.dpred_in), ptr(hdw.w), ptr(hdw.zero_bias), ptr(dact), None, N, Do, Ho, Wo, Ch)
        self.emit(lambda s, a=a: L.rho_stem_conv3d(*a, s), "dgrad", flops=2.0 * N * Do * Ho * Wo * Ch * 27,
                  nbytes=4.0 * N * Do * Ho * Wo + float(self.esz) * dact.numel())
        im = self.im2col_of(plan.dpred_in, (N, Do, Ho, Wo))
        off_w, off_b = self.gemm_wgrad(head["xact"], im, 32)
        pool.put(im)
        self.fin_add(kind=2, off=off_w, param=hcw.weight, rs=None, cout=1, cin=Ch, coutp=32, cinb=Ch, k=(3, 3, 3))   # (walks [ci][tap])
        self.fin_add(kind=0, off=off_b + 13, param=hcw.bias_param, rs=None, cout=1, cin=1, coutp=1, cinb=1, k=(1, 1, 1))
        self.fin_params_add(hcw)
        self.gn_backward(head["pre"], self.eng.act, head["x"], None, dact)
        pool.put(dact)
        self.mark([head["pre"]["norm"].weight, head["pre"]["norm"].bias])

    def head_packed(self, head):
        """dpred [N, Cout, S] float32 -> channels-last, as wide as the dgrad weights expect: the dY of the head's conv node."""
        L = self.L
        hw = head["cw"].wd.shape[2]
        N, Do, Ho, Wo = head["out_dims"]
        dhead = self.pool.get((N, Do, Ho, Wo, hw), self.dt)
        a = (ptr(self.plan.dpred_in), ptr(dhead), self.dtc, N, head["cw"].cout, Do * Ho * Wo, hw)
        self.emit(lambda s, a=a: L.rho_pack_input(*a, s), "pack")
        self.G[key(head["y2"])] = dhead
        self.written.add(key(head["y2"]))

    def stem_direct(self, node):
        """One-input-channel stem conv (unet_v2.py:535): weight gradient = GEMM of the im2col of the input against dY
        (dw[co][tap], the parameter's own layout), bias gradient = channel sums of dY; no data gradient."""
        dY = self.take_grad(node["y"], "the stem output")
        scw = node["cw"]
        im = self.im2col_of(self.plan.x_in, node["out_dims"])
        off_w, off_b = self.gemm_wgrad(im, dY, scw.cout)
        self.pool.put(im)
        self.pool.put(dY)
        self.fin_add(kind=0, off=off_w, param=scw.weight, rs=None, cout=scw.cout, cin=27, coutp=scw.cout, cinb=32, k=(1, 1, 1))
        self.fin_add(kind=0, off=off_b, param=scw.bias_param, rs=None, cout=scw.cout, cin=1, coutp=dY.shape[-1], cinb=1, k=(1, 1, 1))
        self.fin_params_add(scw)
        self.fin_close()

    def resample(self, node):
        """y = avgpool / nearest-upsample(x): the transposed map into the gradient of x (accumulating if x has other consumers)."""
        L, esz = self.L, self.esz
        dy = self.take_grad(node["y"], "a resampled tensor")
        xt = node["x"]
        gx, accx = self.gradbuf(xt)
        rs_hw = (1, 1) if self.eng.dims >= 2 else (0, 1)
        a = (ptr(dy), ptr(gx), self.dtc, xt.shape[0] * xt.shape[1], xt.shape[2], xt.shape[3], xt.shape[4], rs_hw[0], rs_hw[1], int(accx))
        if node["mode"] == "up":
            self.emit(lambda s, a=a: L.rho_pool2x_sum(*a, s), "pool2x", nbytes=5.0 * esz * xt.numel())
        else:
            self.emit(lambda s, a=a: L.rho_avgpool2x_bwd(*a, s), "avgpool_bwd", nbytes=3.0 * esz * xt.numel())
        self.written.add(key(xt))
        self.pool.put(dy)

    def act(self, node):
        dact = self.take_grad(node["y"], "a materialised activation")
        self.gn_backward(node["pre"], node["pre_silu"], node["x1"], node["x2"], dact)
        self.pool.put(dact)
        self.mark([node["pre"]["norm"].weight, node["pre"]["norm"].bias])

    def attn(self, node):
        pool, L, G = self.pool, self.L, self.G
        self.flush_add(key(node["ao"]))
        dao = G.get(key(node["ao"]))
        N, T, Cc = node["N"], node["T"], node["C"]
        dqkv = pool.get(tuple(node["qk"].shape[:4]) + (3 * Cc,), self.dt)   # = dY of the qkv projection
        delta = pool.get((N, node["heads"], T), torch.float32)
        a = (ptr(node["qk"]), ptr(node["vt"]), ptr(node["ao"]), ptr(dao), ptr(node["lse"]), ptr(delta), dqkv.data_ptr(), 3 * Cc,
             dqkv.data_ptr() + 2 * Cc * self.esz, 3 * Cc, self.dtc, N, T, node["heads"], Cc // node["heads"])
        self.emit(lambda s, a=a: L.rho_attention_bwd(*a, s), "attention_bwd", flops=14.0 * N * T * T * Cc)
        G[key(node["qk"])] = dqkv
        self.written.add(key(node["qk"]))
        pool.put(delta)
        pool.put(G.pop(key(node["ao"])))

    def conv(self, node):
        L, G = self.L, self.G
        out_t = node["y"] if node["y"] is not None else node["y2"]
        self.flush_add(key(out_t))
        dY = G.get(key(out_t))
        if dY is None:
            raise hip.RhoHipError("internal: missing output gradient in backward plan")
        dyw = dY.shape[-1]
        held_for_add = False
        # residual input of the epilogue: alias (first contribution) or accumulate
        if node["res"] is not None:
            rk = key(node["res"])
            if rk not in G:
                G[rk] = dY
                self.written.add(rk)
            elif rk not in self.pending_add and G[rk].shape == dY.shape:
                self.pending_add[rk] = dY                  # joins G[rk] in the next apply pass that accumulates into it
                held_for_add = True
            else:
                self.flush_add(rk)
                a = (ptr(G[rk]), ptr(dY), self.dtc, dY.numel())
                self.emit(lambda s, a=a: L.rho_add_inplace(*a, s), "add", nbytes=3.0 * self.esz * dY.numel())
        self.bias_and_wgrad(node, dY, dyw)
        held_skip = False
        if not node["stem"]:
            held_skip = self.dgrad(node, dY, dyw)
        # the output gradient is dead now unless a residual aliased it
        aliased = node["res"] is not None and G.get(key(node["res"])) is dY
        G.pop(key(out_t), None)
        if not aliased and not held_for_add and not held_skip:
            self.pool.put(dY)
        if node["pre"] is not None:          # (the conv's own parameters are reported with their finalize batch)
            self.mark([node["pre"]["norm"].weight, node["pre"]["norm"].bias])
        self.fin_close()

    def embedding(self):
        """Embedding path (needs the FiLM gradients of every block): the batched FiLM projections, then time_embed."""
        plan, eng, L = self.plan, self.eng, self.L
        B, film_stride = plan.B, self.film_stride
        e = 4 * eng.mc
        first = True
        emb_params: List[nn.Parameter] = []
        for blk in eng._film_blocks:
            lin = blk.emb_layers[1]
            off = eng._film_off[id(blk)]
            O = lin.weight.shape[0]
            dptr = plan.dfilm.data_ptr() + 4 * off
            self.emit(lambda s, lin=lin, dptr=dptr, O=O, first=first: L.rho_linear_bwd(
                dptr, film_stride, ptr(plan.emb), ptr(lin.weight), pgrad(lin.weight), pgrad(lin.bias), ptr(plan.demb), B, e, O, eng.act, 1,
                0 if first else 1, s), "linear_bwd", flops=4.0 * B * e * O)
            first = False
            emb_params += [lin.weight, lin.bias]
        te0, te2 = eng.model.time_embed[0], eng.model.time_embed[2]
        self.emit(lambda s: L.rho_linear_bwd(ptr(plan.demb), 0, ptr(plan.emb_h), ptr(te2.weight), pgrad(te2.weight), pgrad(te2.bias),
                                             ptr(plan.demb_h), B, e, e, eng.act, 1, 0, s), "linear_bwd")
        self.emit(lambda s: L.rho_linear_bwd(ptr(plan.demb_h), 0, ptr(plan.sin_in), ptr(te0.weight), pgrad(te0.weight), pgrad(te0.bias),
                                             None, B, eng.mc, e, 0, 1, 0, s), "linear_bwd")
        emb_params += [te2.weight, te2.bias, te0.weight, te0.bias]
        self.mark(emb_params)

    def pair_skips(self) -> None:
        """1x1x1 skip-conv nodes whose block input also feeds a normalised conv (the block's in-conv, an earlier node): id(skip
        node) -> id(in-conv node).  Their data gradient is held until that node's GroupNorm backward (fuse_skip_dgrad)."""
        nodes = self.plan.nodes
        for i, nd in enumerate(nodes):
            if (nd["k"] == "conv" and nd["cw"].taps == 1 and nd["pre"] is None and not nd["stem"] and nd["up_hw"] == (0, 0)
                    and tuple(nd["stride_hw"]) == (1, 1) and nd["res"] is None and not nd.get("phased") and not nd.get("s2")):
                for pj in range(i - 1, -1, -1):
                    pn = nodes[pj]
                    if (pn["k"] == "conv" and pn["pre"] is not None and pn["x1"] is nd["x1"] and pn["x2"] is nd["x2"]
                            and pn["up_hw"] == (0, 0) and not pn["stem"]):
                        self.skip_partner[id(nd)] = id(pn)
                        break

    # ------------------------------------------------------------------ the plan
    def build(self) -> None:
        plan, eng, dev, pool = self.plan, self.eng, self.dev, self.pool
        plan.keep.append(pool)
        for cw in eng._convs:
            cw.enable_dgrad()
        B = plan.B
        plan.dfilm = torch.empty(B, max(eng.film_total, 1), dtype=torch.float32, device=dev)
        plan.demb = torch.empty(B, 4 * eng.mc, dtype=torch.float32, device=dev)
        plan.demb_h = torch.empty(B, 4 * eng.mc, dtype=torch.float32, device=dev)
        plan.deterministic = self.deterministic
        plan.dpred_in = torch.empty(tuple(plan.out.shape), dtype=torch.float32, device=dev)
        self.emit(lambda s: (self.arena.zero_(), 0)[1], "memset")
        arena_memset_info = plan.bwd_info[-1]
        head = plan.nodes[-1]
        if head["k"] == "head_direct":
            self.head_direct(head)
        else:
            self.head_packed(head)
        if self.sw.fuse_skip_dgrad:
            self.pair_skips()
        kinds = {"stem_direct": self.stem_direct, "resample": self.resample, "act": self.act, "attn": self.attn, "conv": self.conv}
        for node in reversed(plan.nodes):
            if node["k"] != "head_direct":                     # (handled above)
                kinds[node["k"]](node)
        if self.pending_add:
            raise hip.RhoHipError("internal: a residual gradient was never added (backward plan)")
        if self.held_skips:
            raise hip.RhoHipError("internal: a held skip data gradient was never launched (backward plan)")
        self.fin_close(force=True)
        self.arena = torch.empty(max(self.arena_floats, 64), dtype=torch.float32, device=dev)
        arena_memset_info["bytes"] = 4.0 * self.arena.numel()
        plan.arena_bytes = 4 * self.arena.numel()          # (a fixed cost of the model's size, whatever the plan keeps of activations)
        pool.all.append(self.arena)
        self.embedding()
        if self.deterministic and self.det_ws_bytes > 0:
            self.det_ws = torch.empty((self.det_ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
            pool.all.append(self.det_ws)
        plan.pool_bytes = sum(t.numel() * t.element_size() for t in pool.all)
