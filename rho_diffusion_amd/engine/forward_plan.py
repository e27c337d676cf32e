"""Forward half of a plan: walks the ``UNet`` module tree and appends the launches of the embedding chain, the stem, every
ResBlock / AttentionBlock / Down / Upsample and the head to ``plan.ops``, and one node per differentiable step to ``plan.nodes``
(what ``backward_plan.BackwardBuilder`` walks in reverse).  Built once per plan by ``ForwardBuilder(plan).build()``; see the
module docstring of unet_engine for what is fused into which launch.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch
from torch import nn

from .. import hip
from ..hip import ptr
from . import ops
from .weights import _HeadAsGemm, _StemAsGemm

Tensor = torch.Tensor


def conv_node(cw, x1, x2, y, y2, out_dims, *, stride_hw=(1, 1), up_hw=(0, 0), pre=None, pre_silu=False, res=None, res_add_off=None,
              stem=False, xact=None, phased=False, s2=False, drop=None) -> dict:
    """The backward's view of one convolution (plan.nodes)."""
    return dict(k="conv", cw=cw, x1=x1, x2=x2, y=y, y2=y2, stride_hw=stride_hw, up_hw=up_hw, pre=pre, pre_silu=pre_silu, res=res,
                res_add_off=res_add_off, stem=stem, out_dims=out_dims, xact=xact, phased=phased, s2=s2, drop=drop)


class ForwardBuilder:
    """State of the forward construction of one ``_Plan``."""

    def __init__(self, plan):
        self.plan = plan
        self.eng = eng = plan.eng
        self.sw = sw = plan.sw
        self.L = plan.L
        self.train = train = plan.train
        self.dt = dt = eng.dtype
        self.dtc = hip.dtype_code(dt)
        self.dev = eng.device
        self.esz = 2 if dt == torch.bfloat16 else 4
        self.B = plan.B
        self.D, self.H, self.W = ops.spatial5(plan.xshape[2:])
        self.scratch_of: Dict[tuple, Tensor] = {}
        self.rs_hw = (1, 1) if eng.dims >= 2 else (0, 1)      # axes a Down/Upsample touches: H and W (3-D: depth stays), 1-D: W only
        # bf16 engine: the ResBlock's 1x1x1 skip convolution inside its out-conv's forward launch
        # (training plans: the forward launch only - backward keeps the skip branch's own data / weight-gradient launches)
        self.fold_skip = dt == torch.bfloat16 and sw.fold_skip
        # Inference plans of the bf16 engine run a 1-channel stem / head as 1x1x1 GEMMs (see rho_im2col_taps /
        # rho_tap_gather_sum: the 3x3x3 form pads the single channel to 32 and spends 31/32 of its matrix work on zeros).
        self.gemm_ends = (not train) and dt == torch.bfloat16 and sw.gemm_ends
        # 3-D, one input / output channel: each end is ONE launch with its intermediate in LDS (csrc/ends.hip) instead of the GEMM
        # form's two (im2col + GEMM, GEMM + tap gather).  Training plans: the same two forward launches; their backward =
        # GEMM-shaped weight gradients against an im2col of the one-channel operand (k_wgrad1) and, for the head's data gradient,
        # rho_stem_conv3d on dpred with mirrored taps - instead of 3x3x3 launches whose single channel is padded to 32
        self.direct_ends = dt == torch.bfloat16 and eng.dims == 3 and sw.direct_ends and (train or sw.gemm_ends)
        self.stem = self.stem_direct_w = None     # the stem's weights for ``conv``, or for the one rho_stem_conv3d launch

    # ------------------------------------------------------------------ buffers
    def buf(self, *shape, dtype=None) -> Tensor:
        t = torch.empty(*shape, dtype=dtype or self.dt, device=self.dev)
        self.plan.keep.append(t)
        return t

    def scratch(self, *shape, dtype=None) -> Tensor:
        """A buffer that is dead once the launch after its producer has run (the materialised activated input of ONE conv):
        shared by every request of the same size - launches of a plan are stream-ordered, also inside a captured graph."""
        key = (int(torch.Size(shape).numel()), dtype or self.dt)
        if key not in self.scratch_of:
            self.scratch_of[key] = self.buf(key[0], dtype=key[1])
        return self.scratch_of[key].view(*shape)

    def emit(self, fn, kind, flops=0.0, nbytes=0.0, **more) -> None:
        self.plan.ops.append(fn)
        self.plan.info.append(dict(kind=kind, flops=flops, bytes=nbytes, **more))

    # ------------------------------------------------------------------ helpers that append launches
    def embedding(self) -> None:
        """Embedding chain: table gather -> Linear -> (SiLU) Linear (+cond) -> (SiLU) batched FiLM GEMV.  Sinusoid + Linear + SiLU +
        Linear (+ label embedding) run as ONE launch at the head of run() (rho_timestep_embed: its timestep pointer changes per
        call); sin_in / emb_h are kept for the backward."""
        plan, eng, B = self.plan, self.eng, self.B
        e = 4 * eng.mc
        plan.t_in = self.buf(B, dtype=torch.int64)
        plan.sin_in = self.buf(B, eng.mc, dtype=torch.float32)
        plan.emb_h = self.buf(B, e, dtype=torch.float32)     # PRE-activation of time_embed[0]; the consumer applies SiLU
        plan.emb = self.buf(B, e, dtype=torch.float32)
        plan.cond = self.buf(B, e, dtype=torch.float32) if plan.has_y else None
        plan.film = self.buf(B, max(eng.film_total, 1), dtype=torch.float32)
        plan.cond_idx = self.buf(B, 16, dtype=torch.int32) if plan.has_y else None
        if eng.film_total:
            self.linear(plan.emb, eng.film_w, eng.film_b, None, plan.film, eng.act, False)

    def linear(self, xt, w, b, add, out, act_in, act_out) -> None:
        L = self.L
        Bn, K = xt.shape
        O = w.shape[0]
        args = (ptr(xt), ptr(w), ptr(b), ptr(add), ptr(out), Bn, K, O, int(act_in), int(act_out))
        self.plan.keep.append((xt, w, b, add, out))
        self.emit(lambda s, a=args: L.rho_linear(*a, s), "linear", flops=2.0 * Bn * K * O, nbytes=4.0 * (O * K + Bn * (K + O)))

    def gn(self, x1, x2, norm, film_blk=None) -> dict:
        plan, L, buf = self.plan, self.L, self.buf
        N, c1 = x1.shape[0], x1.shape[-1]
        c2 = x2.shape[-1] if x2 is not None else 0
        S, Cc = x1.numel() // (N * c1), c1 + c2
        nblk = ops.gn_nblk(S)
        part = buf(N * nblk * (Cc // 8) * 16, dtype=torch.float32)
        a = buf(N, Cc, dtype=torch.float32)
        b = buf(N, Cc, dtype=torch.float32)
        st = buf(N, 32, 2, dtype=torch.float32)
        scale = shift = off = None
        stride = 0
        if film_blk is not None:
            off = self.eng._film_off[id(film_blk)]
            scale, shift, stride = plan.film.data_ptr() + 4 * off, plan.film.data_ptr() + 4 * (off + Cc), plan.film.shape[1]
        # per-source partial sums: the producing convolution's fused epilogue statistics when it has them
        # (fmt 1, no extra read of the activation), else one rho_gn_partial pass over that source (fmt 0)
        srcs = []
        for xi, ci in ((x1, c1), (x2, c2)):
            if xi is None:
                continue
            ts = plan.tstats.get(xi.data_ptr())
            if ts is not None:
                srcs.append((ptr(ts[0]), 1, ts[1], ci))
            else:
                part_i = part if len(srcs) == 0 and x2 is None else buf(N * nblk * (ci // 8) * 16, dtype=torch.float32)
                a1 = (ptr(xi), ci, None, 0, self.dtc, N, S, ptr(part_i))
                self.emit(lambda s, a=a1: L.rho_gn_partial(*a, s), "gn_partial", flops=3.0 * N * S * ci, nbytes=float(self.esz) * N * S * ci)
                srcs.append((ptr(part_i), 0, nblk, ci))
        s2 = srcs[1] if len(srcs) > 1 else (None, 0, 0, 0)
        a2 = srcs[0] + s2 + (N, S, ptr(norm.weight), ptr(norm.bias), scale, shift, stride, ptr(st), ptr(a), ptr(b))
        self.emit(lambda s, a=a2: L.rho_gn_finalize2(*a, s), "gn_finalize", nbytes=4.0 * N * Cc * 4)
        return dict(x1=x1, x2=x2, norm=norm, film_off=off, a=a, b=b, st=st, part=part, N=N, S=S, C=Cc, nblk=nblk)

    def resample(self, xt, mode) -> Tensor:
        """avg_pool_nd (mode "avg") / nearest x2 (mode "up") of a channels-last tensor as its own pass: the conv-less
        Down/Upsample of conv_resample = False and the h_upd / x_upd of ResBlock(up / down) (unet_v2.py:122-131,165,221-224)."""
        L, rs_hw = self.L, self.rs_hw
        N_, Dd, Hh, Ww, Cc = xt.shape
        yt = self.buf(N_, Dd, Hh * 2 if rs_hw[0] else Hh, Ww * 2, Cc) if mode == "up" else self.buf(N_, Dd, Hh // 2 if rs_hw[0] else Hh, Ww // 2, Cc)
        a = (ptr(xt), ptr(yt), self.dtc, N_ * Dd, Hh, Ww, Cc, rs_hw[0], rs_hw[1])
        fn = (lambda s, a=a: L.rho_upsample2x(*a, s)) if mode == "up" else (lambda s, a=a: L.rho_avgpool2x(*a, s))
        self.emit(fn, "resample", nbytes=float(self.esz) * (xt.numel() + yt.numel()))
        self.plan.nodes.append(dict(k="resample", mode=mode, x=xt, y=yt))
        return yt

    def gn_apply(self, x1, x2, pre, act, out, drop=None) -> None:
        """out = act(a * concat(x1, x2) + b) (, dropout) as one HBM-rate pass."""
        self.emit(ops.gn_apply_launch(x1, x2, pre, act, out, drop, self.plan.drop_ctr), "gn_apply", nbytes=2.0 * self.esz * out.numel())

    def activated(self, x1, x2, pre, pre_silu) -> Tensor:
        """act(a * concat(x1, x2) + b) materialised as a tensor of its own (needed when something other than a conv loader
        consumes it: the h_upd of an up / down ResBlock resamples AFTER GroupNorm + SiLU, unet_v2.py:277-281)."""
        yt = self.buf(*x1.shape[:4], x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0))
        self.gn_apply(x1, x2, pre, pre_silu, yt)
        self.plan.nodes.append(dict(k="act", x1=x1, x2=x2, pre=pre, pre_silu=pre_silu, y=yt))
        return yt

    def drop_of(self, blk):
        """(p, seed, block) of the block's nn.Dropout when it is active in this plan, else None: one Philox key per block."""
        p_ = float(getattr(blk, "dropout", 0.0) or 0.0)
        if not self.plan.drop_active or p_ <= 0.0:
            return None
        idx = self.eng._film_blocks.index(blk)
        seed = (int(getattr(self.eng.model, "dropout_seed", 777)) + 0x9E3779B97F4A7C15 * (idx + 1)) & 0xFFFFFFFFFFFFFFFF
        return (p_, seed, blk)

    # ------------------------------------------------------------------ convolution: its five decisions, then the launches
    def conv_input(self, x1, x2, cw, up_hw, pre, pre_silu, ckpt, drop):
        """Decision 1 - does the conv read act(GroupNorm(x)) from a tensor (one materialising pass) or apply it in its loader?
        Returns (x1, x2, pre) as the launch sees them and the materialised tensor where the backward may reuse it."""
        plan, dt = self.plan, self.dt
        # 1x1x1 projections with many cout tiles (the attention qkv: 12 tiles of 128) redo the prologue per tile with
        # nothing to hide it under (probe: 0.70 ms with, 0.43 ms without, for 0.06 ms of materialising pass)
        wide_1x1 = cw.taps == 1 and cw.cout >= 512
        # 3x3(x3) convs with >= 2 cout tiles of 128 (the 256- and 512-wide levels): every cout tile redoes GroupNorm + SiLU on the
        # halo tile it stages (2.5x the input per tile): 8.5 % of the launch against a 0.05 ms pass that applies it once
        # (tools/ab_conv.py, "+pre" rows; only where the tensor is small enough that the extra pass costs less than the prologue)
        wide_3x3 = (cw.taps > 1 and cw.cout >= self.sw.materialize_min_cout and dt == torch.bfloat16)
        # ``ckpt`` (a ResBlock built with use_checkpoint=True; reference: layers.py:153-199 re-runs the block in backward instead of
        # keeping its intermediates): the activated inputs of the block's convs are NOT kept - backward re-materialises them
        # into a recycled buffer (the recompute path of bias_and_wgrad), the forward conv applies GroupNorm + FiLM + SiLU in its
        # loader or, for the wide layers, from a scratch copy that the next conv overwrites
        keep_act = self.train and self.sw.materialize_act and not ckpt
        # (an activation other than SiLU exists in the materialising pass only: the conv loaders know identity and SiLU)
        other_act = pre is not None and int(pre_silu) > 1
        if other_act and up_hw != (0, 0):
            raise hip.RhoHipError("internal: a normalised conv behind an upsample with a non-SiLU activation")
        if drop is not None and (pre is None or up_hw != (0, 0)):
            raise hip.RhoHipError("internal: dropout on a conv without a materialisable normalised input")
        if not (pre is not None and up_hw == (0, 0) and (keep_act or wide_1x1 or wide_3x3 or other_act or drop is not None)):
            return x1, x2, pre, None
        # training: the activated input act(a*x+b) is needed twice (this conv, its weight gradient) and the conv
        # loader would recompute it 2.3x (halo) per cout tile: materialise it once (one HBM-rate pass, kept for
        # backward: +1 activation-sized buffer per normalised conv, 38 GB at c3) and feed both from it
        xact = (self.buf if keep_act else self.scratch)(*x1.shape[:4], x1.shape[-1] + (x2.shape[-1] if x2 is not None else 0))
        self.gn_apply(x1, x2, pre, pre_silu, xact, drop)
        if drop is not None:
            plan.drop_delta = max(plan.drop_delta, (xact.numel() + 3) // 4)
            plan.drop_nodes.append(dict(blk=drop[2], p=float(drop[0]), seed=int(drop[1]), shape=tuple(xact.shape)))
        return xact, None, None, (xact if keep_act else None)

    def conv_form(self, x1, cw, out_dims, stride_hw, up_hw, plain_only: bool) -> str:
        """Decision 2 - "s2" (parity split of a stride-2 conv), "phased" (sub-pixel phases behind an upsample) or "plain".
        ``plain_only``: the launch has a prologue, a second input, a split output or a residual, which only the plain form knows."""
        sw = self.sw
        npos = out_dims[0] * out_dims[1] * out_dims[2] * out_dims[3]
        tiles_c = max(1, cw.coutp // 128)
        # A conv behind a nearest x2 upsample as one 2-tap launch per output parity on the SOURCE tensor (rho_conv_desc.ph_h):
        # 12 / 27 of the multiply-adds in 3-D, same result up to the rounding of the summed weights.
        # (only where each phase launch still fills the chip: on the small 2-D grids of c1 four launches of a few workgroups
        #  each are slower than one - 20.2 -> 21.5 ms per step there)
        n_ph = (2 if up_hw[0] else 1) * (2 if up_hw[1] else 1)
        phased = (sw.phase_upsample and up_hw != (0, 0) and not plain_only and all(cw.kernel[1 + i] == 3 for i in range(2) if up_hw[i])
                  and (npos // n_ph // 256) * tiles_c >= sw.phase_min_wgs)
        # Downsample's stride-(1, 2, 2) conv as four stride-1 launches, one per input parity, accumulated in place: no 2x halo
        # per strided tile (the strided loader ran 380 - 870 TF/s), same multiply-adds
        s2 = (sw.s2_split and tuple(stride_hw) == (2, 2) and tuple(cw.kernel) == (3, 3, 3) and up_hw == (0, 0) and not plain_only
              and x1.shape[2] % 2 == 0 and x1.shape[3] % 2 == 0 and (npos // 256) * tiles_c >= sw.phase_min_wgs)
        return "s2" if s2 else "phased" if phased else "plain"

    def conv_descs(self, form, x1, x2, pre, pre_silu, cw, y, y2, split, stride_hw, up_hw, res, res_add_off, fold_skip) -> list:
        """Decision 3 - the rho_conv_desc of every launch of this conv."""
        cout, film = cw.cout, self.plan.film
        if form == "s2":
            cw.enable_s2(dgrad=self.train)
            return [ops.make_conv_desc(x1, None, wt, cw.b if i == 0 else cw.zero_b, kernel=(3, len(cw.S2_FWD[a]), len(cw.S2_FWD[b])),
                                       cout=cout, split=split, y=y, y2=None, res=y if i > 0 else None, phase_dgrad_hw=(a + 1, b + 1))
                    for i, ((a, b), wt) in enumerate(cw.ws2)]
        if form == "phased":
            cw.enable_phases(up_hw, dgrad=self.train)
            return [ops.make_conv_desc(x1, None, wt, cw.b, kernel=cw.phase_kernel(ph), cout=cout, split=split, y=y, y2=None, phase_hw=ph)
                    for ph, wt in cw.wph]
        d = ops.make_conv_desc(x1, x2, cw.w, cw.b, kernel=cw.kernel, cout=cout, split=split, y=y, y2=y2, stride_hw=stride_hw,
                               up_hw=up_hw, pre_a=pre["a"] if pre else None, pre_b=pre["b"] if pre else None,
                               pre_silu=pre_silu if pre else False, res=res, res_add=None, skip=fold_skip)
        if res_add_off is not None:
            d.res_add = film.data_ptr() + 4 * res_add_off
            d.res_add_stride = film.shape[1]
        return [d]

    def conv_stats(self, descs, form, y, N, cout) -> None:
        """Decision 4 - GroupNorm statistics of the output ride along in the epilogue where the geometry allows it (phases: all
        launches of this output together; parity split: the last launch stores the final values)."""
        carriers = descs[-1:] if form == "s2" else descs
        tiles = int(self.L.rho_conv_stats_tiles(C.byref(carriers[0])))
        if tiles > 0:
            sbuf = self.buf(N * tiles * 2 * cout, dtype=torch.float32)
            for d in carriers:
                d.stats = sbuf.data_ptr()
            self.plan.tstats[y.data_ptr()] = (sbuf, tiles)

    def conv_launches(self, descs, form, cw, npos_in, npos_out, has_res) -> None:
        """Decision 5 - the launches and their roofline bookkeeping (algorithmic = unpadded MACs * 2)."""
        plan, L, cout, n = self.plan, self.L, cw.cout, len(descs)
        s2 = form == "s2"
        for d in descs:
            plan.keep.append(d)
            plan.fwd_descs.append(d)
            taps_run = d.kd * d.kh * d.kw
            self.emit(lambda s, d=d: L.rho_conv_nd_fwd(C.byref(d), s), "conv3" if cw.taps > 1 else "conv1", taps=cw.taps, cin=cw.cin,
                      cout=cout, positions=npos_out if s2 else npos_out // n,
                      flops=2.0 * npos_out * cout * cw.cin * taps_run if s2 else 2.0 * npos_out * cout * cw.cin * cw.taps / n,
                      executed_flops=2.0 * npos_out * cout * cw.cin * taps_run / (1 if s2 else n),
                      nbytes=float(self.esz) * (npos_in * cw.cin + npos_out * cout * (2 if has_res else 1) / n + taps_run * cout * cw.cin))

    def conv(self, x1, x2, cw, *, stride_hw=(1, 1), up_hw=(0, 0), pre=None, pre_silu=False, res=None, res_add_off=None,
             split=None, y2_dtype=None, stem=False, want_stats=True, ckpt=False, fold_skip=None, node_res=None, drop=None):
        cout = cw.cout
        split_ = cout if split is None else split
        out_dims = N, Do, Ho, Wo = ops.conv_out_shape(x1.shape, cw.kernel, stride_hw, up_hw)
        y = self.buf(N, Do, Ho, Wo, split_) if split_ > 0 else None
        y2 = self.buf(N, cout - split_, Do * Ho * Wo, dtype=y2_dtype or self.dt) if split_ < cout else None
        cx1, cx2, cpre, xact = self.conv_input(x1, x2, cw, up_hw, pre, pre_silu, ckpt, drop)
        plain_only = cpre is not None or cx2 is not None or split_ != cout or res is not None or res_add_off is not None
        form = self.conv_form(x1, cw, out_dims, stride_hw, up_hw, plain_only)
        descs = self.conv_descs(form, cx1, cx2, cpre, pre_silu, cw, y, y2, split_, stride_hw, up_hw, res, res_add_off, fold_skip)
        if y is not None and split_ == cout and want_stats:
            self.conv_stats(descs, form, y, N, cout)
        self.conv_launches(descs, form, cw, x1.numel() // x1.shape[-1], N * Do * Ho * Wo, res is not None)
        # (node_res: the backward's view of a folded skip - the gradient of this output also belongs to the skip branch's node)
        self.plan.nodes.append(conv_node(cw, x1, x2, y, y2, out_dims, stride_hw=stride_hw, up_hw=up_hw, pre=pre, pre_silu=pre_silu,
                                         res=res if node_res is None else node_res, res_add_off=res_add_off, stem=stem, xact=xact,
                                         phased=form == "phased", s2=form == "s2", drop=drop))
        return y, y2

    # ------------------------------------------------------------------ blocks
    def folded_skip_out(self, blk, h1, h2, t1, g2, skw, ocw):
        """skip_connection(x) + out_layers(h) (unet_v2.py:245-256,293) in ONE forward launch - the 1x1x1 skip is contracted into
        the out-conv's accumulators before its tap loop (rho_conv_desc.sk_*): no launch, no `sk` tensor written and read back as
        the residual.  None where the kernel has no such variant (rho_conv_variant says so: narrow / wide cout tiles, large
        halos): the two launches stay."""
        plan = self.plan
        fs = (h1, h2, skw.w, skw.b)
        probe = ops.make_conv_desc(t1, None, ocw.w, ocw.b, kernel=ocw.kernel, cout=ocw.cout, split=ocw.cout, y=t1, y2=None, skip=fs)
        if self.L.rho_conv_variant(C.byref(probe), C.create_string_buffer(128), 128) != 0:
            return None
        skd = None
        if self.train:
            # backward is the unfused graph: a node for the skip branch whose "output" is a key-only tensor; the
            # out-conv's node names it as its residual, so its dY is aliased to the skip node exactly as before
            skd = self.buf(8, dtype=torch.uint8)
            plan.nodes.append(conv_node(skw, h1, h2, skd, None, tuple(t1.shape[:4])))
        out, _ = self.conv(t1, None, ocw, pre=g2, pre_silu=self.eng.act, ckpt=bool(blk.use_checkpoint), fold_skip=fs, node_res=skd,
                           drop=self.drop_of(blk))
        # the launch's work = the 27-tap conv + the folded 1x1x1 (both algorithmic FLOPs of the reference's
        # formulation); the 1x1x1 share is also reported on its own (bench: roofline.folded_conv1_flops_per_step)
        npos, info = t1.numel() // t1.shape[-1], plan.info[-1]
        info["folded_conv1_flops"] = fl = 2.0 * npos * ocw.cout * skw.cin
        info["flops"] += fl
        info["executed_flops"] += fl
        info["bytes"] += float(self.esz) * npos * skw.cin
        return out

    def resblock(self, blk, h1, h2):
        """ResBlock._forward (unet_v2.py:273-293).  The up / down form differs in where the three inputs come from - the in-conv
        reads the resampled activated tensor, the skip branch the resampled block input - and in not folding the skip."""
        from ..models.unet_v2 import Upsample
        eng = self.eng
        ck = bool(blk.use_checkpoint)
        in_cw, ocw = eng._conv(blk.in_layers[2]), eng._conv(blk.out_layers[3])
        g1 = self.gn(h1, h2, blk.in_layers[0])
        radd = None if blk.use_scale_shift_norm else eng._film_off[id(blk)]
        updown = getattr(blk, "updown", False)
        if updown:
            mode = "up" if isinstance(blk.h_upd, Upsample) else "avg"
            hh = self.resample(self.activated(h1, h2, g1, eng.act), mode)
            s1 = self.resample(h1, mode)
            s2 = self.resample(h2, mode) if h2 is not None else None
            t1, _ = self.conv(hh, None, in_cw, res_add_off=radd)
        else:
            s1, s2 = h1, h2
            t1, _ = self.conv(h1, h2, in_cw, pre=g1, pre_silu=eng.act, res_add_off=radd, ckpt=ck)
        g2 = self.gn(t1, None, blk.out_layers[0], film_blk=blk if blk.use_scale_shift_norm else None)
        if isinstance(blk.skip_connection, nn.Identity):
            assert s2 is None
            sk = s1
        else:
            skw = eng._conv(blk.skip_connection)
            if self.fold_skip and not updown and skw.taps == 1 and ocw.taps == 27:
                out = self.folded_skip_out(blk, h1, h2, t1, g2, skw, ocw)
                if out is not None:
                    return out
            sk, _ = self.conv(s1, s2, skw)
        out, _ = self.conv(t1, None, ocw, pre=g2, pre_silu=eng.act, res=sk, ckpt=ck, drop=self.drop_of(blk))
        return out

    def attention(self, blk, xin):
        L, eng = self.L, self.eng
        N, Dd, Hh, Ww, Cc = xin.shape
        T = Dd * Hh * Ww
        g = self.gn(xin, None, blk.norm)
        qk, vt = self.conv(xin, None, eng._conv(blk.qkv), pre=g, pre_silu=False, split=2 * Cc)
        ao = self.buf(N, Dd, Hh, Ww, Cc)
        lse = self.buf(N, blk.num_heads, T, dtype=torch.float32) if self.train else None
        args = (ptr(qk), ptr(vt), ptr(ao), ptr(lse), self.dtc, N, T, blk.num_heads, Cc // blk.num_heads)
        self.emit(lambda s, a=args: L.rho_attention_fwd(*a, s), "attention", flops=4.0 * N * T * T * Cc, nbytes=float(self.esz) * 4 * N * T * Cc)
        self.plan.nodes.append(dict(k="attn", qk=qk, vt=vt, ao=ao, lse=lse, heads=blk.num_heads, N=N, T=T, C=Cc))
        out, _ = self.conv(ao, None, eng._conv(blk.proj_out), res=xin)
        return out

    def block(self, seq, h1, h2):
        from ..models.unet_v2 import AttentionBlock, Downsample, ResBlock, Upsample
        eng = self.eng
        for layer in seq:
            if isinstance(layer, ResBlock):
                h1, h2 = self.resblock(layer, h1, h2), None
            elif isinstance(layer, AttentionBlock):
                h1 = self.attention(layer, h1)
            elif isinstance(layer, Downsample):
                if not layer.use_conv:
                    h1 = self.resample(h1, "avg")
                else:
                    h1, _ = self.conv(h1, None, eng._conv(layer.op), stride_hw=(2, 2) if eng.dims >= 2 else (1, 2))
            elif isinstance(layer, Upsample):
                if not layer.use_conv:
                    h1 = self.resample(h1, "up")
                else:
                    h1, _ = self.conv(h1, None, eng._conv(layer.conv), up_hw=self.rs_hw)
            elif self.stem_direct_w is not None:  # the stem conv as one launch on the fp32 input (rho_stem_conv3d)
                h1 = self.stem_direct()
            else:  # the stem conv
                h1, _ = self.conv(h1, None, self.stem, stem=True)
        return h1

    # ------------------------------------------------------------------ the two ends
    def select_stem(self) -> None:
        """The input buffers and the form the stem conv runs in: one direct launch, a GEMM over an im2col, or the generic conv on
        the channels-last packed input (the last two pack here; the conv itself is launched by ``block``)."""
        plan, eng, L, B, D, H, W = self.plan, self.eng, self.L, self.B, self.D, self.H, self.W
        xshape, mod = plan.xshape, eng.model.input_blocks[0][0]
        self.stem = stem = eng._conv(mod)
        plan.x_in = self.buf(*xshape, dtype=torch.float32)
        if self.direct_ends and xshape[1] == 1 and tuple(stem.kernel) == (3, 3, 3) and stem.cout in (32, 64):
            self.stem_direct_w = eng._conv_as_gemm(mod, _StemAsGemm)
            plan.x_cl = plan.x_in
            return
        if self.gemm_ends and stem.taps > 1 and stem.cin * stem.taps <= 32:
            self.stem = stem = eng._conv_as_gemm(mod, _StemAsGemm)
            plan.x_cl = self.buf(B, D, H, W, stem.cinp)
            pk = (ptr(plan.x_in), ptr(plan.x_cl), self.dtc, B, xshape[1], D, H, W) + stem.kernel3 + (stem.cinp,)
            fn = lambda s, a=pk: L.rho_im2col_taps(*a, s)      # noqa: E731
        else:
            plan.x_cl = self.buf(B, D, H, W, stem.cinp)
            pk = (ptr(plan.x_in), ptr(plan.x_cl), self.dtc, B, xshape[1], D * H * W, stem.cinp)
            fn = lambda s, a=pk: L.rho_pack_input(*a, s)       # noqa: E731
        self.emit(fn, "pack", nbytes=4.0 * B * xshape[1] * D * H * W + 2.0 * B * D * H * W * stem.cinp)

    def stem_direct(self) -> Tensor:
        plan, L, B, D, H, W, sg = self.plan, self.L, self.B, self.D, self.H, self.W, self.stem_direct_w
        y = self.buf(B, D, H, W, sg.cout)
        tiles = ops.stem_conv3d_tiles(D, H, W)
        sbuf = self.buf(B * tiles * 2 * sg.cout, dtype=torch.float32)
        a = (ptr(plan.x_in), ptr(sg.w), ptr(sg.b), ptr(y), ptr(sbuf), B, D, H, W, sg.cout)
        plan.tstats[y.data_ptr()] = (sbuf, tiles)
        npos = B * D * H * W
        self.emit(lambda s_, a=a: L.rho_stem_conv3d(*a, s_), "stem", flops=2.0 * npos * sg.cout * 27,
                  nbytes=4.0 * npos + float(self.esz) * npos * sg.cout)
        if self.train:
            plan.nodes.append(dict(k="stem_direct", y=y, cw=self.stem, out_dims=(B, D, H, W)))
        return y

    def head(self, h) -> Tensor:
        """Final GroupNorm - activation - conv (unet_v2.py:679-683) -> float32 [B, Cout, S]: one direct launch, a GEMM + tap
        gather, or the generic conv."""
        plan, eng, L, B, D, H, W, train = self.plan, self.eng, self.L, self.B, self.D, self.H, self.W, self.train
        mod = eng.model.out[2]
        g = self.gn(h, None, eng.model.out[0])
        head = eng._conv(mod)
        Ch = h.shape[-1]
        if (self.direct_ends and tuple(head.kernel) == (3, 3, 3) and head.cout == 1
                and Ch in ((32, 64) if train else (32, 64, 96, 128))):      # (training: dpred -> dact runs on rho_stem_conv3d)
            hg = eng._conv_as_gemm(mod, _HeadAsGemm)
            y2 = self.buf(B, 1, D * H * W, dtype=torch.float32)
            npos = B * D * H * W
            if train or eng.act != 1:
                # training: the activated input is kept (the head's weight gradient contracts it with the im2col of dpred);
                # a non-SiLU activation: applied by the materialising pass (the head kernel's own prologue knows SiLU only)
                xact = (self.buf if train else self.scratch)(B, D, H, W, Ch)
                self.gn_apply(h, None, g, eng.act, xact)
                ga = (ptr(xact), None, None, 0, ptr(hg.w), ptr(mod.bias), ptr(y2), B, D, H, W, Ch)
                if train:
                    plan.nodes.append(dict(k="head_direct", x=h, pre=g, xact=xact, cw=head, y2=y2, out_dims=(B, D, H, W)))
            else:
                ga = (ptr(h), ptr(g["a"]), ptr(g["b"]), 1, ptr(hg.w), ptr(mod.bias), ptr(y2), B, D, H, W, Ch)
            plan.keep.append(g)
            self.emit(lambda s, a=ga: L.rho_head_conv3d(*a, s), "head", flops=2.0 * npos * Ch * 27, nbytes=float(self.esz) * npos * Ch + 4.0 * npos)
        elif self.gemm_ends and head.taps > 1 and head.cout == 1:
            hg = eng._conv_as_gemm(mod, _HeadAsGemm)
            tt, _ = self.conv(h, None, hg, pre=g, pre_silu=eng.act, want_stats=False)          # [B, D, H, W, 32]: one column per tap
            y2 = self.buf(B, 1, D * H * W, dtype=torch.float32)
            ga = (ptr(tt), self.dtc, B, D, H, W) + hg.kernel3 + (hg.coutp, ptr(mod.bias), ptr(y2))
            self.emit(lambda s, a=ga: L.rho_tap_gather_sum(*a, s), "tap_sum", nbytes=2.0 * tt.numel() + 4.0 * y2.numel())
        else:
            _, y2 = self.conv(h, None, head, pre=g, pre_silu=eng.act, split=0, y2_dtype=torch.float32)
        return y2

    # ------------------------------------------------------------------ the plan
    def build(self) -> None:
        plan, m = self.plan, self.eng.model
        self.embedding()
        self.select_stem()
        hs: List[Tensor] = []
        h: Optional[Tensor] = plan.x_cl
        for blk in m.input_blocks:
            h = self.block(blk, h, None)
            hs.append(h)
        h = self.block(m.middle_block, h, None)
        for blk in m.output_blocks:
            h = self.block(blk, h, hs.pop())
        plan.out = self.head(h).view(self.B, m.out_channels, *plan.xshape[2:])
