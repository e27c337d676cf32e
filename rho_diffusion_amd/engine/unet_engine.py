"""Lowering of a ``UNet`` module tree (models/unet_v2.py) to flat lists of HIP kernel launches,
forward AND backward.

Reference semantics: UNet.forward, rho_diffusion/models/unet_v2.py:685-732, with ResBlock._forward
(:273-293), AttentionBlock._forward (:336-342), Downsample / Upsample (:103-169) and the final
GroupNorm-SiLU-conv (:679-683); the backward is what torch autograd derives for those ops.

Forward, per ResBlock:
    gn_partial, gn_finalize            statistics + folded (GroupNorm * FiLM) affine per (n, c)
    conv3   (prologue: affine+SiLU)    in_layers   [+ additive embedding in the epilogue]
    gn_partial, gn_finalize
    [conv1x1 skip]
    conv3   (prologue: affine+SiLU, epilogue: + skip)
torch.cat of the skip connections, nearest-upsample, strides, SiLU, FiLM and residual adds never
exist as separate passes over HBM.

Backward, per conv: bias gradient (channel sums of dY), weight gradient (rho_conv_nd_wgrad, input
activation recomputed in its loader), data gradient (the forward kernel on dY with flipped /
transposed weights) followed by the GroupNorm+FiLM+SiLU backward (reduce / finalize / apply).
Only pre-norm activations, GroupNorm statistics and the attention log-sum-exp are kept from the
forward; normalised / activated tensors and attention probabilities are recomputed (the reference
recomputes attention too, unet_v2.py:334).  Where a tensor has several consumers its gradient
buffer is aliased (identity skips, residuals) or accumulated in the producing kernel's epilogue;
the choice is made once, when the plan is built.

A plan (all descriptors + all buffers) is built once per (batch, spatial shape, mode) and replayed;
buffer addresses are stable.  PyTorch supplies memory and streams only.  ``_Plan`` holds a plan's state and replays it; its
launches are appended by ``forward_plan.ForwardBuilder`` and, for a training plan, ``backward_plan.BackwardBuilder``.  The
prepared weight layouts live in ``weights``.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import hip
from ..hip import check, ptr
from . import ops
from .backward_plan import BackwardBuilder
from .forward_plan import ForwardBuilder
from .weights import _ConvW, _HeadDgradW

Tensor = torch.Tensor


PlanSwitches = namedtuple("PlanSwitches", "materialize_act materialize_min_cout phase_upsample phase_upsample_bwd phase_min_wgs fold_skip "
                                     "s2_split s2_split_bwd fuse_gn_bwd gemm_ends direct_ends fuse_skip_dgrad gemm1x1 conv_geo")


class UNetEngine:
    def __init__(self, model: nn.Module, dtype: torch.dtype):
        self.model = model
        self.dtype = dtype
        p = next(model.parameters())
        hip.require_gpu(p, "UNet parameters")
        hip.load()
        self.device = p.device
        self.dims = model.dims
        self.mc = model.model_channels
        self.ssn = bool(model.use_scale_shift_norm)
        # activation code of the network (1 = SiLU: fused into the conv loaders; anything else runs in the materialising passes)
        self.act = int(getattr(model, "act_code", 1))
        self._plans: Dict[tuple, "_Plan"] = {}
        self._convs: List[_ConvW] = []
        self._aux_weights: list = []          # prepared layouts that are not convolutions of their own (see _head_dgrad)
        self._conv_of: Dict[int, _ConvW] = {}
        self._film_blocks: List[nn.Module] = []
        self._omega: Optional[Tensor] = None
        self._cond_dev = None      # device-side tables of the label embedding (MultiEmbeddings), built on first use
        self._param_version = -1
        self._ptr_sig = None
        self._prep_table = None
        self._prep_sig = None
        self._prep_eager: List[_ConvW] = []
        self._last_train_plan: Optional["_Plan"] = None
        self._train_generation = 0      # counts forward(train=True) calls: a backward names the forward it belongs to (backward())
        self._cond_keep: Optional[Tensor] = None      # label-dropout mask for the next training forward (set_cond_keep)
        with torch.inference_mode(False):
            self._collect()
            self.refresh_weights(force=True)

    # ------------------------------------------------------------------ weights
    def _conv(self, mod: nn.Module, row_src: Optional[Tensor] = None) -> _ConvW:
        key = id(mod)
        if key not in self._conv_of:
            cw = _ConvW(mod.weight, mod.bias, self.dtype, row_src)
            self._conv_of[key] = cw
            self._convs.append(cw)
        return self._conv_of[key]

    def _conv_as_gemm(self, mod: nn.Module, cls) -> _ConvW:
        """The stem / head convolution re-read as a 1x1x1 GEMM (inference plans of the bf16 engine)."""
        key = (id(mod), cls.__name__)
        if key not in self._conv_of:
            cw = cls(mod.weight, mod.bias, self.dtype)
            self._conv_of[key] = cw
            self._convs.append(cw)
        return self._conv_of[key]

    def _head_dgrad(self, mod: nn.Module) -> "_HeadDgradW":
        """Mirrored taps-as-contraction weights of the one-channel head conv (training plans: its data gradient runs on rho_stem_conv3d)."""
        key = (id(mod), "_HeadDgradW")
        if key not in self._conv_of:
            hw = _HeadDgradW(mod.weight, self.dtype)
            self._conv_of[key] = hw
            self._aux_weights.append(hw)
        return self._conv_of[key]

    def _qkv_row_src(self, blk) -> Tensor:
        """Row gather that brings the qkv projection to the canonical [Q heads | K heads | V heads]
        order the attention kernel reads (legacy order interleaves q,k,v per head, unet_v2.py:384)."""
        c, h = blk.channels, blk.num_heads
        ch = c // h
        idx = torch.arange(3 * c, dtype=torch.int64)
        if not blk.use_new_attention_order:
            part = idx // c            # 0 = q, 1 = k, 2 = v in the canonical layout
            head = (idx % c) // ch
            i = idx % ch
            idx = head * 3 * ch + part * ch + i
        return idx.to(torch.int32).to(self.device)

    def _collect(self) -> None:
        from ..models.unet_v2 import AttentionBlock, Downsample, ResBlock, Upsample
        m = self.model
        for mod in m.modules():
            if isinstance(mod, ResBlock):
                self._film_blocks.append(mod)
                self._conv(mod.in_layers[2])
                self._conv(mod.out_layers[3])
                if not isinstance(mod.skip_connection, nn.Identity):
                    self._conv(mod.skip_connection)
            elif isinstance(mod, AttentionBlock):
                self._conv(mod.qkv, self._qkv_row_src(mod))
                self._conv(mod.proj_out)
            elif isinstance(mod, Downsample):
                if mod.use_conv:
                    self._conv(mod.op)
            elif isinstance(mod, Upsample):
                if mod.use_conv:
                    self._conv(mod.conv)
        self._conv(m.input_blocks[0][0])
        self._conv(m.out[2])
        # FiLM / additive-embedding projections of all ResBlocks, batched into one GEMV launch
        self._film_off: Dict[int, int] = {}
        off = 0
        for blk in self._film_blocks:
            self._film_off[id(blk)] = off
            off += blk.emb_layers[1].weight.shape[0]
        self.film_total = off
        e = 4 * self.mc
        self.film_w = torch.empty(off, e, dtype=torch.float32, device=self.device)
        self.film_b = torch.empty(off, dtype=torch.float32, device=self.device)

    def _versions(self) -> int:
        return sum(p._version for p in self.model.parameters())

    def _pointer_signature(self) -> int:
        return hash(tuple(p.data_ptr() for p in self.model.parameters()))

    def refresh_weights(self, force: bool = False) -> None:
        """Re-run the weight preparation kernels if any parameter changed (optimizer step, load_state_dict);
        drop the plans if parameter storage moved (e.g. re-homed into an optimizer arena).

        A change is seen through the parameters' version counters: every in-place torch op bumps them (``p.copy_`` under
        ``no_grad``, the stock optimizers, ``load_state_dict``), and the library's own raw-pointer writers bump them by hand
        (``HipAdamW.step``, ``ExponentialMovingAverage.update``).  A write through ``p.data`` - or any other raw-pointer write -
        bypasses the counter: after one, call ``refresh_weights(force=True)``, or the convolutions keep the layouts prepared from
        the old values."""
        sig = self._pointer_signature()
        if self._ptr_sig is not None and sig != self._ptr_sig:
            self._plans.clear()
            self._last_train_plan = None
            force = True
        self._ptr_sig = sig
        v = self._versions()
        if not force and v == self._param_version:
            return
        # ONE launch (rho_prep_batch) re-packs every layout of every conv, the padded biases and the FiLM matrix; the table is
        # rebuilt when a layout is added (first training plan, phases, parity splits) or parameter storage moves
        allw = self._convs + self._aux_weights
        lsig = tuple(cw.layout_signature() for cw in allw) + tuple(blk.emb_layers[1].weight.data_ptr() for blk in self._film_blocks)
        if self._prep_table is None or self._prep_sig != lsig:
            table = ops.PrepTable(self.device)
            self._prep_eager = [cw for cw in allw if not cw.prep_into(table)]
            off = 0
            for blk in self._film_blocks:
                lin = blk.emb_layers[1]
                n = lin.weight.shape[0]
                table.add_vec(lin.weight.detach().reshape(-1), self.film_w[off:off + n].reshape(-1))
                table.add_vec(lin.bias.detach(), self.film_b[off:off + n])
                off += n
            self._prep_table, self._prep_sig = table, lsig
        self._prep_table.launch()
        for cw in self._prep_eager:
            cw.refresh()
        self._param_version = v

    def omega(self) -> Tensor:
        """Denominators wavelength^(2i / mc) of the timestep sinusoid (float32 [mc / 2]); the kernel evaluates sin / cos for any t."""
        if self._omega is None:
            self._omega = ops.sinusoid_frequencies(self.mc, 10000, self.device)
        return self._omega

    def err_flag(self) -> Tensor:
        """int32[1] device flag the kernels OR error bits into (bit 1: label not in the parameter space); polled by ``check_errors``."""
        if getattr(self, "_err_flag", None) is None:
            self._err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._err_flag

    def check_errors(self) -> None:
        """Host poll of the device error flag (one synchronisation: call it outside the hot loop)."""
        if getattr(self, "_err_flag", None) is not None:
            v = int(self._err_flag.item())
            if v & 2:
                self._err_flag.zero_()
                raise IndexError("MultiEmbeddings: a label value is not in the parameter space (conditioning.py:132)")

    def cond_device_tables(self):
        """Device-side description of ``model.cond_fn`` when it is a MultiEmbeddings (conditioning.py:31-139): the value lists of
        the parameter space concatenated as float32, their offsets, and a pointer array of the embedding tables.  None for any
        other cond_fn module (evaluated as given)."""
        from ..models.conditioning import MultiEmbeddings
        fn = getattr(self.model, "cond_fn", None)
        if not isinstance(fn, MultiEmbeddings) or fn.parameter_space is None or len(fn.embedding_layers) == 0:
            return None
        weights = [layer.weight for layer in fn.embedding_layers.values()]
        sig = tuple(w.data_ptr() for w in weights)
        if self._cond_dev is not None and self._cond_dev["sig"] == sig:
            return self._cond_dev
        keys = list(fn.embedding_layers.keys())
        if len(keys) > 16:
            return None
        vals, off = [], [0]
        for k in keys:
            v = torch.tensor(fn.parameter_space[k]).to(torch.float32)      # torch.tensor(list): the reference's conversion (:131)
            vals.append(v)
            off.append(off[-1] + v.numel())
        dev = self.device
        self._cond_dev = dict(sig=sig, nkeys=len(keys), weights=weights,
                              space=torch.cat(vals).to(dev).contiguous(),
                              key_off=torch.tensor(off, dtype=torch.int32, device=dev),
                              tables=torch.tensor(list(sig), dtype=torch.int64, device=dev))
        return self._cond_dev

    def param_order(self) -> List[nn.Parameter]:
        """Embedding-path parameters first (their gradients complete last), then every other parameter in
        forward order: backward finalises gradients from the tail of this list to its head, so contiguous
        ranges of an optimizer arena laid out this way are ready-made data-parallel all-reduce buckets."""
        emb = list(self.model.time_embed.parameters())
        for blk in self._film_blocks:
            emb.extend(blk.emb_layers[1].parameters())
        if getattr(self.model, "cond_fn", None) is not None:
            emb.extend(self.model.cond_fn.parameters())
        emb_ids = {id(p_) for p_ in emb}
        main = [p_ for p_ in self.model.parameters() if id(p_) not in emb_ids]
        return emb + main

    # ------------------------------------------------------------------ forward / backward
    def set_cond_keep(self, keep: Optional[Tensor]) -> None:
        """Label dropout (classifier-free guidance training): hand the NEXT ``forward(train=True)`` a keep mask [B] (nonzero = the
        sample keeps its labels).  A dropped sample's condition becomes the zero row and contributes no gradient to the label
        embedding.  One forward consumes the mask; inference forwards neither see nor consume it; None withdraws it."""
        self._cond_keep = keep

    def forward(self, x: Tensor, timesteps: Tensor, y: Optional[Tensor] = None,
                t_scalar_dev: Optional[Tensor] = None, train: bool = False) -> Tensor:
        hip.require_gpu(x, "x")
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        self.refresh_weights()
        key = (tuple(x.shape), y is not None, bool(train)) + self._plan_signature()
        plan = self._plans.get(key)
        if plan is None:
            with torch.inference_mode(False), torch.no_grad():     # plan buffers must stay ordinary tensors
                plan = self._plans[key] = _Plan(self, tuple(x.shape), y is not None, bool(train))
        keep = None
        if train:
            self._last_train_plan = plan
            self._train_generation += 1
            keep, self._cond_keep = self._cond_keep, None
        return plan.run(x, timesteps, y, t_scalar_dev, keep)

    # environment switches a plan reads while it is built (A/B knobs): part of the plan key, so flipping one rebuilds the plan
    # (exactly the names _plan_switches reads, the engine's only reads - tests/test_host_logic.py holds the two together; the library's
    #  own RHO_CONV_SPLITK is latched at its first launch, so no rebuild could follow it and it is not part of the key; RHO_CONV_GEO is
    #  latched the same way and listed all the same, so that plans built under different settings never share a key)
    _PLAN_ENV = ("RHO_TRAIN_MATERIALIZE", "RHO_MATERIALIZE_MIN_COUT", "RHO_PHASE_UPSAMPLE", "RHO_PHASE_UPSAMPLE_BWD", "RHO_PHASE_MIN_WGS",
                 "RHO_FOLD_SKIP", "RHO_S2_SPLIT", "RHO_S2_SPLIT_BWD", "RHO_FUSE_GN_BWD", "RHO_GEMM_ENDS", "RHO_DIRECT_ENDS",
                 "RHO_FUSE_SKIP_DGRAD", "RHO_GEMM1X1", "RHO_CONV_GEO")

    @staticmethod
    def _plan_switches() -> PlanSwitches:
        """The switches of ``_PLAN_ENV`` parsed into the immutable record both plan builders read (``plan.sw``)."""
        return PlanSwitches(
            materialize_act=os.environ.get("RHO_TRAIN_MATERIALIZE", "1") != "0",       # memory-for-time trade of training plans
            materialize_min_cout=int(os.environ.get("RHO_MATERIALIZE_MIN_COUT", "256")),
            phase_upsample=os.environ.get("RHO_PHASE_UPSAMPLE", "1") != "0",           # Upsample + conv as sub-pixel phases
            phase_upsample_bwd=os.environ.get("RHO_PHASE_UPSAMPLE_BWD", "1") != "0",
            phase_min_wgs=int(os.environ.get("RHO_PHASE_MIN_WGS", "256")),
            fold_skip=os.environ.get("RHO_FOLD_SKIP", "1") != "0",      # bf16: a ResBlock's 1x1x1 skip inside its out-conv's forward launch
            s2_split=os.environ.get("RHO_S2_SPLIT", "1") != "0",
            s2_split_bwd=os.environ.get("RHO_S2_SPLIT_BWD", "1") != "0",
            # backward: GroupNorm's reductions (sum dz, sum dz * x) in the epilogue of the dgrad launch that produces dz - from this
            # many channels up (0 = never): on the 64-channel layers the extra epilogue VALU work (one sigmoid per element) costs the
            # issue-bound narrow tiles more than the separate reduce pass it replaces
            fuse_gn_bwd=int(os.environ.get("RHO_FUSE_GN_BWD", "128")),
            gemm_ends=os.environ.get("RHO_GEMM_ENDS", "1") != "0",
            direct_ends=os.environ.get("RHO_DIRECT_ENDS", "1") != "0",
            # backward of a ResBlock with a 1x1x1 skip convolution: the skip's data gradient and the GroupNorm backward apply of the
            # in-conv path write the same dX - one launch (rho_conv_desc.gna_*) instead of a data-gradient launch plus an apply pass
            # that re-reads and re-writes it
            fuse_skip_dgrad=os.environ.get("RHO_FUSE_SKIP_DGRAD", "1") != "0",
            # read by the library at every conv query and launch (gemm1x1.h: k_gemm1x1 for the wide bf16 1x1x1 convs, 0 = k_conv);
            # recorded here so that a plan - its variant names and statistics rows - is rebuilt when the switch flips
            gemm1x1=os.environ.get("RHO_GEMM1X1", "1") != "0",
            # read by the library and latched at its first conv query (conv.hip: the compile-time 4 x 8 x 8 tile form of the bf16
            # 3x3x3 k_conv variants, 0 = the generic form); recorded here so that plans are keyed on it like the other knobs
            conv_geo=os.environ.get("RHO_CONV_GEO", "1") != "0")

    def _plan_signature(self) -> tuple:
        """Everything besides (shape, labels, mode) that is baked into a plan when it is built: the per-ResBlock ``use_checkpoint``
        flags (layers.py:153-199 semantics, honoured per block), the library's deterministic switch and the A/B environment knobs.
        A change of any of them selects (builds) another plan instead of silently replaying the old one."""
        ck = tuple(bool(b.use_checkpoint) for b in self._film_blocks)
        env = tuple(os.environ.get(k) for k in self._PLAN_ENV)
        # nn.Dropout is active iff the module is in training mode (with or without autograd): part of the key where p > 0
        drop = bool(self.model.training) if any(float(getattr(b, "dropout", 0.0) or 0.0) > 0.0 for b in self._film_blocks) else None
        return (ck, ops.deterministic(), env, drop)

    def drop_plans(self, train_only: bool = False) -> None:
        """Release cached plans (and their device buffers): all of them, or only the training plans."""
        self._plans = {k: v for k, v in self._plans.items() if train_only and not k[2]}
        self._last_train_plan = None

    def backward(self, dpred: Tensor, on_ready: Optional[Callable[[List[nn.Parameter]], None]] = None,
                 generation: Optional[int] = None) -> None:
        """Backward of the most recent ``forward(train=True)``: accumulates into ``p.grad`` of every
        parameter (allocated as zeros if missing).  ``on_ready(params)`` is called as groups of
        parameter gradients become final (used to overlap the data-parallel all-reduce).

        ``generation``: the value of ``_train_generation`` right after the forward this backward belongs to (UNetFunction
        remembers it).  The engine keeps the activations of ONE training forward - a plan's buffers are overwritten by the next
        forward of that shape, and another shape selects another plan - so a backward of an older forward cannot be computed
        and raises instead of returning the gradients of the wrong forward."""
        plan = self._last_train_plan
        if plan is None:
            raise hip.RhoHipError("backward() without a preceding forward(train=True)")
        if generation is not None and generation != self._train_generation:
            raise hip.RhoHipError(
                f"backward() of training forward #{generation}, but the most recent forward(train=True) of this engine is "
                f"#{self._train_generation}: the engine keeps the activations of the most recent training forward only - "
                "run each forward's backward before the next training forward (one forward over the concatenated batch, or "
                "forward / backward per micro-batch with gradient accumulation)")
        with torch.no_grad():
            plan.run_backward(dpred, on_ready)


class _Plan:
    """All buffers + launch closures for one input shape (forward, and backward when train=True)."""

    def __init__(self, eng: UNetEngine, xshape: Tuple[int, ...], has_y: bool, train: bool):
        self.eng, self.train, self.has_y = eng, train, has_y
        self.sw = eng._plan_switches()
        self.L = hip.lib()
        self.B, self.xshape = xshape[0], xshape
        self.ops: List[Callable[[int], int]] = []
        self.info: List[dict] = []     # per launch: kind, algorithmic flops / bytes (for bench roofline)
        self.keep: List[object] = []   # descriptors / tensors referenced by raw pointers
        self.tstats: Dict[int, Tuple[Tensor, int]] = {}   # conv output data_ptr -> (fused statistics buffer, tiles per sample)
        self.nodes: List[dict] = []                # one per differentiable step of the forward, in forward order
        self.fwd_descs: List[object] = []          # rho_conv_desc of every forward / data-gradient launch (variants())
        self.wgrad_descs: List[tuple] = []         # (forward-shaped descriptor, dY row width) of every weight-gradient launch
        self.cond_src = None
        # dropout (nn.Dropout(p) of ResBlock.out_layers, unet_v2.py:239; active iff the model is in training mode): Philox masks in the
        # materialising pass, regenerated in backward from (seed of the block, a device counter advanced once per forward)
        self.drop_active = bool(eng.model.training) and any(float(getattr(b, "dropout", 0.0) or 0.0) > 0.0 for b in eng._film_blocks)
        self.drop_ctr = torch.zeros(1, dtype=torch.int64, device=eng.device) if self.drop_active else None
        self.drop_delta = 0
        self.drop_nodes: List[dict] = []          # (test aid) block, p, seed, activated-tensor shape of every dropout site
        self.bwd: List[Callable[[int], int]] = []
        self.bwd_info: List[dict] = []
        self.bwd_marks: List[Tuple[int, List[nn.Parameter]]] = []   # after bwd[:i] these parameters' gradients are final
        ForwardBuilder(self).build()        # -> ops, info, nodes, the embedding buffers, x_in, x_cl, out
        if train:
            BackwardBuilder(self).build()   # -> bwd, bwd_info, bwd_marks, dpred_in, the gradient arena and pool
        # k-split of the small-grid 2-D / 1-D launches (rho_conv_desc.ws): one workspace per plan, shared by its ordered launches
        ws = ops.attach_conv_workspace(self.fwd_descs, eng.device)
        if ws is not None:
            self.keep.append(ws)

    def nbytes(self) -> int:
        """Device bytes this plan owns (forward buffers kept for its lifetime + the backward pool)."""
        seen, tot = set(), 0
        for t in self.keep:
            if torch.is_tensor(t) and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                tot += t.numel() * t.element_size()
        return tot + int(getattr(self, "pool_bytes", 0))

    def variants(self) -> List[str]:
        """Names of the k_conv / k_wgrad instantiations this plan launches (rho_conv_variant / rho_conv_wgrad_variant)."""
        out = [ops.conv_variant(d) for d in self.fwd_descs]
        out += [ops.conv_wgrad_variant(d, w_) for d, w_ in self.wgrad_descs]
        return out

    # ------------------------------------------------------------------ execution
    def run(self, x: Tensor, timesteps: Optional[Tensor], y: Optional[Tensor], t_scalar_dev: Optional[Tensor],
            keep: Optional[Tensor] = None) -> Tensor:
        """``keep`` (training plans only, see UNetEngine.set_cond_keep): [B] mask, a sample whose entry is 0 loses its condition."""
        eng = self.eng
        m = eng.model
        if x.data_ptr() != self.x_in.data_ptr():
            self.x_in.copy_(x)
        te0, te2 = m.time_embed[0], m.time_embed[2]
        self.cond_src = None
        self.cond_dev = None
        if keep is not None:
            if self.cond is None:
                raise hip.RhoHipError("a label keep mask was set, but this forward has no labels to drop")
            if keep.numel() != self.B:
                raise hip.RhoHipError(f"the label keep mask has {keep.numel()} entries for a batch of {self.B}")
            keep = (keep.reshape(-1) != 0).to(device=self.cond.device, dtype=torch.uint8)
        if self.cond is not None:
            # label handling of unet_v2.py:702-719
            if y.dim() == 2 and tuple(y.shape) == tuple(self.emb.shape):
                self.cond.copy_(y.to(self.cond.device))
                if keep is not None:
                    ops.cond_drop(self.cond, None, keep)       # rows of the copy: the caller's tensor stays as it is
            else:
                if y.dim() == 1:
                    assert y.shape == (x.shape[0],)
                else:
                    assert y.shape[0] == self.emb.shape[0]
                cd = eng.cond_device_tables()
                if cd is not None:
                    # MultiEmbeddings on the device: category lookup by exact equality + row sum, no host synchronisation
                    yf = y.to(device=self.cond.device, dtype=torch.float32).contiguous()
                    if yf.dim() == 2 and yf.shape[1] != cd["nkeys"]:
                        raise hip.RhoHipError(f"labels have {yf.shape[1]} columns, the parameter space has {cd['nkeys']} keys")
                    self.keep_y = yf
                    check(self.L.rho_multi_embed(ptr(yf), 1 if yf.dim() == 1 else yf.shape[1], ptr(cd["space"]), ptr(cd["key_off"]),
                                                 ptr(cd["tables"]), cd["nkeys"], self.B, self.cond.shape[1], ptr(self.cond),
                                                 ptr(self.cond_idx), ptr(eng.err_flag()), hip.stream()), "rho_multi_embed")
                    if keep is not None:
                        # zero row + category -1: rho_multi_embed_bwd skips the sample, its table rows get no gradient
                        ops.cond_drop(self.cond, self.cond_idx, keep, cd["nkeys"])
                    self.cond_dev = cd
                else:
                    with (torch.enable_grad() if self.train else torch.no_grad()):
                        c = m.cond_fn(y)          # a user-supplied cond_fn module (not MultiEmbeddings): evaluated as given
                        if keep is not None:
                            c = c * keep.to(c.dtype).reshape((-1,) + (1,) * (c.dim() - 1))      # under autograd: no gradient from a dropped row
                    self.cond_src = c if (self.train and c.requires_grad) else None
                    self.cond.copy_(c.detach())
        # timestep embedding: sinusoid of t (any integer) -> Linear -> SiLU -> Linear (+ cond), one launch
        if t_scalar_dev is not None:
            tptr, tsptr = None, ptr(t_scalar_dev)
        else:
            hip.require_gpu(timesteps, "timesteps")
            self.t_in.copy_(timesteps.reshape(-1))
            tptr, tsptr = ptr(self.t_in), None
        check(self.L.rho_timestep_embed(ptr(eng.omega()), tptr, tsptr, ptr(te0.weight), ptr(te0.bias), ptr(te2.weight), ptr(te2.bias),
                                        ptr(self.cond), ptr(self.sin_in), ptr(self.emb_h), ptr(self.emb), self.B, eng.mc,
                                        self.emb.shape[1], eng.act, hip.stream()), "rho_timestep_embed")
        s = hip.stream()
        if self.drop_active:
            # a fresh stretch of every block's Philox stream for this forward (and its backward, which reads the same counter)
            check(self.L.rho_step_advance(None, ptr(self.drop_ctr), self.drop_delta, s), "rho_step_advance")
        for op in self.ops:
            rc = op(s)
            if rc != 0:
                check(rc, "UNet plan launch")
        return self.out

    def run_backward(self, dpred: Tensor, on_ready=None) -> None:
        eng = self.eng
        for p_ in eng.model.parameters():
            if p_.grad is None:
                p_.grad = torch.zeros_like(p_)
        self.dpred_in.copy_(dpred.reshape(self.dpred_in.shape))
        s = hip.stream()
        marks: Dict[int, list] = {}
        for i, ps in self.bwd_marks:
            marks.setdefault(i, []).extend(ps)
        for i, op in enumerate(self.bwd):
            rc = op(s)
            if rc != 0:
                check(rc, "UNet backward plan launch")
            if on_ready is not None and (i + 1) in marks:
                on_ready(marks[i + 1])
        if self.cond_dev is not None:
            cd = self.cond_dev
            gsig = tuple(w.grad.data_ptr() for w in cd["weights"])
            if getattr(self, "_gp_sig", None) != gsig:              # gradient storage is stable under the arena optimizer
                self._gp = torch.tensor(list(gsig), dtype=torch.int64, device=self.demb.device)
                self._gp_sig = gsig
            gp = self._gp
            check(self.L.rho_multi_embed_bwd(ptr(self.demb), ptr(self.cond_idx), ptr(gp), cd["nkeys"], self.B, self.demb.shape[1], s),
                  "rho_multi_embed_bwd")
        elif self.cond_src is not None:
            with torch.enable_grad():
                self.cond_src.backward(self.demb)      # a user-supplied cond_fn module
        if on_ready is not None:
            on_ready([])

    def profile(self, repeats: int = 3, backward: bool = False) -> List[dict]:
        """Replay the plan with a HIP event pair around every launch (events recorded on the stream the
        kernels are launched on) and return per-launch dicts {kind, flops, bytes, ms} (ms = mean over
        repeats).  Inputs are whatever the buffers currently hold."""
        s = hip.stream()
        lst, infos = (self.bwd, self.bwd_info) if backward else (self.ops, self.info)
        tot = [0.0] * len(lst)
        for _ in range(repeats):
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in lst]
            for op, (e0, e1) in zip(lst, evs):
                e0.record()
                rc = op(s)
                e1.record()
                if rc != 0:
                    check(rc, "UNet plan launch (profile)")
            torch.cuda.synchronize()
            for i, (e0, e1) in enumerate(evs):
                tot[i] += e0.elapsed_time(e1)
        return [dict(info, ms=tot[i] / repeats) for i, info in enumerate(infos)]
