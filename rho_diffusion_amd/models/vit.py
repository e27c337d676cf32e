"""VisionTransformer backbone (reference: rho_diffusion/models/vit.py:32-372) on the HIP engine.

``PatchEmbedding``, ``AttentionBlock`` and ``VisionTransformer`` keep the reference's constructor signatures, defaults and
``state_dict`` layout (``patch_embedder.conv_shaper``, ``transformer_blocks.N.{norm_1, norm_2, attention_layer, linear_block.0 / .3,
time_transform.1}``, ``output_projection``, ``output_conv``, ``pos_embedding.1``), so reference checkpoints load.  The parameters
live in stock ``nn`` modules that are never called: forward and backward are sequences of HIP launches.

Token rows ``[B, N, E]`` are the engine's channels-last layout with N positions and E channels, so
  * every ``nn.Linear`` over tokens, the kernel = stride = p convolution of the patch embedding (vit.py:73-78) and the ConvTranspose of
    the output (vit.py:282-288) are 1x1x1 launches of ``rho_conv_nd_fwd`` (forward, data gradient) and ``rho_conv_nd_wgrad``;
  * the q / k / v projection is ONE launch whose split output is the ``qk`` channels-last + ``vt`` channel-major pair that
    ``rho_attention_fwd`` / ``rho_attention_bwd`` read (they scale by ch^-0.5 as ``nn.MultiheadAttention`` does);
  * LayerNorm (+ the time-embedding add), the patch gather / scatter, the activation and the positional add are csrc/vit.hip;
  * the ``[N, E]`` positional table and the ``[B, E]`` time transforms run on ``rho_timestep_embed`` / ``rho_linear`` /
    ``rho_linear_bwd``.

Launches per block, forward: layernorm(+t), qkv conv, attention, out_proj conv (+ residual), layernorm, linear conv, activation,
linear conv (+ residual) - 8, plus 2 small ones for the time transform (rho_linear, rho_bias_act; the sinusoid of t is evaluated
once per forward and shared by the blocks).  The reference's data flow is kept as it is, including the
residual of the attention being ``norm_1(x + t_embed) + attn(...)`` rather than ``x + attn(...)`` (vit.py:178-184).

Differences to the reference: ``forward(input_data, t, y=None)`` accepts the third argument the pipelines pass but
``y`` must be None; a standalone ``AttentionBlock.forward`` returns ``attn_weights`` None (the flash kernels never materialise the
averaged weights); what the kernels do not cover is refused at construction, naming the reference lines; ``dropout > 0`` runs in
eval mode (identity) and raises in training mode (vit.py:149-154: ``nn.MultiheadAttention`` drops attention probabilities).
"""
from __future__ import annotations

import math
from collections.abc import Mapping
from typing import Optional, Union

import torch
from torch import nn

from ..registry import registry
from .common import SinusoidalPositionEmbedding

__all__ = ["PatchEmbedding", "AttentionBlock", "VisionTransformer"]

_HEAD_WIDTHS = (16, 32, 64, 128, 256)
_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "f32": torch.float32}


def _act_code(activation) -> int:
    """Activation code of the C ABI for a registry name / class / instance; anything else is refused (vit.py:157,289)."""
    from ..engine import ops
    cls = activation
    if isinstance(activation, str):
        cls = registry.get("activations", activation)
    if isinstance(cls, nn.Module):
        cls = type(cls)
    name = getattr(cls, "__name__", str(cls))
    if name not in ops.ACT_CODES or name == "Identity" or (isinstance(activation, nn.GELU) and activation.approximate != "none"):
        raise NotImplementedError(f"VisionTransformer (vit.py:157,289): the HIP path implements the activations "
                                  f"{sorted(k for k in ops.ACT_CODES if k != 'Identity')}, got {activation!r}")
    return ops.ACT_CODES[name]


def _act_module(activation) -> nn.Module:
    cls = registry.get("activations", activation) if isinstance(activation, str) else activation
    return cls if isinstance(cls, nn.Module) else cls()


def _check_norm_width(embed_dim: int) -> None:
    from .. import hip
    cap = int(hip.lib().rho_layernorm_max_dim())
    if embed_dim > cap:
        raise NotImplementedError(f"AttentionBlock (vit.py:145-146): the LayerNorm kernels hold a row of at most {cap} elements in "
                                  f"registers, got embed_dim {embed_dim}")


def _c32(v: int) -> int:
    return ((int(v) + 31) // 32) * 32


def _grad_of(p: nn.Parameter) -> torch.Tensor:
    """``p.grad`` as it is NOW (HipAdamW re-homes it into its arena after the first step): resolved at launch time.  Only for a
    parameter that requires grad: a frozen one keeps ``.grad`` None (``_wants`` / ``_grad_or_scratch``)."""
    assert p.requires_grad
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def _wants(p: Optional[nn.Parameter]) -> bool:
    return p is not None and p.requires_grad


def _grad_or_scratch(p: nn.Parameter) -> torch.Tensor:
    """Target of a kernel that writes this parameter's gradient next to other results (LayerNorm's dgamma / dbeta): ``p.grad``, or
    for a frozen parameter a scratch tensor that is dropped."""
    return _grad_of(p) if p.requires_grad else torch.zeros_like(p)


class _Gemm:
    """The GEMM forms of one parameter viewed as W [P, Q]: y = x W^T (an nn.Linear / kernel = stride convolution) or, ``transposed``,
    y = x W (a ConvTranspose with kernel = stride).  Prepared layouts are cached until the parameter's storage or version counter
    moves.  The parameters are looked up on their module at every use, never held: ``load_state_dict(..., assign=True)`` and
    ``module.weight = nn.Parameter(...)`` put ANOTHER object there, and a held one would go on serving the old weights and
    collecting the gradients."""

    def __init__(self, owner: nn.Module, wname: str, P: int, Q: int, bname: Optional[str] = None, transposed: bool = False):
        self._owner, self._wname, self._bname = owner, wname, bname
        self.P, self.Q, self.transposed = int(P), int(Q), transposed
        self._key = None
        self._zero = {}

    @property
    def weight(self) -> nn.Parameter:
        return getattr(self._owner, self._wname)

    @property
    def bias(self) -> Optional[nn.Parameter]:
        return getattr(self._owner, self._bname) if self._bname is not None else None

    def _w2d(self) -> torch.Tensor:
        return self.weight.detach().view(self.P, self.Q)

    def prepared(self, dt):
        from ..engine import ops
        w = self._w2d()
        key = (w.data_ptr(), self.weight._version, dt)
        if self._key != key:
            P32, Q32 = _c32(self.P), _c32(self.Q)
            self.A = ops.prep_conv_weight(w, dt, coutp=P32, cinp=Q32)                       # [1, P32, Q32]: rows P, contraction over Q
            self.Bm = ops.prep_conv_weight_dgrad(w, dt, out=torch.empty(1, Q32, P32, dtype=dt, device=w.device))   # rows Q, contraction over P
            self._key = key
        return (self.Bm, self.A) if self.transposed else (self.A, self.Bm)

    def zero_bias(self, n: int, dev) -> torch.Tensor:
        z = self._zero.get((n, dev))
        if z is None:
            z = self._zero[(n, dev)] = torch.zeros(n, dtype=torch.float32, device=dev)
        return z

    @property
    def out_w(self) -> int:
        return _c32(self.Q if self.transposed else self.P)

    @property
    def in_w(self) -> int:
        return _c32(self.P if self.transposed else self.Q)

    def fwd(self, x, res=None, split=None):
        """x channels-last [B, 1, 1, N, in_w] -> [B, 1, 1, N, out_w] (+ res); ``split``: (channels-last, channel-major) pair."""
        from ..engine import ops
        wf, _ = self.prepared(x.dtype)
        b = self.bias.detach() if self.bias is not None else self.zero_bias(self.out_w, x.device)
        y, y2 = ops.conv(x, None, wf, b, kernel=(1, 1, 1), cout=self.out_w, split=split, res=res)
        return y if split is None else (y, y2)

    def dgrad(self, dy, res=None):
        from ..engine import ops
        _, wd = self.prepared(dy.dtype)
        y, _ = ops.conv(dy, None, wd, self.zero_bias(self.in_w, dy.device), kernel=(1, 1, 1), cout=self.in_w, res=res)
        return y

    def wgrad(self, x, dy) -> None:
        """Accumulates the weight (and bias) gradient of y = fwd(x) into ``p.grad``; nothing is launched for frozen parameters."""
        from .. import hip
        from ..engine import ops
        want_b = self.bias is not None and not self.transposed and self.bias.requires_grad
        if not (self.weight.requires_grad or want_b):
            return
        a, b = (dy, x) if self.transposed else (x, dy)                       # dw[P, Q] = sum_pos b[pos, P] a[pos, Q]
        P32, Q32 = _c32(self.P), _c32(self.Q)
        wA = self.prepared(x.dtype)[1 if self.transposed else 0]
        desc = ops.make_conv_desc(a, None, wA, self.zero_bias(P32, x.device), kernel=(1, 1, 1), cout=P32, split=P32, y=b, y2=None)
        dw = torch.zeros(1, P32, Q32, dtype=torch.float32, device=x.device)
        db = torch.zeros(P32, dtype=torch.float32, device=x.device) if want_b else None
        ops.conv_wgrad(desc, b, dw, db)
        if self.weight.requires_grad:
            g = _grad_of(self.weight)
            hip.check(hip.lib().rho_wgrad_finalize(hip.ptr(dw), hip.ptr(g), self.P, self.Q, 1, P32, Q32, None, 1, hip.stream()),
                      "rho_wgrad_finalize")
        if want_b:
            gb = _grad_of(self.bias)
            hip.check(hip.lib().rho_add_inplace(hip.ptr(gb), hip.ptr(db), hip.RHO_F32, self.P, hip.stream()), "rho_add_inplace")


def _small_linear_bwd(dz, x, lin: nn.Linear) -> None:
    """Parameter gradients of z = lin(x) for the [B, E] / [N, E] sized host-side pieces, accumulated into ``p.grad`` (a frozen
    parameter gets none; with both frozen nothing is launched)."""
    from ..engine import ops
    dw = _grad_of(lin.weight) if lin.weight.requires_grad else None
    db = _grad_of(lin.bias) if _wants(lin.bias) else None
    if dw is None and db is None:
        return
    ops.linear_bwd(dz, x, lin.weight.detach(), dw, db, None, acc_params=True)


class PatchEmbedding(nn.Module):
    """vit.py:32-129: a kernel = stride = patch_size convolution, tokens in ``(h w d)`` order.  Holds the parameters; the launches are
    issued by ``VisionTransformer`` (``forward`` runs the same launches for a standalone call and returns float32 [B, N, E])."""

    def __init__(self, num_channels: int, patch_size: int, embedding_dim: int, data_dims: int) -> None:
        super().__init__()
        assert 3 >= data_dims > 0, "data_dims must be between 1 and 3 for convolution."
        self.num_channels, self.patch_size, self.embedding_dim, self.data_dims = num_channels, patch_size, embedding_dim, data_dims
        if embedding_dim % 32:
            raise NotImplementedError(f"PatchEmbedding (vit.py:73-78): the HIP path needs embedding_dim % 32 == 0, got {embedding_dim}")
        self._conv_type = registry.get("nn", f"Conv{data_dims}d")
        self.conv_shaper = self._conv_type(num_channels, embedding_dim, kernel_size=patch_size, stride=patch_size)
        self.stored_shape = None
        self._gemm = _Gemm(self.conv_shaper, "weight", embedding_dim, num_channels * patch_size ** data_dims, "bias")

    def tokens(self, data: torch.Tensor, dt) -> torch.Tensor:
        """float32 [B, C, *spatial] -> embedded tokens, channels-last [B, 1, 1, N, E] in ``dt`` (+ the patch operand for the backward)."""
        from ..engine import ops
        sp = tuple(data.shape[2:])
        if len(sp) != self.data_dims or data.shape[1] != self.num_channels or any(s % self.patch_size for s in sp):
            raise ValueError(f"PatchEmbedding (vit.py:123-129): expected [B, {self.num_channels}, *spatial] with {self.data_dims} spatial "
                             f"axes divisible by patch_size {self.patch_size}, got {tuple(data.shape)}")
        self.stored_shape = tuple(s // self.patch_size for s in sp)
        pt = ops.patchify(data.float().contiguous(), self.patch_size, dt)
        pt5 = pt.view(pt.shape[0], 1, 1, pt.shape[1], pt.shape[2])
        return self._gemm.fwd(pt5), pt5

    def forward(self, data: torch.Tensor) -> torch.Tensor:
        from .. import hip
        hip.require_gpu(data, "data")
        y, _ = self.tokens(data, torch.float32)
        return y.view(y.shape[0], y.shape[3], y.shape[4])


class AttentionBlock(nn.Module):
    """vit.py:132-185.  ``run`` / ``run_bwd`` are the HIP launch sequences; a standalone ``forward(data, t)`` runs them in float32
    and returns ``{"output": ..., "attn_weights": None}``."""

    def __init__(self, embed_dim: int, hidden_dim: int, num_heads: int, dropout: float = 0.0, activation: Union[str, nn.Module] = "GELU",
                 time_dim: int = 128, **attn_kwargs):
        super().__init__()
        _check_norm_width(embed_dim)
        if embed_dim % 32 or hidden_dim % 32:
            raise NotImplementedError(f"AttentionBlock (vit.py:145-164): the HIP path needs embed_dim and hidden_dim to be multiples of "
                                      f"32, got {embed_dim} / {hidden_dim}")
        if num_heads <= 0 or embed_dim % num_heads or embed_dim // num_heads not in _HEAD_WIDTHS:
            raise NotImplementedError(f"AttentionBlock (vit.py:149-154): the attention kernels take head widths {_HEAD_WIDTHS}, got "
                                      f"embed_dim / num_heads = {embed_dim} / {num_heads}")
        if dict(attn_kwargs) not in ({}, {"batch_first": True}):
            raise NotImplementedError(f"AttentionBlock (vit.py:148-154): attention kwargs other than batch_first=True are not built, "
                                      f"got {dict(attn_kwargs)}")
        self.act_code = _act_code(activation)
        self.embed_dim, self.hidden_dim, self.num_heads, self.dropout, self.time_dim = embed_dim, hidden_dim, num_heads, float(dropout), time_dim
        self.norm_1 = nn.LayerNorm(embed_dim)
        self.norm_2 = nn.LayerNorm(embed_dim)
        self.attention_layer = nn.MultiheadAttention(embed_dim, num_heads, dropout, batch_first=True)
        self.linear_block = nn.Sequential(nn.Linear(embed_dim, hidden_dim), _act_module(activation), nn.Dropout(dropout),
                                          nn.Linear(hidden_dim, embed_dim), nn.Dropout(dropout))
        self.time_transform = nn.Sequential(SinusoidalPositionEmbedding(time_dim), nn.Linear(time_dim, embed_dim, bias=False),
                                            _act_module(activation))
        at = self.attention_layer
        self._qkv = _Gemm(at, "in_proj_weight", 3 * embed_dim, embed_dim, "in_proj_bias")
        self._proj = _Gemm(at.out_proj, "weight", embed_dim, embed_dim, "bias")
        self._lin1 = _Gemm(self.linear_block[0], "weight", hidden_dim, embed_dim, "bias")
        self._lin2 = _Gemm(self.linear_block[3], "weight", embed_dim, hidden_dim, "bias")

    def _check_dropout(self):
        if self.training and self.dropout > 0:
            raise NotImplementedError("AttentionBlock (vit.py:149-154,161,163): a training-mode forward with dropout > 0 is not built - "
                                      "nn.MultiheadAttention drops attention probabilities and the flash attention kernels do not; "
                                      "use dropout=0.0 or eval()")

    def run(self, x, pe, keep: bool):
        """x channels-last [B, 1, 1, N, E]; pe float32 [B, time_dim] (the sinusoid of t); returns (output, saved-for-backward)."""
        from ..engine import ops
        self._check_dropout()
        B, N, E = x.shape[0], x.shape[3], x.shape[4]
        act = self.act_code
        tz = ops.linear(pe, self.time_transform[1].weight.detach(), None)                               # vit.py:175
        temb = ops.bias_act(tz, act)
        n1, st1 = ops.layernorm(x, self.norm_1.weight.detach(), self.norm_1.bias.detach(), add=temb)     # :176-178
        qk, vt = self._qkv.fwd(n1, split=2 * E)                                                          # :179 (in_proj)
        lse = torch.empty(B, self.num_heads, N, dtype=torch.float32, device=x.device) if keep else None
        ao = ops.attention(qk.view(B, N, 2 * E), vt, self.num_heads, lse=lse)
        ao5 = ao.view(B, 1, 1, N, E)
        ar = self._proj.fwd(ao5, res=n1)                                                                 # :181 norm_data + attn_o
        n2, st2 = ops.layernorm(ar, self.norm_2.weight.detach(), self.norm_2.bias.detach())              # :182
        z1 = self._lin1.fwd(n2)
        a1 = ops.bias_act(z1, act)
        out = self._lin2.fwd(a1, res=ar)                                                                 # :184
        saved = dict(x=x, pe=pe, tz=tz, temb=temb, n1=n1, st1=st1, qk=qk, vt=vt, lse=lse, ao=ao5, ar=ar, st2=st2, n2=n2, z1=z1,
                     a1=a1) if keep else None
        return out, saved

    def run_bwd(self, dout, s):
        """dout: gradient of ``run``'s output (consumed: it is accumulated into); returns the gradient of ``x``."""
        from ..engine import ops
        B, N, E = s["x"].shape[0], s["x"].shape[3], s["x"].shape[4]
        act = self.act_code
        # out = ar + lin2(act(lin1(norm_2(ar))))
        self._lin2.wgrad(s["a1"], dout)
        da1 = self._lin2.dgrad(dout)
        dz1 = ops.bias_act_bwd(s["z1"], da1, act)
        self._lin1.wgrad(s["n2"], dz1)
        dn2 = self._lin1.dgrad(dz1)
        n2 = self.norm_2
        ops.layernorm_bwd(dn2, s["ar"], s["st2"], n2.weight.detach(), _grad_or_scratch(n2.weight), _grad_or_scratch(n2.bias), dx=dout,
                          acc_dx=True, acc_params=True)
        dar = dout                                                                                        # d attn_residual
        # ar = n1 + out_proj(attention(qkv(n1)))
        self._proj.wgrad(s["ao"], dar)
        dao = self._proj.dgrad(dar)
        dqkv = ops.attention_bwd(s["qk"].view(B, N, 2 * E), s["vt"], s["ao"].view(B, N, E), dao.view(B, N, E), s["lse"], self.num_heads)
        dqkv5 = dqkv.view(B, 1, 1, N, 3 * E)
        self._qkv.wgrad(s["n1"], dqkv5)
        dn1 = self._qkv.dgrad(dqkv5, res=dar)
        # n1 = norm_1(x + t_embed): x reaches the output through the norm only (vit.py:178-184)
        n1 = self.norm_1
        dx, dtemb = ops.layernorm_bwd(dn1, s["x"], s["st1"], n1.weight.detach(), _grad_or_scratch(n1.weight), _grad_or_scratch(n1.bias),
                                      add=s["temb"], acc_params=True)
        if self.time_transform[1].weight.requires_grad:
            dtz = ops.bias_act_bwd(s["tz"], dtemb, act)
            _small_linear_bwd(dtz, s["pe"], self.time_transform[1])
        return dx

    def forward(self, data: torch.Tensor, t: torch.Tensor) -> dict:
        from .. import hip
        hip.require_gpu(data, "data")
        B, N, E = data.shape
        with torch.no_grad():
            pe = self.time_transform[0](t)
            out, _ = self.run(data.detach().float().contiguous().view(B, 1, 1, N, E), pe, keep=False)
        return {"output": out.view(B, N, E), "attn_weights": None}


class _ViTFunction(torch.autograd.Function):
    """pred = VisionTransformer(x, t).  ``anchor`` is a parameter that requires grad: it only makes autograd call ``backward``;
    parameter gradients are written by the kernels into ``p.grad`` (as autograd.UNetFunction does)."""

    @staticmethod
    def forward(ctx, x, anchor, model, t):
        pred, saved = model._forward_impl(x, t, keep=True)
        ctx.model, ctx.saved = model, saved
        ctx.want_dx = x.requires_grad
        return pred

    @staticmethod
    def backward(ctx, dout):
        saved, ctx.saved = ctx.saved, None
        if saved is None:
            raise RuntimeError("VisionTransformer: backward through the same forward twice is not supported")
        dx = ctx.model._backward_impl(dout.contiguous().float(), saved, ctx.want_dx)
        return dx, None, None, None


@registry.register_model("VisionTransformer")
class VisionTransformer(nn.Module):
    """vit.py:188-372.  Extra (optional) kwarg ``compute_dtype``: "bf16" (default) or "fp32", as on ``UNet``."""

    def __init__(self, patch_size: int, input_shapes: list, num_channels: int, embedding_dim: int, hidden_dim: int,
                 activation: Union[str, nn.Module], transformer_depth: int = 8, pos_embedding_dim: int = 128, time_embedding_dim: int = 128,
                 max_seq_length: int = 20_000, dropout: float = 0.2, num_heads: int = 16, attention_kwargs: Optional[Mapping] = {},
                 compute_dtype="bf16") -> None:
        super().__init__()
        data_dims = len(input_shapes)
        if not 1 <= data_dims <= 3:
            raise NotImplementedError(f"VisionTransformer (vit.py:256-263): 1-D / 2-D / 3-D data only, got input_shapes {input_shapes}")
        if any(int(s) % int(patch_size) for s in input_shapes):
            raise NotImplementedError(f"VisionTransformer (vit.py:73-78,282-288): every entry of input_shapes {list(input_shapes)} must be "
                                      f"divisible by patch_size {patch_size} (the strided convolution would drop the remainder and the "
                                      f"output would not have the input's shape)")
        if embedding_dim % 32 or hidden_dim % 32:
            raise NotImplementedError(f"VisionTransformer (vit.py:258-279): the HIP path needs embedding_dim and hidden_dim to be "
                                      f"multiples of 32, got {embedding_dim} / {hidden_dim}")
        if pos_embedding_dim % 2 or time_embedding_dim % 2 or max(pos_embedding_dim, time_embedding_dim) > 2048:
            raise NotImplementedError("VisionTransformer (vit.py:166,292): sinusoid widths must be even and at most 2048")
        _check_norm_width(embedding_dim)
        self.act_code = _act_code(activation)
        self.input_shapes = list(input_shapes)
        self.max_seq_length = max_seq_length
        self.patch_embedder = PatchEmbedding(num_channels, patch_size, embedding_dim, data_dims)
        self.transformer_blocks = nn.ModuleList([
            AttentionBlock(embedding_dim, hidden_dim, num_heads, dropout, activation, time_embedding_dim, **dict(attention_kwargs or {}))
            for _ in range(transformer_depth)])
        self.output_projection = nn.Linear(embedding_dim, hidden_dim, bias=False)
        conv_type = registry.get("nn", f"ConvTranspose{data_dims}d")
        self.output_conv = conv_type(hidden_dim, num_channels, kernel_size=patch_size, stride=patch_size)
        self.pos_embedding = nn.Sequential(SinusoidalPositionEmbedding(pos_embedding_dim), nn.Linear(pos_embedding_dim, embedding_dim),
                                           _act_module(activation))
        if compute_dtype not in _DTYPES and compute_dtype not in _DTYPES.values():
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        self.compute_dtype = _DTYPES.get(compute_dtype, compute_dtype)
        self.num_channels, self.embedding_dim, self.hidden_dim = num_channels, embedding_dim, hidden_dim
        self._oproj = _Gemm(self.output_projection, "weight", hidden_dim, embedding_dim)
        self._oconv = _Gemm(self.output_conv, "weight", hidden_dim, num_channels * patch_size ** data_dims, transposed=True)
        self._pos_cache = None

    # ------------------------------------------------------------------ reference properties
    @property
    def input_shape_dim_names(self):
        return [key for _, key in zip(self.input_shapes, ["j", "k", "l"])]

    @property
    def patch_size(self) -> int:
        return self.patch_embedder.patch_size

    @property
    def data_dims(self) -> int:
        return self.patch_embedder.data_dims

    @property
    def stored_shape(self):
        return self.patch_embedder.stored_shape

    @property
    def stored_shape_ein(self):
        return {key: value for key, value in zip(["j", "k", "l"], self.stored_shape)}

    # ------------------------------------------------------------------ host-side pieces
    def _pos_table(self, n: int, dev, keep: bool):
        """act(Linear(sinusoid(arange(N)))) float32 [N, E] (vit.py:349-351); cached on the no-grad path (``keep`` False, whatever
        train() / eval() says) until the version counter or the storage of its weight or bias moves."""
        from ..engine import ops
        lin = self.pos_embedding[1]
        key = (n, str(dev), lin.weight._version, lin.bias._version, lin.weight.data_ptr(), lin.bias.data_ptr())
        if not keep and self._pos_cache is not None and self._pos_cache[0] == key:
            return self._pos_cache[1], None
        idx = torch.arange(n, device=dev, dtype=torch.int64)
        pe = self.pos_embedding[0](idx)
        z = ops.linear(pe, lin.weight.detach(), lin.bias.detach())
        pos = ops.bias_act(z, self.act_code)
        if not keep:
            self._pos_cache = (key, pos)
        return pos, (pe, z)

    # ------------------------------------------------------------------ launch sequences
    def _forward_impl(self, x: torch.Tensor, t: torch.Tensor, keep: bool):
        from ..engine import ops
        dt = self.compute_dtype
        emb, pt5 = self.patch_embedder.tokens(x.detach(), dt)                                 # vit.py:347
        B, N, E = emb.shape[0], emb.shape[3], emb.shape[4]
        pos, pos_saved = self._pos_table(N, x.device, keep)
        ops.pos_add(emb, pos)                                                                # :353
        tt = t.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
        if tt.numel() != B:
            raise ValueError(f"VisionTransformer: t must hold one timestep per sample ({B}), got {tuple(t.shape)}")
        h = emb
        blocks = []
        pes = {}
        for blk in self.transformer_blocks:                                                  # :354-356
            pe = pes.get(blk.time_dim)
            if pe is None:
                pe = pes[blk.time_dim] = blk.time_transform[0](tt)
            h, s = blk.run(h, pe, keep)
            blocks.append(s)
        hp = self._oproj.fwd(h)                                                              # :360
        tk = self._oconv.fwd(hp)                                                             # :371 as a GEMM ...
        pred = ops.unpatchify(tk.view(B, N, tk.shape[4]), tuple(x.shape), self.patch_size, bias=self.output_conv.bias.detach())  # ... + scatter
        saved = dict(pt5=pt5, pos=pos_saved, blocks=blocks, h=h, hp=hp, shape=tuple(x.shape)) if keep else None
        return pred, saved

    def _backward_impl(self, dpred: torch.Tensor, s: dict, want_dx: bool):
        from ..engine import ops
        dt = self.compute_dtype
        B = s["shape"][0]
        dtk = ops.patchify(dpred, self.patch_size, dt, dbias=_grad_or_scratch(self.output_conv.bias), acc_dbias=True)
        dtk5 = dtk.view(B, 1, 1, dtk.shape[1], dtk.shape[2])
        self._oconv.wgrad(s["hp"], dtk5)
        dhp = self._oconv.dgrad(dtk5)
        self._oproj.wgrad(s["h"], dhp)
        dh = self._oproj.dgrad(dhp)
        for blk, sb in zip(reversed(self.transformer_blocks), reversed(s["blocks"])):
            dh = blk.run_bwd(dh, sb)
        # embedded = conv_shaper(patches) + pos
        if any(p.requires_grad for p in self.pos_embedding[1].parameters()):
            pe, z = s["pos"]
            dpos = ops.pos_add_bwd(dh.view(B, dh.shape[3], dh.shape[4]))
            dz = ops.bias_act_bwd(z, dpos, self.act_code)
            _small_linear_bwd(dz, pe, self.pos_embedding[1])
        g = self.patch_embedder._gemm
        g.wgrad(s["pt5"], dh)
        if not want_dx:
            return None
        dpt = g.dgrad(dh)
        return ops.unpatchify(dpt.view(B, dpt.shape[3], dpt.shape[4]), s["shape"], self.patch_size)

    def forward(self, input_data: torch.Tensor, t: torch.Tensor, y=None) -> torch.Tensor:
        """vit.py:319-372; returns float32 with the input's shape.  ``y`` must be None: the reference model is unconditional, the slot
        only lets the pipelines (which always pass three arguments) drive it."""
        from .. import hip
        if y is not None:
            raise NotImplementedError("VisionTransformer.forward (vit.py:319): the model is unconditional - y must be None")
        hip.require_gpu(input_data, "input_data")
        if tuple(input_data.shape[2:]) != tuple(self.input_shapes) or input_data.shape[1] != self.num_channels:
            raise ValueError(f"VisionTransformer: expected [B, {self.num_channels}, {', '.join(map(str, self.input_shapes))}], got "
                             f"{tuple(input_data.shape)}")
        params = [p for p in self.parameters() if p.requires_grad]
        if torch.is_grad_enabled() and (params or input_data.requires_grad):
            x = input_data if input_data.dtype == torch.float32 else input_data.float()
            return _ViTFunction.apply(x, params[0] if params else None, self, t)
        pred, _ = self._forward_impl(input_data, t, keep=False)
        return pred
