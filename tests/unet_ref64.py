"""Dtype-generic restatement of the UNetv2 forward of ``oracle/ref_torch.py`` (TEST INFRASTRUCTURE).

``oracle.ref_torch.unet_forward`` is float32 by construction: GroupNorm32 and the softmax cast to ``.float()``, the sinusoid is built in
the default dtype.  This module states the same layer mathematics - GroupNorm32, ResBlock with both embedding forms and up / down,
attention in both orders, pool / nearest, stem, head, timestep and label embeddings - with every ``.float()`` replaced by
``.to(dtype)``, and takes the layer list from ``oracle.ref_torch.unet_structure``.  At ``dtype=torch.float32`` it issues the same
torch ops in the same order as the oracle (tests/test_unet_sweep_host.py requires ``torch.equal`` on the prediction and, through
autograd, on every parameter gradient): that pins this twin to the oracle, which the g4 / g15 digests pin to the reference.  At
``dtype=torch.float64`` everything, the timestep sinusoid included, is evaluated in float64: the reference the whole-UNet GPU tests
compare with.  Dropout masks (``cfg["_drop_masks"]`` of the oracle) are not restated: the sweep runs at dropout 0."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle import ref_torch as R

Tensor = torch.Tensor


# --------------------------------------------------------------------------- embeddings
def sinusoidal_embedding(t: Tensor, dim: int, dtype, wavelength: int = 10000) -> Tensor:
    """ref_torch.sinusoidal_embedding: interleaved sin / cos of t / wavelength^(2i / dim), exponent, power, quotient and sin / cos in ``dtype``."""
    assert dim % 2 == 0
    i = torch.arange(dim // 2)
    omega = torch.pow(wavelength, (2 * i).to(dtype) / dim)
    pe = torch.empty(len(t), dim, dtype=dtype)
    arg = t.to(dtype)[:, None] / omega[None, :]
    pe[:, 2 * i] = torch.sin(arg).to(dtype)
    pe[:, 2 * i + 1] = torch.cos(arg).to(dtype)
    return pe


def multi_embeddings(y: Tensor, parameter_space, sd: Dict[str, Tensor], prefix: str = "cond_fn.") -> Optional[Tensor]:
    """ref_torch.multi_embeddings: the category of y[:, i] by exact equality in the (float32) value list, embedded and summed over keys."""
    emb = None
    for i, key in enumerate(parameter_space.keys()):
        yi = y if y.dim() == 1 else y[:, i]
        space = torch.tensor(parameter_space[key])
        categorical = torch.where(yi[:, None] == space[None, :])[1]
        e = F.embedding(categorical, sd[f"{prefix}embedding_layers.{key}.weight"])
        emb = e if emb is None else emb + e
    return emb


def unet_embedding(sd, cfg, timesteps: Tensor, y, parameter_space, dtype) -> Tensor:
    act = R._act(cfg)
    assert (y is not None) == (cfg.get("num_classes", None) is not None)
    e = sinusoidal_embedding(timesteps, cfg["model_channels"], dtype)
    e = F.linear(e, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    e = F.linear(act(e), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    if y is not None:
        if y.dim() == 2 and y.shape == e.shape:
            e = e + y.to(dtype)
        else:
            e = e + multi_embeddings(y, parameter_space, sd)
    return e


# --------------------------------------------------------------------------- layers
def group_norm32(x: Tensor, w: Tensor, b: Tensor, dtype) -> Tensor:
    return F.group_norm(x.to(dtype), 32, w, b, eps=1e-5).type(x.dtype)


def conv_nd(dims: int, x: Tensor, w: Tensor, b: Optional[Tensor], stride=1, padding=0) -> Tensor:
    return {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}[dims](x, w, b, stride=stride, padding=padding)


def upsample(dims: int, x: Tensor) -> Tensor:
    """Nearest x2; 3-D keeps the depth."""
    if dims == 3:
        return F.interpolate(x, (x.shape[2], x.shape[3] * 2, x.shape[4] * 2), mode="nearest")
    return F.interpolate(x, scale_factor=2, mode="nearest")


def avg_pool(dims: int, x: Tensor) -> Tensor:
    """Average pool, kernel = stride = 2; 3-D: (1, 2, 2)."""
    if dims == 3:
        return F.avg_pool3d(x, (1, 2, 2), (1, 2, 2))
    return {1: F.avg_pool1d, 2: F.avg_pool2d}[dims](x, 2, 2)


def resblock(dims: int, x: Tensor, emb: Tensor, sd, p: str, use_scale_shift_norm: bool, updown, act, dtype) -> Tensor:
    h = act(group_norm32(x, sd[p + "in_layers.0.weight"], sd[p + "in_layers.0.bias"], dtype))
    if updown is not None:
        rs = (lambda v: upsample(dims, v)) if updown == "up" else (lambda v: avg_pool(dims, v))
        h, x = rs(h), rs(x)
    h = conv_nd(dims, h, sd[p + "in_layers.2.weight"], sd[p + "in_layers.2.bias"], padding=1)
    emb_out = F.linear(act(emb), sd[p + "emb_layers.1.weight"], sd[p + "emb_layers.1.bias"]).type(h.dtype)
    while emb_out.dim() < h.dim():
        emb_out = emb_out[..., None]
    if use_scale_shift_norm:
        scale, shift = torch.chunk(emb_out, 2, dim=1)
        h = group_norm32(h, sd[p + "out_layers.0.weight"], sd[p + "out_layers.0.bias"], dtype) * (1 + scale) + shift
        h = conv_nd(dims, act(h), sd[p + "out_layers.3.weight"], sd[p + "out_layers.3.bias"], padding=1)
    else:
        h = h + emb_out
        h = group_norm32(h, sd[p + "out_layers.0.weight"], sd[p + "out_layers.0.bias"], dtype)
        h = conv_nd(dims, act(h), sd[p + "out_layers.3.weight"], sd[p + "out_layers.3.bias"], padding=1)
    if (p + "skip_connection.weight") in sd:
        w = sd[p + "skip_connection.weight"]
        pad = 1 if w.shape[-1] == 3 else 0
        x = conv_nd(dims, x, w, sd[p + "skip_connection.bias"], padding=pad)
    return x + h


def qkv_attention(qkv: Tensor, n_heads: int, new_order: bool, dtype) -> Tensor:
    bs, width, length = qkv.shape
    assert width % (3 * n_heads) == 0
    ch = width // (3 * n_heads)
    scale = 1 / math.sqrt(math.sqrt(ch))
    if new_order:
        q, k, v = qkv.chunk(3, dim=1)
        q = (q * scale).reshape(bs * n_heads, ch, length)
        k = (k * scale).reshape(bs * n_heads, ch, length)
        v = v.reshape(bs * n_heads, ch, length)
    else:
        q, k, v = qkv.reshape(bs * n_heads, ch * 3, length).split(ch, dim=1)
        q, k = q * scale, k * scale
    weight = torch.einsum("bct,bcs->bts", q, k)
    weight = torch.softmax(weight.to(dtype), dim=-1).type(weight.dtype)
    a = torch.einsum("bts,bcs->bct", weight, v)
    return a.reshape(bs, -1, length)


def attention_block(x: Tensor, sd, p: str, n_heads: int, new_order: bool, dtype) -> Tensor:
    b, c, *spatial = x.shape
    x = x.reshape(b, c, -1)
    qkv = F.conv1d(group_norm32(x, sd[p + "norm.weight"], sd[p + "norm.bias"], dtype), sd[p + "qkv.weight"], sd[p + "qkv.bias"])
    h = qkv_attention(qkv, n_heads, new_order, dtype)
    h = F.conv1d(h, sd[p + "proj_out.weight"], sd[p + "proj_out.bias"])
    return (x + h).reshape(b, c, *spatial)


def _run_layers(dims, layers, h, emb, sd, cfg, dtype):
    ssn = bool(cfg.get("use_scale_shift_norm", False))
    new_order = bool(cfg.get("use_new_attention_order", False))
    act = R._act(cfg)
    for layer in layers:
        kind, p = layer[0], layer[1]
        if kind == "conv":
            h = conv_nd(dims, h, sd[p + "weight"], sd[p + "bias"], padding=1)
        elif kind == "res":
            h = resblock(dims, h, emb, sd, p, ssn, None, act, dtype)
        elif kind in ("res_up", "res_down"):
            h = resblock(dims, h, emb, sd, p, ssn, kind[4:], act, dtype)
        elif kind == "pool":
            h = avg_pool(dims, h)
        elif kind == "up_only":
            h = upsample(dims, h)
        elif kind == "attn":
            h = attention_block(h, sd, p, layer[3], new_order, dtype)
        elif kind == "down":
            stride = 2 if dims != 3 else (1, 2, 2)
            h = conv_nd(dims, h, sd[p + "weight"], sd[p + "bias"], stride=stride, padding=1)
        elif kind == "up":
            h = conv_nd(dims, upsample(dims, h), sd[p + "weight"], sd[p + "bias"], padding=1)
        else:
            raise KeyError(kind)
    return h


# --------------------------------------------------------------------------- UNetv2
def unet_forward(sd: Dict[str, Tensor], cfg: dict, x: Tensor, timesteps: Tensor, y: Optional[Tensor] = None, parameter_space=None,
                 dtype=torch.float64) -> Tensor:
    """ref_torch.unet_forward in ``dtype``.  ``sd`` tensors of another dtype are cast (a tensor already in ``dtype`` is used as it is,
    so float32 leaves keep their autograd identity); for float64 gradients hand in float64 leaves (``loss_and_grads``)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    dims = cfg.get("dims", 2)
    st = R.unet_structure(cfg)
    emb = unet_embedding(sd, cfg, timesteps, y, parameter_space, dtype)
    hs = []
    h = x.to(dtype)
    for layers in st["input"]:
        h = _run_layers(dims, layers, h, emb, sd, cfg, dtype)
        hs.append(h)
    h = _run_layers(dims, st["middle"], h, emb, sd, cfg, dtype)
    for layers in st["output"]:
        h = torch.cat([h, hs.pop()], dim=1)
        h = _run_layers(dims, layers, h, emb, sd, cfg, dtype)
    h = group_norm32(h, sd["out.0.weight"], sd["out.0.bias"], dtype)
    return conv_nd(dims, R._act(cfg)(h), sd["out.2.weight"], sd["out.2.bias"], padding=1)


def loss_and_grads(forward, sd: Dict[str, Tensor], cfg: dict, x, t, y, parameter_space, target: Tensor, dtype):
    """(prediction, mse loss, {name: gradient}) of ``forward`` - this module's ``unet_forward`` or the oracle's - on leaves of ``dtype``
    made from ``sd``; a parameter the loss does not depend on gets a zero gradient."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    if forward is R.unet_forward:
        assert dtype == torch.float32
        pred = forward(leaves, cfg, x, t, y, parameter_space)
    else:
        pred = forward(leaves, cfg, x, t, y, parameter_space, dtype=dtype)
    loss = F.mse_loss(pred, target.to(dtype))
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    return pred.detach(), loss.detach(), grads
