"""Test-side restatement of the VisionTransformer in stock ``torch.nn`` (CPU or GPU, float32 autograd), written from the model's
description: kernel = stride patch convolution -> tokens in row-major patch order, + act(Linear(sinusoid(position))), ``depth`` blocks
of [t = act(Linear(sinusoid(timestep))); n1 = LN(x + t); r = n1 + MHA(n1); out = r + MLP(LN(r))], a bias-free projection to
``hidden_dim`` and a kernel = stride transposed convolution back to the input shape.  Same ``state_dict`` layout as the product
model, so ``det_state_dict`` weights load into both; pinned to the reference by tests/golden/g23_vit.npz (test_vit_host.py)."""
import math

import torch
from torch import nn


class Sinusoid(nn.Module):
    def __init__(self, dim, wavelength=10000):
        super().__init__()
        self.dim, self.wavelength = dim, wavelength

    def forward(self, t):
        w = torch.pow(self.wavelength, 2 * torch.arange(self.dim // 2, device=t.device) / self.dim)
        a = t.reshape(-1, 1).float() / w
        return torch.stack([a.sin(), a.cos()], dim=-1).reshape(t.numel(), self.dim)


class _Patch(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv_shaper = conv


class Block(nn.Module):
    def __init__(self, E, hidden, heads, act, time_dim):
        super().__init__()
        self.norm_1, self.norm_2 = nn.LayerNorm(E), nn.LayerNorm(E)
        self.attention_layer = nn.MultiheadAttention(E, heads, 0.0, batch_first=True)
        self.linear_block = nn.Sequential(nn.Linear(E, hidden), act(), nn.Identity(), nn.Linear(hidden, E), nn.Identity())
        self.time_transform = nn.Sequential(Sinusoid(time_dim), nn.Linear(time_dim, E, bias=False), act())

    def forward(self, x, t):
        n1 = self.norm_1(x + self.time_transform(t).unsqueeze(1))
        r = n1 + self.attention_layer(n1, n1, n1, need_weights=False)[0]
        return r + self.linear_block(self.norm_2(r))


class VitRef(nn.Module):
    def __init__(self, patch_size, input_shapes, num_channels, embedding_dim, hidden_dim, activation, transformer_depth=8,
                 pos_embedding_dim=128, time_embedding_dim=128, max_seq_length=20_000, dropout=0.0, num_heads=16, attention_kwargs=None):
        super().__init__()
        d = len(input_shapes)
        act = getattr(nn, activation)
        conv, tconv = getattr(nn, f"Conv{d}d"), getattr(nn, f"ConvTranspose{d}d")
        self.patch_embedder = _Patch(conv(num_channels, embedding_dim, patch_size, patch_size))
        self.transformer_blocks = nn.ModuleList([Block(embedding_dim, hidden_dim, num_heads, act, time_embedding_dim)
                                                 for _ in range(transformer_depth)])
        self.output_projection = nn.Linear(embedding_dim, hidden_dim, bias=False)
        self.output_conv = tconv(hidden_dim, num_channels, patch_size, patch_size)
        self.pos_embedding = nn.Sequential(Sinusoid(pos_embedding_dim), nn.Linear(pos_embedding_dim, embedding_dim), act())

    def forward(self, x, t, y=None):
        f = self.patch_embedder.conv_shaper(x)                     # [B, E, *grid]
        grid = f.shape[2:]
        h = f.flatten(2).transpose(1, 2)                           # [B, N, E], row-major patch order
        h = h + self.pos_embedding(torch.arange(h.shape[1], device=x.device))
        for blk in self.transformer_blocks:
            h = blk(h, t)
        h = self.output_projection(h)
        return self.output_conv(h.transpose(1, 2).reshape(x.shape[0], -1, *grid))


def build(kwargs: dict, state_dict: dict) -> VitRef:
    m = VitRef(**{k: v for k, v in kwargs.items() if k != "compute_dtype"})
    m.load_state_dict(state_dict)
    return m
