"""Case table and reference runs of the whole-ViT sweep (tests/test_vit_sweep_host.py on the CPU, tests/test_gpu_vit_sweep.py and
tests/test_gpu_vit_lifecycle.py on the device).  The error bars are those of tests/unet_sweep_cases.py, imported and not restated:
got against the float64 twin (tests/vit_ref64.py), the float32 restatement (tests/vit_ref.py) only sizing the bound, K = 4 times
its own distance from float64 plus 16 float32 ulps of the tensor's size, in both norms; LIVE / ZERO classify the gradient tensors.

Cases: value = (VisionTransformer constructor kwargs, batch) as in vit_cfg.VIT_CASES.  Each of SWEEP_CASES reaches what the model
accepts and no VIT_CASES entry runs (see the comments), at the smallest shapes at which that path can still go wrong.  Weights:
``det_state_dict`` over the restatement's own state_dict layout (held against the reference's recorded key lists by the host test),
salt = case name; x = det_normal(case + "x"), target = det_normal(case + "tgt"), t = [3, 17, 41, 999, 0][:B]."""
from __future__ import annotations

import functools

import torch

import vit_ref
import vit_ref64 as V64
from detdata import det_normal, det_state_dict
from unet_sweep_cases import (FLOOR, K, LIVE, ZERO, bounds, check_against_refs, classify, describe, ratios, tensor_errors,  # noqa: F401
                              within_bars)
from vit_cfg import VIT_CASES

INPUT = V64.INPUT
TIMESTEPS = [3, 17, 41, 999, 0]

SWEEP_CASES = {
    # B = 1, head width 64, Tanh, hidden < E, N = 7 tokens, K = C p = 6 padded to 32, unequal sinusoid widths
    "b1_tanh_hw64": (dict(patch_size=2, input_shapes=[14], num_channels=3, embedding_dim=128, hidden_dim=32, activation="Tanh",
                          transformer_depth=1, num_heads=2, pos_embedding_dim=64, time_embedding_dim=32, dropout=0.0), 1),
    # head width 128, ELU, an odd patch, N = 3 * 5 = 15, K = 2 * 9 = 18, time sinusoid of 256
    "elu_hw128_2d": (dict(patch_size=3, input_shapes=[9, 15], num_channels=2, embedding_dim=128, hidden_dim=160, activation="ELU",
                          transformer_depth=2, num_heads=1, pos_embedding_dim=32, time_embedding_dim=256, dropout=0.0), 3),
    # head width 256, Sigmoid, p = 1 (K = 1), N = 65: one key tile plus one row
    "sigmoid_hw256": (dict(patch_size=1, input_shapes=[5, 13], num_channels=1, embedding_dim=256, hidden_dim=64, activation="Sigmoid",
                           transformer_depth=1, num_heads=1, dropout=0.0), 2),
    # a LayerNorm row of 1024, 3-D, N = 2 tokens
    "wide_e1024": (dict(patch_size=4, input_shapes=[4, 4, 8], num_channels=1, embedding_dim=1024, hidden_dim=32, activation="SiLU",
                        transformer_depth=1, num_heads=8, dropout=0.0), 2),
    # N = 1 (a softmax over one key, 5 GEMM rows in all), B = 5, depth 3
    "n1_token": (dict(patch_size=4, input_shapes=[4, 4], num_channels=5, embedding_dim=32, hidden_dim=96, activation="GELU",
                      transformer_depth=3, num_heads=2, dropout=0.0), 5),
    # E = 96 (no power of two), N = 133, hidden 224
    "long_ragged": (dict(patch_size=1, input_shapes=[7, 19], num_channels=2, embedding_dim=96, hidden_dim=224, activation="ReLU",
                         transformer_depth=2, num_heads=3, dropout=0.0), 2),
}

ALL_CASES = dict(SWEEP_CASES, **VIT_CASES)


# --------------------------------------------------------------------------- inputs
def state_template(kw: dict):
    """name -> tensor of the shape the reference's ``state_dict`` has for these kwargs, in its order (the restatement's own layout;
    the host tests hold it against the recorded key lists)."""
    return vit_ref.VitRef(**kw).state_dict()


def sweep_inputs(case: str):
    """(kwargs, x, t, target, state dict) of a case, all float32 on the CPU; for a VIT_CASES entry what ``vit_cfg.vit_inputs`` and
    tests/test_gpu_vit.py use."""
    kw, B = ALL_CASES[case]
    shape = (B, kw["num_channels"], *kw["input_shapes"])
    sd = det_state_dict(state_template(kw), case)
    return dict(kw), det_normal(shape, case + "x"), torch.tensor(TIMESTEPS[:B]), det_normal(shape, case + "tgt"), sd


def reference_runs(kw, x, t, target, sd):
    """{"f64": (pred, loss, grads) of the float64 twin, "f32": the same of the float32 restatement} for any weights."""
    return {"f64": V64.loss_and_grads(V64.build(kw, sd, torch.float64), x, t, target),
            "f32": V64.loss_and_grads(vit_ref.build(kw, sd), x, t, target)}


def reference_preds(kw, x, t, sd):
    """The predictions alone, in the layout of ``reference_runs`` (loss and gradients None)."""
    with torch.no_grad():
        p64 = V64.build(kw, sd, torch.float64)(x.double(), t)
        p32 = vit_ref.build(kw, sd)(x, t)
    return {"f64": (p64, None, None), "f32": (p32, None, None)}


@functools.lru_cache(maxsize=None)
def case_refs(case: str):
    """The two reference runs of a case, computed once per process and shared (read-only) by every test that needs them."""
    kw, x, t, target, sd = sweep_inputs(case)
    return reference_runs(kw, x, t, target, sd)
