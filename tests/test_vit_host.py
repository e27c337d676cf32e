"""CPU: the VisionTransformer class surface (registry, state_dict layout, refusals, C-ABI symbols) and the test-side restatement
tests/vit_ref.py pinned to the reference's recorded outputs (tests/golden/g23_vit.npz, written by make_golden_g23.py)."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import det_state_dict, golden_template, grad_digest_of, load_golden, rel_l2
from vit_cfg import VIT_CASES, vit_inputs
import vit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_SYMBOLS = ["rho_layernorm_fwd", "rho_layernorm_bwd", "rho_layernorm_bwd_workspace_bytes", "rho_layernorm_max_dim", "rho_patchify",
               "rho_patchify_dbias_workspace_bytes",
               "rho_unpatchify", "rho_bias_act", "rho_bias_act_bwd", "rho_pos_add", "rho_pos_add_bwd"]


def test_registry_resolves_vision_transformer():
    from rho_diffusion_amd import registry
    from rho_diffusion_amd.models.vit import VisionTransformer
    assert registry.get("models", "VisionTransformer") is VisionTransformer


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_state_dict_layout_equals_the_reference(case):
    from rho_diffusion_amd.models.vit import VisionTransformer
    g = load_golden("g23_vit.npz")
    model = VisionTransformer(**VIT_CASES[case][0])
    got = [f"{k}|{','.join(str(s) for s in v.shape)}" for k, v in model.state_dict().items()]
    assert got == [str(s) for s in g[f"{case}/keys"]]
    model.load_state_dict(det_state_dict(golden_template(g, case), case))          # a reference-shaped checkpoint loads
    ref = vit_ref.build(VIT_CASES[case][0], model.state_dict())
    assert list(ref.state_dict().keys()) == list(model.state_dict().keys())


def test_defaults_follow_the_reference():
    import inspect
    from rho_diffusion_amd.models.vit import AttentionBlock, VisionTransformer
    p = inspect.signature(VisionTransformer.__init__).parameters
    assert list(p)[1:7] == ["patch_size", "input_shapes", "num_channels", "embedding_dim", "hidden_dim", "activation"]
    assert [p[k].default for k in ("transformer_depth", "pos_embedding_dim", "time_embedding_dim", "max_seq_length", "dropout", "num_heads",
                                   "attention_kwargs", "compute_dtype")] == [8, 128, 128, 20_000, 0.2, 16, {}, "bf16"]
    q = inspect.signature(AttentionBlock.__init__).parameters
    assert [q[k].default for k in ("dropout", "activation", "time_dim")] == [0.0, "GELU", 128]


BASE = dict(patch_size=4, input_shapes=[16, 16], num_channels=1, embedding_dim=64, hidden_dim=64, activation="GELU", transformer_depth=1,
            num_heads=2)


@pytest.mark.parametrize("change,lines", [
    (dict(embedding_dim=48, num_heads=3), "vit.py:258-279"),
    (dict(hidden_dim=72), "vit.py:258-279"),
    (dict(embedding_dim=4096, num_heads=16), "vit.py:145-146"),    # wider than a LayerNorm row in registers
    (dict(num_heads=8), "vit.py:149-154"),              # head width 8
    (dict(embedding_dim=1024, num_heads=2), "vit.py:149-154"),      # head width 512
    (dict(input_shapes=[16, 18]), "vit.py:73-78"),
    (dict(attention_kwargs={"bias": False}), "vit.py:148-154"),
    (dict(attention_kwargs={"batch_first": False}), "vit.py:148-154"),
    (dict(activation="PReLU"), "vit.py:157"),
    (dict(activation="Softmax"), "vit.py:157"),
])
def test_refusals_name_the_reference_lines(change, lines):
    from rho_diffusion_amd.models.vit import VisionTransformer
    with pytest.raises(NotImplementedError, match=re.escape(lines)):
        VisionTransformer(**dict(BASE, **change))


def test_standalone_block_refusals_name_their_lines():
    from rho_diffusion_amd.models.vit import AttentionBlock
    with pytest.raises(NotImplementedError, match=re.escape("vit.py:145-164")):
        AttentionBlock(48, 64, 3)
    with pytest.raises(NotImplementedError, match=re.escape("vit.py:145-164")):
        AttentionBlock(64, 72, 2)


def test_accepted_attention_kwargs_and_dropout_construct():
    from rho_diffusion_amd.models.vit import VisionTransformer
    for kw in ({}, {"batch_first": True}, None):
        VisionTransformer(**dict(BASE, attention_kwargs=kw))
    m = VisionTransformer(**dict(BASE, dropout=0.2))
    with pytest.raises(NotImplementedError, match=re.escape("vit.py:149-154")):
        m.transformer_blocks[0]._check_dropout()                      # training mode
    m.eval().transformer_blocks[0]._check_dropout()


def test_new_symbols_are_declared_and_bound():
    from rho_diffusion_amd import hip
    text = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    assert re.search(r"#define\s+RHO_ABI_VERSION\s+10\b", text) and hip.ABI_VERSION == 10
    for name in VIT_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in hip.SIGNATURES, name
    lib = hip.load()
    assert lib.rho_layernorm_max_dim() >= 2048


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_vit_ref_is_pinned_to_the_reference(case):
    g = load_golden("g23_vit.npz")
    kw, x, t, target = vit_inputs(case)
    ref = vit_ref.build(kw, det_state_dict(golden_template(g, case), case))
    pred = ref(x, t)
    loss = torch.nn.functional.mse_loss(pred, target)
    loss.backward()
    assert rel_l2(pred, torch.from_numpy(g[f"{case}/pred"])) < 1e-5
    assert abs(float(loss.detach()) - float(g[f"{case}/loss"])) < 1e-5 * float(g[f"{case}/loss"])
    n = 0
    for name, p in ref.named_parameters():
        d, rec = grad_digest_of(p.grad), g[f"{case}/grad/{name}"]
        assert abs(d[0] - rec[0]) <= 1e-4 * rec[0] + 1e-6, name
        assert np.max(np.abs(d[2:] - rec[2:])) <= 1e-4 * max(rec[0] / np.sqrt(p.numel()), 1e-7) * 10 + 1e-6, name
        n += 1
    assert n == len(g[f"{case}/keys"])
