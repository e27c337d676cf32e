"""-m gpu: the VisionTransformer backbone on the HIP engine against the reference's recorded outputs (tests/golden/g23_vit.npz) and,
tensor by tensor, against the autograd gradients of tests/vit_ref.py (pinned to the same golden by test_vit_host.py).

Bounds: forward rel_l2 < 1e-4 (fp32) / 3e-2 (bf16), as test_gpu_unet.py applies to UNetv2; fp32 gradients rel_l2 <= 2e-3 on every whole
tensor; bf16 gradients cosine >= 0.99 and norm within 5 % (a gradient below 1e-5 of the global norm is checked by magnitude), the rule of
test_gpu_training.py::test_unet_backward_bf16_tracks_reference."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

from helpers import cosine, det_normal, det_state_dict, det_uniform, golden_template, load_golden, rel_l2
from gpu_util import DEV
from vit_cfg import VIT_CASES, vit_inputs
import vit_ref

pytestmark = pytest.mark.gpu

F32_TOL, BF16_TOL = 1e-4, 3e-2
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _weights(case):
    return det_state_dict(golden_template(load_golden("g23_vit.npz"), case), case)


def _model(case, dtype):
    from rho_diffusion_amd.models.vit import VisionTransformer
    m = VisionTransformer(**VIT_CASES[case][0], compute_dtype=dtype)
    m.load_state_dict(_weights(case))
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _reference_grads(case):
    """name -> gradient (and "input") of mse(model(x, t), target) by stock autograd on the CPU, computed once per case."""
    kw, x, t, target = vit_inputs(case)
    ref = vit_ref.build(kw, _weights(case))
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.mse_loss(ref(xr, t), target).backward()
    out = {k: p.grad.detach() for k, p in ref.named_parameters()}
    out["input"] = xr.grad.detach()
    return out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", list(VIT_CASES))
def test_forward_matches_the_reference(case, dtype):
    g = load_golden("g23_vit.npz")
    kw, x, t, _ = vit_inputs(case)
    model = _model(case, dtype).eval()
    with torch.no_grad():
        pred = model(x.to(DEV), t.to(DEV))
    assert pred.dtype == torch.float32 and tuple(pred.shape) == tuple(x.shape)
    e = rel_l2(pred, torch.from_numpy(g[f"{case}/pred"]))
    print(f"vit forward {case} {dtype}: rel_l2 {e:.3e}")
    assert e < (F32_TOL if dtype == "fp32" else BF16_TOL)
    with torch.no_grad():                                  # the cached positional table serves the second call
        again = model(x.to(DEV), t.to(DEV), None)
    assert torch.equal(pred, again)


def _run_backward(case, dtype):
    from rho_diffusion_amd.autograd import mse_loss
    kw, x, t, target = vit_inputs(case)
    model = _model(case, dtype).train()
    xd = x.to(DEV).requires_grad_(True)
    loss = mse_loss(model(xd, t.to(DEV)), target.to(DEV))
    loss.backward()
    return model, xd, loss


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_backward_fp32_every_gradient_tensor(case):
    g = load_golden("g23_vit.npz")
    model, xd, loss = _run_backward(case, "fp32")
    assert abs(loss.item() - float(g[f"{case}/loss"])) < 2e-4 * max(1.0, float(g[f"{case}/loss"]))
    ref = _reference_grads(case)
    bad, worst = [], 0.0
    for name, p in list(model.named_parameters()) + [("input", xd)]:
        assert p.grad is not None, name
        e = rel_l2(p.grad, ref[name])
        worst = max(worst, e)
        if e > 2e-3:
            bad.append((name, e))
    print(f"vit backward fp32 {case}: worst per-tensor rel_l2 {worst:.3e}")
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_backward_bf16_tracks_the_reference(case):
    g = load_golden("g23_vit.npz")
    model, xd, loss = _run_backward(case, "bf16")
    assert abs(loss.item() - float(g[f"{case}/loss"])) < 5e-2 * max(1.0, float(g[f"{case}/loss"]))
    ref = _reference_grads(case)
    gtot = float(np.sqrt(sum(float(v.double().norm()) ** 2 for k, v in ref.items() if k != "input")))
    bad, lo_cos, hi_norm = [], 1.0, 0.0
    for name, p in list(model.named_parameters()) + [("input", xd)]:
        assert p.grad is not None, name
        rn, dn = float(ref[name].double().norm()), float(p.grad.double().norm())
        if rn < 1e-5 * gtot:
            if dn > 1e-3 * gtot:
                bad.append((name, "should be ~0", dn, rn))
            continue
        c = cosine(p.grad, ref[name])
        lo_cos, hi_norm = min(lo_cos, c), max(hi_norm, abs(dn - rn) / rn)
        if c < 0.99 or abs(dn - rn) > 0.05 * rn:
            bad.append((name, round(c, 4), round(dn / rn, 4)))
    print(f"vit backward bf16 {case}: lowest cosine {lo_cos:.4f}, largest norm deviation {hi_norm:.4f}")
    assert not bad, bad[:8]


def test_standalone_blocks():
    from rho_diffusion_amd.models.vit import AttentionBlock, PatchEmbedding
    case = "vit2d"
    kw, x, t, _ = vit_inputs(case)
    sd = _weights(case)
    ref = vit_ref.build(kw, sd)
    pe = PatchEmbedding(kw["num_channels"], kw["patch_size"], kw["embedding_dim"], 2)
    pe.load_state_dict({k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("patch_embedder.")})
    tok = pe.to(DEV)(x.to(DEV))
    want = ref.patch_embedder.conv_shaper(x).flatten(2).transpose(1, 2)
    assert rel_l2(tok, want) < F32_TOL and pe.stored_shape == (4, 6)
    blk = AttentionBlock(kw["embedding_dim"], kw["hidden_dim"], kw["num_heads"], 0.0, kw["activation"])
    blk.load_state_dict({k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith("transformer_blocks.0.")})
    out = blk.to(DEV)(want.detach().to(DEV), t.to(DEV))
    assert out["attn_weights"] is None
    assert rel_l2(out["output"], ref.transformer_blocks[0](want, t)) < F32_TOL


def test_ddpm_pipeline_trains_and_samples():
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.optim import HipAdamW
    kw, x, _, _ = vit_inputs("vit2d")
    T = 50
    ddpm = DDPM("VisionTransformer", dict(kw), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T)
    ddpm.backbone.load_state_dict(_weights("vit2d"))
    ddpm = ddpm.to(DEV)
    ddpm.backbone.train()
    batch = det_uniform(tuple(x.shape), "vitpipe", -1.0, 1.0).to(DEV)
    eps = det_normal(tuple(x.shape), "vitpipe_eps").to(DEV)
    ddpm.noise = lambda data: eps.clone()
    ddpm.random_timesteps = lambda n: torch.tensor([3, 17, 41][:n])
    opt = HipAdamW(ddpm.backbone.parameters(), lr=1e-3)
    losses = []
    for step in range(5):
        opt.zero_grad()
        loss = ddpm.training_step(batch)
        loss.backward()
        if step >= 1:                                                  # the arena exists: the kernels' gradients land in it
            flat = opt.flat_grads[0]
            lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
            for name, p in ddpm.backbone.named_parameters():
                assert lo <= p.grad.data_ptr() < hi, name
            assert float(flat.abs().sum()) > 0
        opt.step()
        losses.append(loss.item())
    print("vit ddpm losses", [round(v, 4) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    del ddpm.noise
    ddpm.backbone.eval()
    out = ddpm.reverse_process(torch.zeros(tuple(x.shape), device=DEV))["denoised"]
    assert tuple(out.shape) == tuple(x.shape) and bool(torch.isfinite(out).all())
    with pytest.raises(NotImplementedError, match="y must be None"):
        ddpm.backbone(batch, torch.tensor([1, 2, 3], device=DEV), torch.zeros(3, device=DEV))


def test_dropout_rule():
    from rho_diffusion_amd.models.vit import VisionTransformer
    kw, x, t, _ = vit_inputs("vit1d")
    sd = _weights("vit1d")
    m0 = VisionTransformer(**dict(kw, dropout=0.0)).to(DEV)
    m2 = VisionTransformer(**dict(kw, dropout=0.2)).to(DEV)
    m0.load_state_dict(sd), m2.load_state_dict(sd)
    with pytest.raises(NotImplementedError, match=r"vit\.py:149-154"):
        m2.train()(x.to(DEV), t.to(DEV))
    with torch.no_grad():
        assert torch.equal(m2.eval()(x.to(DEV), t.to(DEV)), m0.eval()(x.to(DEV), t.to(DEV)))
