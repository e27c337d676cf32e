"""-m gpu: GaussianDiffusionPipeline with a learned variance (model_var_type LEARNED / LEARNED_RANGE, gaussian_diffusion.py:368-383)
and the hybrid loss (:893-930) on csrc/gaussian.hip, against tests/golden/g19_learned_variance.npz (make_golden_g19.py, recorded from
the reference) and against the reference's float32 operations restated in numpy.

Tolerances as test_gpu_gaussian_api.py: step outputs 3e-7 of g19 (per-element variance 1e-6 relative: one exp), VLB terms KL 1e-5 /
NLL 1e-4 relative, chains on the fp32 engine rel-L2 2e-3, bf16 5e-2; the output gradient rel-L2 1e-5 against the reference's autograd."""
import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, det_normal, det_state_dict, grad_digest_of, load_golden, rel_l2
from gpu_util import DEV

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [("tiny2d", 50), ("tiny3d", 20)]
VTS = ("LEARNED", "LEARNED_RANGE")
MTS = ("START_X", "EPSILON")
GRAD_KEYS = ("input_blocks.0.0.weight", "time_embed.0.weight", "out.2.weight", "out.2.bias")


def _pipeline(case, T, dtype="fp32", vt="LEARNED_RANGE", **extra):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelVarType
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES[case]
    kw = dict(kw, out_channels=2 * kw["in_channels"], compute_dtype=dtype, **extra)
    pipe = GaussianDiffusionPipeline(UNet, kw, LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T)
    pipe.backbone.load_state_dict(det_state_dict(pipe.backbone.state_dict(), case + "_lv"))
    pipe.model_var_type = ModelVarType[vt]
    pipe.log = lambda *a, **k: None
    return pipe.to(DEV), xshape


def _g(case, T):
    return load_golden("g19_learned_variance.npz"), f"{case}_T{T}"


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _close(a, b, tol=3e-7):
    return torch.allclose(a.detach().cpu().float(), _t(b).reshape(a.shape).float(), rtol=tol, atol=tol)


def _rows(pipe, t, nd):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import gd_table_rows_learned
    from rho_diffusion_amd.engine.ops import GD_ROW
    tab = gd_table_rows_learned(pipe.tables)
    return {k: tab[i][np.asarray(t)].reshape(-1, *([1] * (nd - 1))) for k, i in GD_ROW.items()}


def _np_logvar(r, v, vt):
    if vt == "LEARNED":
        return v
    frac = (v + f32(1)) / f32(2)
    return frac * r["log_beta"] + (f32(1) - frac) * r["post_logvar"]


def _set(pipe, vt, mt, lt="MSE"):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import LossType, ModelMeanType, ModelVarType
    pipe.model_var_type, pipe.model_mean_type, pipe.loss_type = ModelVarType[vt], ModelMeanType[mt], LossType[lt]


@pytest.mark.parametrize("case,T", CASES)
def test_p_mean_variance_steps_and_vb_terms_vs_reference(case, T):
    from rho_diffusion_amd.engine import ops
    g, tag = _g(case, T)
    pipe, xshape = _pipeline(case, T)
    C = xshape[1]
    xt, x0 = _t(g[f"{tag}/xt"]), _t(g[f"{tag}/x0"])
    xtd, x0d = xt.to(DEV), x0.to(DEV)
    tt = _t(g[f"{tag}/t"])
    noise = det_normal(xshape, "g19_step_noise")
    pipe.noise = lambda d, n=noise.to(DEV): n
    worst = {"kl": 0.0, "nll": 0.0}
    for vt in VTS:
        mo = _t(g[f"{tag}/mo_{vt}"])
        mod = mo.to(DEV)
        model = lambda x, t, **k: mod
        for mt in MTS:
            _set(pipe, vt, mt)
            r = _rows(pipe, tt, len(xshape))
            for clip in (True, False):
                k = f"{tag}/pmv_{vt}_{mt}_{int(clip)}"
                o = pipe.p_mean_variance(model, xtd, tt.to(DEV), clip_denoised=clip)
                assert _close(o["pred_xstart"], g[k + "/pred_xstart"]) and _close(o["mean"], g[k + "/mean"]), k
                lv = torch.from_numpy(g[k + "/log_variance"])
                assert o["log_variance"].shape == xt.shape and _close(o["log_variance"], lv, 1e-6), k
                assert torch.allclose(o["variance"].cpu(), torch.from_numpy(g[k + "/variance"]), rtol=1e-6, atol=0), k
                # numpy restatement: the log-variance bit for bit, x0 / mean given the device quantile
                lvn = _np_logvar(r, mo[:, C:].numpy(), vt)
                assert np.array_equal(o["log_variance"].cpu().numpy(), lvn), k
                x0n = mo[:, :C].numpy()
                if mt == "EPSILON":
                    x0n = r["sqrt_recip"] * xt.numpy() - r["sqrt_recipm1"] * x0n
                if clip:
                    q = ops.abs_quantile(torch.from_numpy(np.ascontiguousarray(x0n)).to(DEV), 0.9).cpu().numpy()
                    s = np.maximum(q, f32(1)).reshape(r["abar"].shape)
                    x0n = np.minimum(np.maximum(x0n, -s), s) / s
                assert np.array_equal(o["pred_xstart"].cpu().numpy(), x0n), k
                assert np.array_equal(o["mean"].cpu().numpy(), r["coef1"] * x0n + r["coef2"] * xt.numpy()), k
            for cn, cf in (("nocond", None), ("cond", lambda x, t, **k: -x)):
                o = pipe.p_sample(model, xtd, tt.to(DEV), clip_denoised=True, cond_fn=cf, model_kwargs={})
                assert _close(o["sample"], g[f"{tag}/psample_{vt}_{mt}_{cn}/sample"], 1e-6), (vt, mt, cn)
            o = pipe.ddim_sample(model, xtd, tt.to(DEV), clip_denoised=True, model_kwargs={}, eta=0.5)
            assert _close(o["sample"], g[f"{tag}/ddim_{vt}_{mt}/sample"]), (vt, mt)
            for tn, tv in (("t0", 0), ("tk", T // 3)):
                tb = torch.full((xshape[0],), tv, dtype=torch.long, device=DEV)
                x_t = pipe.q_sample(x0d, tb, noise=det_normal(xshape, "g19_vb_noise").to(DEV))
                out = pipe._vb_terms_bpd(model, x0d, x_t, tb, clip_denoised=False)["output"].cpu()
                ref = torch.from_numpy(g[f"{tag}/vb_{vt}_{mt}_{tn}"])
                err = float(((out - ref).abs() / ref.abs()).max())
                kind = "nll" if tv == 0 else "kl"
                worst[kind] = max(worst[kind], err)
                assert err <= (1e-4 if kind == "nll" else 1e-5), (vt, mt, tn, err)
    print("vb worst relative errors", worst)


@pytest.mark.parametrize("case,T", CASES)
def test_hybrid_loss_terms_and_output_gradient_vs_reference(case, T):
    g, tag = _g(case, T)
    pipe, xshape = _pipeline(case, T)
    C = xshape[1]
    x0 = _t(g[f"{tag}/x0"]).to(DEV)
    tq = _t(g[f"{tag}/train_t"]).to(DEV)
    tnoise = det_normal(xshape, "g19_train_noise").to(DEV)
    assert int(tq[0]) == 0
    for vt in VTS:
        for mt in MTS:
            for lt in ("MSE", "RESCALED_MSE"):
                _set(pipe, vt, mt, lt)
                k = f"{tag}/train_{vt}_{mt}_{lt}"
                leaf = _t(g[f"{tag}/mo_{vt}"]).to(DEV).requires_grad_(True)
                terms = pipe.training_losses(lambda *a, **kw: leaf, x0, tq, noise=tnoise)
                assert set(terms) == {"mse", "vb", "loss"}
                for n in ("mse", "vb", "loss"):
                    ref = torch.from_numpy(g[f"{k}/{n}"])
                    assert torch.allclose(terms[n].detach().cpu(), ref, rtol=1e-5, atol=1e-7), (k, n, terms[n], ref)
                terms["loss"].mean().backward()
                got, ref = leaf.grad.cpu(), torch.from_numpy(g[f"{k}/dout"])
                # the samples at t > 0 (mean half + the KL's variance gradient) at 1e-5; the whole gradient at 2e-5: the t == 0
                # sample's decoder-NLL gradient carries tanh's ulps through 1 - tanh^2 (below)
                assert rel_l2(got[1:], ref[1:]) <= 1e-5, (k, rel_l2(got[1:], ref[1:]))
                assert rel_l2(got, ref) <= 2e-5, (k, rel_l2(got, ref))
                # the mean half carries the MSE gradient only: -(g/n)*2*(target - m), the VLB's share exactly 0
                target = x0 if mt == "START_X" else tnoise
                n = x0[0].numel()
                gm = torch.full((xshape[0],), 1.0 / xshape[0], device=DEV)
                mse_only = -((gm / n).view(-1, *([1] * (len(xshape) - 1))) * (2.0 * (target - leaf.detach()[:, :C])))
                assert torch.equal(leaf.grad[:, :C], mse_only), k
                # the t == 0 sample's variance half (decoder NLL through the tanh CDF) on its own, at the NLL's bar (1e-4: the CDF
                # differences cancel as in the forward and 1 - tanh^2 amplifies tanh's ulps; measured worst 3.8e-5), zero exactly where
                # the clamps cut the path
                assert rel_l2(got[0, C:], ref[0, C:]) <= 1e-4, (k, rel_l2(got[0, C:], ref[0, C:]))
                assert torch.equal(got[0, C:] == 0, ref[0, C:] == 0), k
                assert float(got[0, C:].abs().max()) > 0


def test_hybrid_loss_and_bpd_bit_reproducible_and_split_across_workgroups():
    from rho_diffusion_amd.engine import ops
    pipe, xshape = _pipeline("tiny3d", 20)
    _set(pipe, "LEARNED_RANGE", "EPSILON", "RESCALED_MSE")
    shape = (2, 1, 128, 128, 128)
    x0 = det_normal(shape, "g19_big_x0").clamp(-1, 1).to(DEV)
    noise = det_normal(shape, "g19_big_noise").to(DEV)
    mo = torch.cat([noise * 0.9, det_normal(shape, "g19_big_v").clamp(-1, 1).to(DEV)], dim=1).contiguous()
    t = torch.tensor([0, 7], device=DEV)
    x_t = pipe.q_sample(x0, t, noise=noise)
    tab = pipe._tab(DEV)
    outs = []
    for _ in range(2):
        loss, mse, vb = ops.gd_hybrid_loss(x0, x_t, noise, mo, t, tab, ops.GD_EPSILON, ops.GD_LEARNED_RANGE, 0.02)
        grad = ops.gd_hybrid_loss_bwd(x0, x_t, noise, mo, t, tab, ops.GD_EPSILON, ops.GD_LEARNED_RANGE, 0.02,
                                      torch.full((2,), 0.5, device=DEV), None, None)
        outs.append((torch.stack([loss, mse, vb]).cpu(), grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the fused pass against the separate VLB entry point on the same halves (KL and NLL of the same elements)
    vbx = torch.empty(2, device=DEV)
    ops.gd_vlb_terms(x0, x_t, mo[:, :1], t, tab, ops.GD_EPSILON, None, None, vbx, var_values=mo[:, 1:], var_type=ops.GD_LEARNED_RANGE)
    assert torch.allclose(outs[0][0][2], vbx.cpu() * 0.02, rtol=1e-6)
    assert torch.isfinite(outs[0][1]).all()
    x = det_normal((2, 1, 4, 8, 8), "g19_bpd_x0").clamp(-1, 1).to(DEV)
    pipe._noise_offset = 0
    a = pipe.calc_bpd_loop(pipe.backbone, x)
    pipe._noise_offset = 0
    b = pipe.calc_bpd_loop(pipe.backbone, x)
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case,T", CASES)
def test_backbone_loops_bpd_and_reverse_process_fp32_vs_reference(case, T):
    g, tag = _g(case, T)
    pipe, xshape = _pipeline(case, T)
    _set(pipe, "LEARNED_RANGE", "EPSILON", "RESCALED_MSE")
    tape = [det_normal(xshape, f"g19tape{T}_{i}").to(DEV) for i in range(T + 1)]
    it = iter(tape)
    pipe.noise = lambda d: next(it)
    out = pipe.p_sample_loop(pipe.backbone, xshape)
    assert rel_l2(out.cpu(), torch.from_numpy(g[f"{tag}/p_sample_loop"])) < 2e-3
    it = iter(tape)
    out = pipe.ddim_sample_loop(pipe.backbone, xshape, eta=0.5)
    assert rel_l2(out.cpu(), torch.from_numpy(g[f"{tag}/ddim_sample_loop"])) < 2e-3
    if T == 20:
        it = iter([det_normal(xshape, f"g19bpd{T}_{i}").to(DEV) for i in range(T)])
        res = pipe.calc_bpd_loop(pipe.backbone, _t(g[f"{tag}/x0"]).to(DEV))
        for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
            ref = torch.from_numpy(g[f"{tag}/bpd/{k}"])
            assert res[k].shape == ref.shape and rel_l2(res[k].cpu(), ref) < 2e-3, k
    _set(pipe, "LEARNED_RANGE", "START_X")
    it = iter(tape)
    out = pipe.reverse_process(torch.zeros(xshape, device=DEV))["denoised"]
    assert rel_l2(out.cpu(), torch.from_numpy(g[f"{tag}/reverse_process"])) < 2e-3
    it = iter(tape)
    pipe.sampling_batch_size = xshape[0]
    pipe.make_image_grid = lambda x, filename=None: x
    out = pipe.generate()
    # generate()'s template takes in_channels with a learned variance (the reference's out_channels would be 2C)
    assert tuple(out.shape) == tuple(xshape) and torch.isfinite(out).all()


def _digest_ok(got, want, tag):
    assert abs(got[0] - want[0]) <= 2e-3 * want[0], (tag, got[0], want[0])
    assert np.abs(got[2:] - want[2:]).max() <= 5e-3 * max(np.abs(want[2:]).max(), 1e-8), tag


@pytest.mark.parametrize("case,T", CASES)
def test_backbone_training_losses_and_training_step_gradients_vs_reference(case, T):
    g, tag = _g(case, T)
    pipe, xshape = _pipeline(case, T)
    pipe.train()
    _set(pipe, "LEARNED_RANGE", "EPSILON", "RESCALED_MSE")
    x0 = _t(g[f"{tag}/x0"]).to(DEV)
    tq = _t(g[f"{tag}/train_t"]).to(DEV)
    tnoise = det_normal(xshape, "g19_train_noise").to(DEV)
    params = dict(pipe.backbone.named_parameters())
    for mt in MTS:
        _set(pipe, "LEARNED_RANGE", mt, "RESCALED_MSE")
        pipe.backbone.zero_grad(set_to_none=True)
        terms = pipe.training_losses(pipe.backbone, x0, tq, noise=tnoise)
        k = f"{tag}/bb_train_{mt}"
        for n in ("loss", "mse", "vb"):
            assert torch.allclose(terms[n].detach().cpu(), torch.from_numpy(g[f"{k}/{n}"]), rtol=2e-4, atol=1e-6), (k, n)
        terms["loss"].mean().backward()
        for p in GRAD_KEYS:
            _digest_ok(grad_digest_of(params[p].grad), g[f"{k}/grad/{p}"], (k, p))
    _set(pipe, "LEARNED_RANGE", "EPSILON", "RESCALED_MSE")
    pipe.backbone.zero_grad(set_to_none=True)
    pipe.random_timesteps = lambda n: tq.cpu()
    pipe.noise = lambda d: tnoise
    loss = pipe.training_step(x0)
    assert torch.allclose(loss.detach().cpu(), torch.from_numpy(g[f"{tag}/step/loss"]), rtol=2e-4, atol=1e-6)
    loss.backward()
    for p in GRAD_KEYS:
        _digest_ok(grad_digest_of(params[p].grad), g[f"{tag}/step/grad/{p}"], ("step", p))


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 5e-2)])
@pytest.mark.parametrize("case", ["tiny2d", "tiny3d"])
@pytest.mark.parametrize("ck", [False, True])
def test_two_channel_head_forward_and_gradients_vs_oracle(case, dtype, tol, ck):
    """UNetv2(out_channels = 2 * in_channels) on the HIP engine: the 2-channel head takes the generic conv (no 1-channel head
    form); forward and parameter gradients against the oracle's torch restatement on the CPU, with and without use_checkpoint."""
    from oracle import ref_torch as R
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES[case]
    cfg = dict(kw, out_channels=2 * kw["in_channels"])
    model = UNet(**dict(cfg, use_checkpoint=ck), compute_dtype=dtype)
    model.load_state_dict(det_state_dict(model.state_dict(), case + "_lv"))
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = det_normal(xshape, case + "_lvx")
    t = torch.tensor([3, 11][: xshape[0]])
    w = det_normal((xshape[0], 2 * xshape[1]) + tuple(xshape[2:]), case + "_lvw")
    pred = model(x.to(DEV), t.to(DEV))
    assert pred.shape == w.shape
    ref = R.unet_forward(sd, cfg, x, t)
    assert rel_l2(pred.detach().cpu(), ref.detach()) < tol
    (pred * w.to(DEV)).sum().backward()
    (ref * w).sum().backward()
    for k in GRAD_KEYS:
        got, want = dict(model.named_parameters())[k].grad.cpu(), sd[k].grad
        assert rel_l2(got, want) < (1e-3 if dtype == "fp32" else 8e-2), (k, rel_l2(got, want))


def test_bf16_learned_sampling_and_training_close_to_reference():
    case, T = "tiny3d", 20
    g, tag = _g(case, T)
    pipe, xshape = _pipeline(case, T, "bf16")
    _set(pipe, "LEARNED_RANGE", "EPSILON", "RESCALED_MSE")
    tape = [det_normal(xshape, f"g19tape{T}_{i}").to(DEV) for i in range(T + 1)]
    it = iter(tape)
    pipe.noise = lambda d: next(it)
    assert rel_l2(pipe.p_sample_loop(pipe.backbone, xshape).cpu(), torch.from_numpy(g[f"{tag}/p_sample_loop"])) < 5e-2
    pipe.train()
    terms = pipe.training_losses(pipe.backbone, _t(g[f"{tag}/x0"]).to(DEV), _t(g[f"{tag}/train_t"]).to(DEV),
                                 noise=det_normal(xshape, "g19_train_noise").to(DEV))
    assert rel_l2(terms["loss"].detach().cpu(), torch.from_numpy(g[f"{tag}/bb_train_EPSILON/loss"])) < 5e-2
    terms["loss"].mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in pipe.backbone.parameters() if p.grad is not None)


def test_out_of_range_timestep_raises_at_the_poll():
    pipe, xshape = _pipeline("tiny2d", 20, "bf16")
    x = det_normal(xshape, "g19_xt").to(DEV)
    mo = torch.zeros((xshape[0], 2 * xshape[1]) + tuple(xshape[2:]), device=DEV)
    pipe.p_mean_variance(lambda *a, **k: mo, x, torch.tensor([3, 20], device=DEV))
    with pytest.raises(IndexError, match="outside"):
        pipe._check_backbone_errors()
    pipe._check_backbone_errors()
