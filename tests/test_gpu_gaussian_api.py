"""-m gpu: GaussianDiffusionPipeline's guided-diffusion API (gaussian_diffusion.py:277-1009) and rho_diffusion.metrics.losses on
csrc/gaussian.hip, against values recorded from the real reference (tests/golden/g18_gaussian_api.npz, make_golden_g18.py) and
against the reference's float32 operation sequence restated in numpy.

Tolerances: step kernels with no transcendental (p_mean_variance, DDIM forward / reverse, with and without cond_fn) bit-exact against
the numpy restatement given the device quantile, and within 3e-7 of g18 (the bar of test_gpu_gaussian.py: ATen's CPU kernels are
not bit-stable across host ISAs); p_sample (exp of the log-variance) 3e-7.  Metrics: normal_kl 2e-6 relative + 2e-6 absolute (two
exps), the discretized log-likelihood 1e-4 absolute + 2e-5 relative (log(cdf_plus - cdf_min) and log(1 - cdf_min) cancel: one ulp
of tanh moves single elements; measured worst 1.2e-4 at a value near -12),
the CDF 3e-7 absolute.  Variational terms: KL relative 1e-5, decoder NLL 1e-4.  Chains on the fp32 engine rel-L2 <= 2e-3, bf16
engine <= 5e-2 (the bars of the existing chains)."""
import numpy as np
import pytest
import torch
from torch import nn

from helpers import UNET_CASES, det_normal, det_state_dict, det_uniform, golden_template, grad_digest_of, load_golden, rel_l2
from gpu_util import DEV

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = [("tiny2d", 50), ("tiny3d", 20)]


def _pipeline(case, T, dtype="fp32"):
    from rho_diffusion_amd.diffusion import GaussianDiffusionPipeline, LinearSchedule
    from rho_diffusion_amd.models import UNet
    g4 = load_golden("g4_unet.npz")
    kw, xshape, _ = UNET_CASES[case]
    pipe = GaussianDiffusionPipeline(UNet, dict(kw, compute_dtype=dtype), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T)
    pipe.backbone.load_state_dict(det_state_dict(golden_template(g4, case), case))
    return pipe.to(DEV), xshape


def _inputs(xshape):
    B = xshape[0]
    scale = torch.tensor([0.3] + [2.5 + i for i in range(B - 1)]).view(-1, *([1] * (len(xshape) - 1)))
    return det_uniform(xshape, "g18_x0", -1.0, 1.0), det_normal(xshape, "g18_xt"), det_normal(xshape, "g18_fake") * scale


def _rows(pipe, t, nd):
    """float32 per-sample table values [B, 1, ...] for the numpy restatement."""
    from rho_diffusion_amd.diffusion.gaussian_diffusion import gd_table_rows
    from rho_diffusion_amd.engine.ops import GD_ROW
    tab = gd_table_rows(pipe.tables, pipe.model_var_type)
    return {k: tab[i][t.numpy()].reshape(-1, *([1] * (nd - 1))) for k, i in GD_ROW.items()}


def _np_x0(r, x, m, eps, quant):
    x0 = (r["sqrt_recip"] * x) - (r["sqrt_recipm1"] * m) if eps else m
    if quant is not None:
        s = np.maximum(quant, f32(1)).reshape(r["abar"].shape)
        x0 = np.minimum(np.maximum(x0, -s), s) / s
    return x0


def _np_ddim(r, x, x0, eta, grad, reverse, noise, t):
    ax = r["sqrt_recip"] * x
    if grad is not None:
        e = (ax - x0) / r["sqrt_recipm1"]
        e = e - np.sqrt(f32(1) - r["abar"]) * grad
        x0 = ax - r["sqrt_recipm1"] * e
    eps = (ax - x0) / r["sqrt_recipm1"]
    if reverse:
        return x0 * np.sqrt(r["abar_next"]) + np.sqrt(f32(1) - r["abar_next"]) * eps, x0
    ab, abp = r["abar"], r["abar_prev"]
    sigma = f32(eta) * np.sqrt((f32(1) - abp) / (f32(1) - ab))
    sigma = sigma * np.sqrt(f32(1) - ab / abp)
    v = x0 * np.sqrt(abp) + np.sqrt((f32(1) - abp) - sigma * sigma) * eps
    if eta != 0.0:
        mask = (t.numpy() != 0).astype(np.float32).reshape(ab.shape)
        v = v + (mask * sigma) * noise
    return v, x0


def _close(a, b, tol=3e-7):
    a = a.cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    b = torch.from_numpy(np.asarray(b)) if not torch.is_tensor(b) else b
    return torch.allclose(a.reshape(b.shape).float(), b.float(), rtol=tol, atol=tol)


def _ps(v):
    return v.reshape(v.shape[0], -1)[:, 0].cpu()


@pytest.mark.parametrize("case,T", CASES)
def test_distribution_helpers_and_p_mean_variance_vs_reference(case, T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelMeanType, ModelVarType
    from rho_diffusion_amd.engine import ops
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T)
    x0, xt, fake = _inputs(xshape)
    x0d, xtd, faked = x0.to(DEV), xt.to(DEV), fake.to(DEV)
    model = lambda x, t, **k: faked
    for tn in ("edge", "mid"):
        tt = torch.from_numpy(g[f"{tag}/t_{tn}"])
        m, v, lv = pipe.q_mean_variance(x0d, tt.to(DEV))
        assert _close(m, g[f"{tag}/qmv_{tn}/mean"]) and torch.equal(_ps(v), torch.from_numpy(g[f"{tag}/qmv_{tn}/var"]))
        assert torch.equal(_ps(lv), torch.from_numpy(g[f"{tag}/qmv_{tn}/logvar"])) and v.shape == x0d.shape
        m, v, lv = pipe.q_posterior_mean_variance(x0d, xtd, tt.to(DEV))
        assert _close(m, g[f"{tag}/qpost_{tn}/mean"]) and torch.equal(_ps(v), torch.from_numpy(g[f"{tag}/qpost_{tn}/var"]))
        assert torch.equal(_ps(lv), torch.from_numpy(g[f"{tag}/qpost_{tn}/logvar"]))
        for mt in ("START_X", "EPSILON"):
            for vt in ("FIXED_LARGE", "FIXED_SMALL"):
                pipe.model_mean_type, pipe.model_var_type = ModelMeanType[mt], ModelVarType[vt]
                r = _rows(pipe, tt, len(xshape))
                for clip in (True, False):
                    k = f"{tag}/pmv_{tn}_{mt}_{vt}_{int(clip)}"
                    out = pipe.p_mean_variance(model, xtd, tt.to(DEV), clip_denoised=clip)
                    assert _close(out["pred_xstart"], g[k + "/pred_xstart"]) and _close(out["mean"], g[k + "/mean"]), k
                    assert torch.equal(_ps(out["variance"]), torch.from_numpy(g[k + "/var"])), k
                    assert torch.equal(_ps(out["log_variance"]), torch.from_numpy(g[k + "/logvar"])), k
                    # bit-exact against the float32 sequence given the device quantile of x0
                    xn, mn = xt.numpy(), fake.numpy()
                    q = None
                    if clip:
                        pre = _np_x0(r, xn, mn, mt == "EPSILON", None)
                        q = ops.abs_quantile(torch.from_numpy(np.ascontiguousarray(pre)).to(DEV), 0.9).cpu().numpy()
                    x0n = _np_x0(r, xn, mn, mt == "EPSILON", q)
                    assert np.array_equal(out["pred_xstart"].cpu().numpy(), x0n), k
                    assert np.array_equal(out["mean"].cpu().numpy(), r["coef1"] * x0n + r["coef2"] * xn), k


@pytest.mark.parametrize("case,T", CASES)
def test_single_steps_vs_reference(case, T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelMeanType
    from rho_diffusion_amd.engine import ops
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T)
    x0, xt, fake = _inputs(xshape)
    xtd, faked = xt.to(DEV), fake.to(DEV)
    noise = det_normal(xshape, "g18_step_noise")
    pipe.noise = lambda d, n=noise.to(DEV): n
    model = lambda x, t, **k: faked
    grad = lambda x, t, **k: -x
    for tn in ("edge", "mid"):
        tt = torch.from_numpy(g[f"{tag}/t_{tn}"])
        for mt in ("START_X", "EPSILON"):
            pipe.model_mean_type = ModelMeanType[mt]
            r = _rows(pipe, tt, len(xshape))
            pre = _np_x0(r, xt.numpy(), fake.numpy(), mt == "EPSILON", None)
            q = ops.abs_quantile(torch.from_numpy(np.ascontiguousarray(pre)).to(DEV), 0.9).cpu().numpy()
            x0n = _np_x0(r, xt.numpy(), fake.numpy(), mt == "EPSILON", q)
            for cn, cf in (("nocond", None), ("cond", grad)):
                o = pipe.p_sample(model, xtd, tt.to(DEV), clip_denoised=True, cond_fn=cf, model_kwargs={})
                k = f"{tag}/psample_{tn}_{mt}_{cn}"
                assert _close(o["pred_xstart"], g[k + "/pred_xstart"]) and _close(o["sample"], g[k + "/sample"]), k
                for eta in (0.0, 0.5):
                    o = pipe.ddim_sample(model, xtd, tt.to(DEV), clip_denoised=True, cond_fn=cf, model_kwargs={}, eta=eta)
                    k = f"{tag}/ddim_{tn}_{mt}_{cn}_eta{eta}"
                    assert _close(o["pred_xstart"], g[k + "/pred_xstart"]) and _close(o["sample"], g[k + "/sample"]), k
                    v, px = _np_ddim(r, xt.numpy(), x0n, eta, -xt.numpy() if cf else None, False, noise.numpy(), tt)
                    assert np.array_equal(o["sample"].cpu().numpy(), v) and np.array_equal(o["pred_xstart"].cpu().numpy(), px), k
            o = pipe.ddim_reverse_sample(model, xtd, tt.to(DEV), clip_denoised=True)
            k = f"{tag}/ddim_rev_{tn}_{mt}"
            assert _close(o["pred_xstart"], g[k + "/pred_xstart"]) and _close(o["sample"], g[k + "/sample"]), k
            v, _ = _np_ddim(r, xt.numpy(), x0n, 0.0, None, True, None, tt)
            assert np.array_equal(o["sample"].cpu().numpy(), v), k


@pytest.mark.parametrize("case,T", CASES)
def test_vb_terms_and_prior_vs_reference(case, T):
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T)
    x0, _, fake = _inputs(xshape)
    x0d = x0.to(DEV)
    model = lambda x, t, **k: (fake * 0.25).to(DEV)
    worst = {"kl": 0.0, "nll": 0.0}
    B = xshape[0]
    for tn, tv in (("t0", 0), ("tk", T // 3), ("tlast", T - 1)):
        tt = torch.full((B,), tv, dtype=torch.long, device=DEV)
        x_t = pipe.q_sample(x0d, tt, noise=det_normal(xshape, "g18_vb_noise").to(DEV))
        for clip in (True, False):
            o = pipe._vb_terms_bpd(model, x0d, x_t, tt, clip_denoised=clip)
            ref = torch.from_numpy(g[f"{tag}/vb_{tn}_{int(clip)}/output"])
            err = float(((o["output"].cpu() - ref).abs() / ref.abs()).max())
            kind = "nll" if tv == 0 else "kl"
            worst[kind] = max(worst[kind], err)
            assert err <= (1e-4 if kind == "nll" else 1e-5), (tn, clip, err)
            assert _close(o["pred_xstart"], g[f"{tag}/vb_{tn}_{int(clip)}/pred_xstart"])
    prior = pipe._prior_bpd(x0d).cpu()
    ref = torch.from_numpy(g[f"{tag}/prior_bpd"])
    assert float(((prior - ref).abs() / ref.abs()).max()) <= 1e-5
    print("vb worst relative errors", worst)


def test_metrics_vs_reference():
    from rho_diffusion_amd.metrics import approx_standard_normal_cdf, discretized_gaussian_log_likelihood, normal_kl
    g = load_golden("g18_gaussian_api.npz")
    d = {k: torch.from_numpy(g[f"metrics/{k}"]).to(DEV) for k in ("m1", "m2", "lv1", "lv2", "ps_lv", "dx", "dmeans", "dls", "dps_ls")}

    def kl_ok(got, key):
        ref = torch.from_numpy(g[f"metrics/{key}"])
        assert got.shape == ref.shape and torch.allclose(got.cpu(), ref, rtol=2e-6, atol=2e-6), (key, float((got.cpu() - ref).abs().max()))
    kl_ok(normal_kl(d["m1"], d["lv1"], d["m2"], d["lv2"]), "kl_full")
    kl_ok(normal_kl(d["m1"], d["ps_lv"], d["m2"], d["lv2"]), "kl_ps")
    kl_ok(normal_kl(d["m1"], d["lv1"], 0.0, 0.0), "kl_scalar")
    for key, ls in (("dgll_full", d["dls"]), ("dgll_ps", d["dps_ls"])):
        got = discretized_gaussian_log_likelihood(d["dx"], means=d["dmeans"], log_scales=ls).cpu()
        ref = torch.from_numpy(g[f"metrics/{key}"])
        # measured worst: 1.2e-4 absolute at a log-probability near -12 (1 - cdf_min cancels in the upper tail)
        assert got.shape == ref.shape and torch.allclose(got, ref, rtol=2e-5, atol=1e-4), (key, float((got - ref).abs().max()))
        # the where-branches at x = +-0.999 (as float32), one ulp either side and +-1 select exactly as the reference
        edge = slice(0, 8)
        assert torch.allclose(got.view(-1)[edge], ref.view(-1)[edge], rtol=1e-5, atol=1e-5), key
    got = approx_standard_normal_cdf(d["m1"] * 3.0).cpu()
    assert float((got - torch.from_numpy(g["metrics/cdf"])).abs().max()) <= 3e-7


@pytest.mark.parametrize("case,T", CASES)
def test_loops_fp32_engine_vs_reference(case, T):
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T)
    tape = [det_normal(xshape, f"g18tape{T}_{i}").to(DEV) for i in range(T + 1)]
    it = iter(tape)
    pipe.noise = lambda d: next(it)
    out = pipe.p_sample_loop(pipe.backbone, xshape)
    assert rel_l2(out.cpu(), torch.from_numpy(g[f"{tag}/p_sample_loop"])) < 2e-3
    for eta in (0.0, 0.5):
        it = iter(tape)
        out = pipe.ddim_sample_loop(pipe.backbone, xshape, eta=eta)
        assert rel_l2(out.cpu(), torch.from_numpy(g[f"{tag}/ddim_sample_loop_eta{eta}"])) < 2e-3, eta
    it = iter([det_normal(xshape, f"g18bpd{T}_{i}").to(DEV) for i in range(T)])
    res = pipe.calc_bpd_loop(pipe.backbone, det_uniform(xshape, "g18_x0", -1.0, 1.0).to(DEV))
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        ref = torch.from_numpy(g[f"{tag}/bpd/{k}"])
        assert res[k].shape == ref.shape and rel_l2(res[k].cpu(), ref) < 2e-3, k


def test_loops_bf16_engine_close_to_reference():
    case, T = "tiny3d", 20
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T, "bf16")
    tape = [det_normal(xshape, f"g18tape{T}_{i}").to(DEV) for i in range(T + 1)]
    it = iter(tape)
    pipe.noise = lambda d: next(it)
    assert rel_l2(pipe.p_sample_loop(pipe.backbone, xshape).cpu(), torch.from_numpy(g[f"{tag}/p_sample_loop"])) < 5e-2
    it = iter(tape)
    assert rel_l2(pipe.ddim_sample_loop(pipe.backbone, xshape, eta=0.5).cpu(), torch.from_numpy(g[f"{tag}/ddim_sample_loop_eta0.5"])) < 5e-2
    it = iter([det_normal(xshape, f"g18bpd{T}_{i}").to(DEV) for i in range(T)])
    res = pipe.calc_bpd_loop(pipe.backbone, det_uniform(xshape, "g18_x0", -1.0, 1.0).to(DEV))
    assert rel_l2(res["vb"].cpu(), torch.from_numpy(g[f"{tag}/bpd/vb"])) < 5e-2


def test_progressive_generators_yield_fresh_tensors():
    pipe, xshape = _pipeline("tiny2d", 20, "bf16")
    for gen in (pipe.p_sample_loop_progressive(pipe.backbone, xshape),
                pipe.ddim_sample_loop_progressive(pipe.backbone, xshape, eta=0.5)):
        outs = list(gen)
        assert len(outs) == 20
        ptrs = {o[k].data_ptr() for o in outs for k in ("sample", "pred_xstart")}
        assert len(ptrs) == 40
        assert not torch.equal(outs[0]["sample"], outs[-1]["sample"])


def test_calc_bpd_loop_bit_reproducible_and_free_of_host_syncs():
    pipe, xshape = _pipeline("tiny2d", 20, "bf16")
    x0 = det_uniform(xshape, "g18_x0", -1.0, 1.0).to(DEV)
    pipe.calc_bpd_loop(pipe.backbone, x0)                    # builds the engine plan
    pipe._noise_offset = 0
    a = pipe.calc_bpd_loop(pipe.backbone, x0)
    # Tensor.item / .cpu / .tolist and torch.cuda.synchronize raise while the loop body runs; the one error poll after the loop
    # (_check_backbone_errors) runs with them restored
    names = ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.cuda, "synchronize"))
    saved = [getattr(o, n) for o, n in names]
    orig_poll = pipe._check_backbone_errors

    def forbid(*a, **k):
        raise AssertionError("host synchronisation inside the loop")

    def restore():
        for (o, n), f in zip(names, saved):
            setattr(o, n, f)

    def poll():
        restore()
        orig_poll()
    pipe._check_backbone_errors = poll
    try:
        for o, n in names:
            setattr(o, n, forbid)
        pipe._noise_offset = 0
        b = pipe.calc_bpd_loop(pipe.backbone, x0)
        for o, n in names:
            setattr(o, n, forbid)
        pipe.p_sample_loop(pipe.backbone, xshape)
        for o, n in names:
            setattr(o, n, forbid)
        pipe.ddim_sample_loop(pipe.backbone, xshape, eta=0.5)
    finally:
        restore()
    for k in ("total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["total_bpd"]).all()


def test_vlb_reduction_splits_samples_across_workgroups_b2_128cubed():
    """B = 2 at 128^3 (c5's geometry): each sample is reduced by many workgroups; the per-sample means agree with a float64 host
    evaluation and are bit-identical run to run."""
    from rho_diffusion_amd.diffusion.gaussian_diffusion import gd_table_rows, ModelVarType
    from rho_diffusion_amd.engine import ops
    pipe, _ = _pipeline("tiny3d", 20)
    shape = (2, 1, 128, 128, 128)
    xs = det_uniform(shape, "g18_big_x0", -1.0, 1.0)
    noise = det_normal(shape, "g18_big_noise")
    t = torch.tensor([0, 7])
    tab = torch.from_numpy(gd_table_rows(pipe.tables, ModelVarType.FIXED_LARGE)).to(DEV)
    xsd, nd, td = xs.to(DEV), noise.to(DEV), t.to(DEV)
    x_t = pipe.q_sample(xsd, td, noise=nd)
    mo = (xsd * 0.9 + 0.05 * nd).contiguous()
    outs = []
    for _ in range(2):
        vb, xm, ms, kl, nll = (torch.empty(2, device=DEV) for _ in range(5))
        ops.gd_vlb_terms(xsd, x_t, mo, td, tab, ops.GD_START_X, None, nd, vb, xm, ms, kl, nll)
        outs.append(torch.stack([vb, xm, ms, kl, nll]).cpu())
    assert torch.equal(outs[0], outs[1])
    # per-element terms in the kernel's float32 operation order (numpy), summed in float64 on the host
    r = _rows(pipe, t, 5)
    x, x0, xt_ = xs.numpy(), mo.cpu().numpy(), x_t.cpu().numpy()
    tm, mm = r["coef1"] * x + r["coef2"] * xt_, r["coef1"] * x0 + r["coef2"] * xt_
    lv1, lv2 = r["post_logvar"], r["model_logvar"]
    k0 = ((f32(-1) + lv2) - lv1) + np.exp(lv1 - lv2)
    kl = f32(0.5) * (k0 + ((tm - mm) * (tm - mm)) * np.exp(-lv2))
    kl64 = kl.astype(np.float64).reshape(2, -1).mean(1) / np.log(2.0)
    eps = (r["sqrt_recip"] * xt_ - x0) / r["sqrt_recipm1"]
    mse64 = ((eps - noise.numpy()) ** 2).astype(np.float64).reshape(2, -1).mean(1)
    xm64 = ((x0 - x) ** 2).astype(np.float64).reshape(2, -1).mean(1)
    got = outs[0].double().numpy()
    # KL: the per-sample constant holds two exps (a few ulp apart from numpy's); the sums themselves agree to ~1e-7
    assert np.all(np.abs(got[3] - kl64) / np.abs(kl64) <= 1e-4), (got[3], kl64)
    assert np.all(np.abs(got[1] - xm64) / xm64 <= 1e-6) and np.all(np.abs(got[2] - mse64) / mse64 <= 1e-6), (got[1:3], xm64, mse64)
    assert got[0][0] == got[4][0] and got[0][1] == got[3][1]            # vb = where(t == 0, nll, kl)


@pytest.mark.parametrize("case,T", CASES)
def test_training_losses_vs_reference(case, T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import ModelMeanType
    g = load_golden("g18_gaussian_api.npz")
    tag = f"{case}_T{T}"
    pipe, xshape = _pipeline(case, T)
    pipe.train()
    x0 = det_uniform(xshape, "g18_x0", -1.0, 1.0).to(DEV)
    tq = torch.from_numpy(g[f"{tag}/train_t"]).to(DEV)
    params = dict(pipe.backbone.named_parameters())
    for mt in ("START_X", "EPSILON"):
        pipe.model_mean_type = ModelMeanType[mt]
        pipe.backbone.zero_grad(set_to_none=True)
        terms = pipe.training_losses(pipe.backbone, x0, tq, noise=det_normal(xshape, "g18_train_noise").to(DEV))
        assert terms["loss"].shape == (xshape[0],) and terms["loss"] is terms["mse"]
        ref = torch.from_numpy(g[f"{tag}/train_{mt}/loss"])
        assert torch.allclose(terms["loss"].detach().cpu(), ref, rtol=2e-4, atol=1e-6), mt
        terms["loss"].mean().backward()
        for k in ("input_blocks.0.0.weight", "time_embed.0.weight", "out.2.weight", "out.2.bias"):
            got, want = grad_digest_of(params[k].grad), g[f"{tag}/train_{mt}/grad/{k}"]
            assert abs(got[0] - want[0]) <= 2e-3 * want[0], (mt, k, got[0], want[0])
            assert np.abs(got[2:] - want[2:]).max() <= 5e-3 * max(np.abs(want[2:]).max(), 1e-8), (mt, k)


def test_out_of_range_timestep_raises_at_the_poll():
    pipe, xshape = _pipeline("tiny2d", 20, "bf16")
    x = det_normal(xshape, "g18_xt").to(DEV)
    pipe.q_mean_variance(x, torch.tensor([3, 20], device=DEV))
    with pytest.raises(IndexError, match="outside"):
        pipe._check_backbone_errors()
    pipe._check_backbone_errors()                              # the flag was cleared
