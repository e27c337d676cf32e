"""-m gpu: DDPM.reverse_process(num_steps=, eta=) - few-step sampling on a spaced timestep sequence (DDIM with eta), in the eager
loop and in the captured HIP graph, plain and under classifier-free guidance.

Networks: tiny2d_multi / tiny2d with their golden-template weights (fp32 engine), as test_gpu_cfg_sampling.py builds them, and an
analytic backbone without an engine.  Schedule: LinearSchedule(20, 1e-3, 0.01), whose alpha_bar is strictly positive - (1e-3, 0.02)
ends at alpha_bar[19] == 0, where no x0 estimate exists and the sampler refuses (test_spaced_host.py)."""
import math

import pytest
import torch
from torch import nn

from helpers import PARAM_SPACE, UNET_CASES, det_normal, det_state_dict, golden_template, load_golden, rel_l2
from gpu_util import DEV
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

CASE = "tiny2d_multi"
T = 20
BETAS = (1e-3, 0.01)
CHAIN_BAR = 2e-3                   # the project's unguided-chain bar for this network and engine (test_gpu_round2.py)
U = 2.0 ** -24
COMBOS = [(0.0, None), (0.5, None), (0.0, 3.0), (0.5, 3.0)]          # (eta, guidance_scale)


def _schedule():
    from rho_diffusion_amd.diffusion import LinearSchedule
    return LinearSchedule(T, *BETAS)


def _tiny_ddpm(case=CASE, **kw):
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    g4 = load_golden("g4_unet.npz")
    cfg, xshape, ykind = UNET_CASES[case]
    ddpm = DDPM(UNet, dict(cfg, compute_dtype="fp32"), _schedule(), nn.MSELoss, timesteps=T, **kw)
    if ykind == "multi":
        ddpm.backbone.cond_fn = MultiEmbeddings(parameter_space=PARAM_SPACE, embedding_dim=4 * cfg["model_channels"])
    ddpm.backbone.load_state_dict(det_state_dict(golden_template(g4, case), case))
    return ddpm.to(DEV), xshape


def _labels(B):
    return R.discrete_parameter_rows(PARAM_SPACE, B)


def _taus(S):
    return [T - 1] if S == 1 else [(2 * i * (T - 1) + (S - 1)) // (2 * (S - 1)) for i in range(S)]


# ----------------------------------------------------------------------------- 1. analytic backbone
class _Analytic(nn.Module):
    """The optimal eps-prediction for iid N(0, s^2) data: eps = sqrt(1 - ab_t) x / (ab_t s^2 + 1 - ab_t), float64 cast to float32.
    No engine: reverse_process calls it with a [B] tensor of the timestep."""

    def __init__(self, s: float):
        super().__init__()
        self.s2 = s * s
        self.ab = _schedule()["alpha_bar_t"].double()
        self.calls = []

    def gain(self, t: int) -> float:
        ab = float(self.ab[t])
        return math.sqrt(1.0 - ab) / (ab * self.s2 + 1.0 - ab)

    def forward(self, x, t, c=None):
        ts = t.tolist()
        assert len(set(ts)) == 1 and len(ts) == x.shape[0] and t.dtype == torch.long and t.device == x.device
        self.calls.append(ts[0])
        return (self.gain(ts[0]) * x.double()).float()


@pytest.mark.parametrize("S", [1, 2, 5, 20])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_analytic_backbone_chain_is_the_float64_recursion(S, eta):
    """With clip_denoised=False the chain is linear in the noise tape: per step x' = M_k x + sigma_k z_k with
    M_k = sqrt_abp (c_recip - c_recipm1 g_k) + coef_eps g_k, g_k the backbone's gain at tau_k.  The same recursion runs here in
    float64 on the float32 rows.  Bound, per element, not chosen by trial: the device chain rounds six times per step - the cast of
    the prediction e to float32, m = c_recipm1 e, x0 = fma(c_recip, x, -m), w = sigma z, v = fma(coef_eps, e, w),
    r = fma(sqrt_abp, x0, v) - each by at most U = 2^-24 of its value; to first order a step adds
        d_k = U [ (coef_eps + sqrt_abp c_recipm1) |e| + sqrt_abp (|m| + |x0|) + |w| + |v| + |r| ]
    (the bound of test_gpu_spaced_step.py without clip, |e| standing for the cast) and carries the error it received through
    |M_k|:  E <- |M_k| E + d_k, S times, from E = 0 at the tape's x_T.  The factor 1.001 covers the second-order terms."""
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients
    shape = (2, 1, 8, 8)
    ddpm = DDPM(_Analytic, dict(s=0.5), _schedule(), nn.MSELoss, timesteps=T)
    net = ddpm.backbone
    assert not hasattr(net, "engine")
    tape = [det_normal(shape, f"spacedtape_{i}") for i in range(S)]
    it = iter(tape)
    drawn = []

    def noise(data):
        drawn.append(tuple(data.shape))
        return next(it).to(DEV).clone()

    ddpm.noise = noise
    res = ddpm.reverse_process(torch.zeros(shape, device=DEV), num_steps=S, eta=eta, clip_denoised=False)
    taus = _taus(S)
    assert net.calls == taus[::-1]
    assert drawn == [shape] * (1 + (S - 1) * (eta > 0))
    assert res["buffer"] is None

    rows = spaced_coefficients(_schedule()["alpha_bar_t"], taus, eta).double()
    x = tape[0].double()
    err = torch.zeros_like(x)
    zi = 1
    for k in range(S - 1, -1, -1):
        c0, c1, _, _, sp, sg, ce = (float(v) for v in rows[k][:7])
        g = net.gain(taus[k])
        e = g * x
        m = c1 * e
        x0 = c0 * x - m
        if eta > 0 and k >= 1:
            w = sg * tape[zi].double()
            zi += 1
        else:
            w = torch.zeros_like(x)
        if ce == 0.0 and sg == 0.0:                                   # row 0: the x0 estimate itself
            r = sp * x0
            step = sp * (c1 * e.abs() + m.abs() + x0.abs()) + r.abs()
            M = sp * (c0 - c1 * g)
        else:
            v = ce * e + w
            r = sp * x0 + v
            step = (ce + sp * c1) * e.abs() + sp * (m.abs() + x0.abs()) + w.abs() + v.abs() + r.abs()
            M = sp * (c0 - c1 * g) + ce * g
        err = abs(M) * err + 1.001 * U * step
        x = r
    got = res["denoised"].double().cpu()
    excess = (got - x).abs() - err
    print(f"analytic chain S={S} eta={eta}: max err {float((got - x).abs().max()):.3e}, max bound {float(err.max()):.3e}, "
          f"max |x| {float(x.abs().max()):.3e}")
    assert torch.isfinite(got).all() and float(excess.max()) <= 0.0, (S, eta, float(excess.max()))
    assert float(err.max()) < 1e-2 * float(x.abs().max())              # the bound stays far below the result's own scale


# ----------------------------------------------------------------------------- 2. eager loop against a hand composition
def _hand_chain(ddpm, xshape, y, S, eta, scale, checkpoints):
    """The spaced walk composed here from engine.forward and the C entry points, Philox draws at the offsets of the eager loop."""
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.diffusion.spaced import spaced_checkpoints, spaced_coefficients
    lib, st = hip.lib(), hip.stream
    B = xshape[0]
    n = int(torch.tensor(xshape).prod())
    delta = (n + 3) // 4
    seed, off = ddpm.noise_seed, 0
    x = torch.empty(xshape, dtype=torch.float32, device=DEV)
    hip.check(lib.rho_philox_normal(x.data_ptr(), n, seed, off, None, st()), "rho_philox_normal")
    off += delta
    cc = ddpm._preembed_conditions(y)
    guided = scale is not None
    if guided:
        cc = torch.cat([cc.float(), torch.zeros_like(cc.float())]).contiguous()
        x_all = torch.cat([x, x])
    else:
        x_all = x
    taus = _taus(S)
    rows = spaced_coefficients(ddpm.schedule["alpha_bar_t"], taus, eta).to(DEV)
    taus_dev = torch.tensor(taus, dtype=torch.int32, device=DEV)
    k_dev = torch.tensor([S - 1], dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([taus[-1]], dtype=torch.int32, device=DEV)
    ck = spaced_checkpoints(T, taus)
    buf = torch.zeros((B, checkpoints) + tuple(xshape[1:]), dtype=torch.float32, device=DEV)
    slot = 0
    eng = ddpm.backbone.engine()
    with torch.no_grad():
        for k in range(S - 1, -1, -1):
            z = None
            if eta > 0 and k >= 1:
                z = torch.empty(xshape, dtype=torch.float32, device=DEV)
                hip.check(lib.rho_philox_normal(z.data_ptr(), n, seed, off, None, st()), "rho_philox_normal")
                off += delta
            pred = eng.forward(x_all, None, cc, t_scalar_dev=t_dev).contiguous()
            hip.check(lib.rho_p_sample_step_spaced(x_all.data_ptr(), pred.data_ptr(), z.data_ptr() if z is not None else None,
                                                   rows.data_ptr(), k_dev.data_ptr(), S, n, int(guided), float(scale or 0.0), 1, st()),
                      "rho_p_sample_step_spaced")
            if taus[k] in ck and slot < checkpoints:
                buf[:, slot].copy_(x_all[:B])
                slot += 1
            hip.check(lib.rho_spaced_advance(k_dev.data_ptr(), t_dev.data_ptr(), taus_dev.data_ptr(), None, 0, st()), "rho_spaced_advance")
    assert int(k_dev.item()) == -1 and int(t_dev.item()) == taus[0]
    return x_all[:B].clone(), buf, off


@pytest.mark.parametrize("eta,scale", COMBOS)
def test_eager_loop_is_the_hand_composition(eta, scale):
    S = 5
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    ddpm, xshape = _tiny_ddpm()
    ddpm.hip_graph_sampling = False
    res = ddpm.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=scale, num_steps=S, eta=eta)
    hand, _ = _tiny_ddpm()
    den, buf, off = _hand_chain(hand, tuple(xshape), y, S, eta, scale, 3)
    assert torch.equal(res["denoised"], den) and torch.equal(res["buffer"], buf)
    assert ddpm._noise_offset == off == ((den.numel() + 3) // 4) * (1 + (S - 1) * (eta > 0))
    assert tuple(res["denoised"].shape) == tuple(xshape) and tuple(res["buffer"].shape) == (B, 3) + tuple(xshape[1:])
    assert torch.isfinite(den).all() and float(den.abs().max()) <= 1.0          # step 0 returns the clamped x0 estimate
    assert float(buf[:, 2].abs().sum()) > 0 and not torch.equal(buf[:, 0], buf[:, 1])


# ----------------------------------------------------------------------------- 3. graph against eager
@pytest.mark.parametrize("env", ["0", "1"])
@pytest.mark.parametrize("eta,scale", COMBOS)
def test_graph_replay_matches_eager_loop(monkeypatch, env, eta, scale):
    """The captured step (Philox draw when eta > 0, forward, spaced update, spaced advance) replayed S - 1 times is the eager loop bit
    for bit, checkpoints and RNG bookkeeping included - whatever RHO_HIP_GRAPH the pipelines were built under."""
    monkeypatch.setenv("RHO_HIP_GRAPH", env)
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    outs = {}
    for mode in (True, False):
        ddpm, xshape = _tiny_ddpm()
        assert ddpm.hip_graph_sampling == (env == "1")
        ddpm.hip_graph_sampling = mode
        res = ddpm.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=scale, num_steps=5, eta=eta)
        assert ddpm.hip_graph_sampling == mode             # the capture did not fall back
        outs[mode] = (res["denoised"].clone(), res["buffer"].clone(), ddpm._noise_offset)
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1], outs[False][1])
    assert outs[True][2] == outs[False][2] == ((outs[True][0].numel() + 3) // 4) * (1 + 4 * (eta > 0))
    assert torch.isfinite(outs[True][0]).all() and float(outs[True][0].abs().max()) <= 1.0
    assert float(outs[True][1].abs().sum()) > 0


# ----------------------------------------------------------------------------- 4. oracle chain
def _oracle_chain(model, x_init, z_tape, S, eta, num_checkpoints):
    """The spaced update restated in float64 torch around the oracle network: coefficients from the oracle's own schedule tables,
    x0 clamped, eps re-derived from the clamped x0, checkpoints by the first-visited-at-or-above rule."""
    ab_all = R.linear_schedule(T, *BETAS)["alpha_bar_t"].float().double()
    taus = _taus(S)
    spc = T // 10
    ck = {min(t for t in taus if t >= m) for m in range(0, T, spc) if any(t >= m for t in taus)}
    x = x_init.double()
    B = x.shape[0]
    buf = torch.zeros((B, num_checkpoints) + tuple(x.shape[1:]), dtype=torch.float64)
    zi, slot = 0, 0
    for k in range(S - 1, -1, -1):
        ab = ab_all[taus[k]]
        abp = ab_all[taus[k - 1]] if k > 0 else torch.tensor(1.0, dtype=torch.float64)
        z = None
        if eta > 0 and k >= 1:
            z = z_tape[zi].double()
            zi += 1
        eps = model(x.float(), torch.full((B,), taus[k], dtype=torch.long)).double()
        x0 = (torch.sqrt(1 / ab) * x - torch.sqrt(1 / ab - 1) * eps).clamp(-1.0, 1.0)
        if k == 0:
            x = x0
        else:
            eps = (x - torch.sqrt(ab) * x0) / torch.sqrt(1 - ab)
            sigma = eta * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
            x = torch.sqrt(abp) * x0 + torch.sqrt((1 - abp - sigma ** 2).clamp_min(0.0)) * eps
            if z is not None:
                x = x + sigma * z
        if taus[k] in ck and slot < num_checkpoints:
            buf[:, slot] = x
            slot += 1
    return x, buf


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_spaced_chain_vs_oracle(eta):
    """generate() with sampling_steps = 5 against the float64 restatement around R.unet_forward, same noise tape.  Bar: the
    unguided chain's 2e-3 (that bar covers 20 evaluations of this network; this chain makes 5)."""
    S = 5
    g4 = load_golden("g4_unet.npz")
    cfg = dict(UNET_CASES[CASE][0])
    sd = det_state_dict(golden_template(g4, CASE), CASE)
    gshape = UNET_CASES[CASE][1]
    B = gshape[0]
    tape = [det_normal(gshape, f"gentape_{i}") for i in range(S)]
    labels = _labels(B)
    with torch.no_grad():
        ref, ref_buf = _oracle_chain(lambda x, t: R.unet_forward(sd, cfg, x, t, labels, PARAM_SPACE), tape[0], tape[1:], S, eta, 3)
    ddpm, _ = _tiny_ddpm(sampling_batch_size=B, sample_parameter_space=PARAM_SPACE, sampling_steps=S, sampling_eta=eta,
                         t_checkpoints=[0, 1, 2])
    it = iter([t.to(DEV) for t in tape])
    drawn = []

    def noise(data):
        drawn.append(tuple(data.shape))
        return next(it).clone()

    ddpm.noise = noise
    out = ddpm.generate()
    den, buf = ddpm.last_samples["denoised"], ddpm.last_samples["buffer"]
    assert out is den and tuple(den.shape) == tuple(gshape)
    assert drawn == [tuple(gshape)] * (1 + (S - 1) * (eta > 0))
    print(f"spaced chain S={S} eta={eta}: rel_l2 denoised {rel_l2(den, ref):.3e}, buffer {rel_l2(buf, ref_buf):.3e} (bar {CHAIN_BAR:.1e})")
    assert float(ref.abs().max()) <= 1.0 and float(ref_buf.abs().sum()) > 0
    assert rel_l2(den, ref) < CHAIN_BAR
    assert rel_l2(buf, ref_buf) < CHAIN_BAR


# ----------------------------------------------------------------------------- 5. defaults and refusals
def test_no_num_steps_is_the_full_loop():
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    a, xshape = _tiny_ddpm()
    ra = a.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2])
    b, _ = _tiny_ddpm(sampling_steps=None, sampling_eta=0.0)
    rb = b.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], num_steps=None, eta=None, clip_denoised=True)
    assert torch.equal(ra["denoised"], rb["denoised"]) and torch.equal(ra["buffer"], rb["buffer"])
    assert a._noise_offset == b._noise_offset == ((ra["denoised"].numel() + 3) // 4) * (T - 1)     # x_T and one z per t > 1
    assert a.hip_graph_sampling and b.hip_graph_sampling
    # an eta without num_steps changes nothing either: it belongs to the spaced walk
    c, _ = _tiny_ddpm(sampling_eta=0.5)
    rc = c.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2])
    assert torch.equal(ra["denoised"], rc["denoised"]) and torch.equal(ra["buffer"], rc["buffer"]) and c._noise_offset == a._noise_offset


def test_constructor_attributes_reach_generate():
    B = UNET_CASES[CASE][1][0]
    a, xshape = _tiny_ddpm(sampling_batch_size=B, sample_parameter_space=PARAM_SPACE, sampling_steps=5, sampling_eta=0.5)
    out = a.generate()
    b, _ = _tiny_ddpm()
    rb = b.reverse_process(torch.zeros(xshape, device=DEV), _labels(B).to(DEV), num_steps=5, eta=0.5)
    assert torch.equal(out, rb["denoised"]) and a._noise_offset == b._noise_offset == ((out.numel() + 3) // 4) * 5
    assert a.hip_graph_sampling and b.hip_graph_sampling                     # the captured graph served both
    # the per-call values override the attributes
    rc = a.reverse_process(torch.zeros(xshape, device=DEV), _labels(B).to(DEV), num_steps=[0, 5, 10, 14, 19], eta=0.0)
    assert a._noise_offset == ((out.numel() + 3) // 4) * 6                   # eta = 0: x_T only
    assert not torch.equal(rc["denoised"], out)
    # the rows were built once per (taus, eta) and uploaded once
    assert len(a._spaced_cache) == 2 and all(len(v["dev"]) == 1 for v in a._spaced_cache.values())
    a.reverse_process(torch.zeros(xshape, device=DEV), _labels(B).to(DEV))
    assert len(a._spaced_cache) == 2


def test_refusals_come_before_any_draw():
    ddpm, xshape = _tiny_ddpm("tiny2d")
    x = torch.zeros(xshape, device=DEV)
    off = ddpm._noise_offset
    for kw in (dict(num_steps=T + 1), dict(num_steps=0), dict(num_steps=[3, 3]), dict(num_steps=[5, 2]), dict(num_steps=[0, T]),
               dict(num_steps=5, eta=-0.1), dict(clip_denoised=False)):
        with pytest.raises(ValueError):
            ddpm.reverse_process(x, **kw)
        assert ddpm._noise_offset == off, kw
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    zero = DDPM(UNet, dict(UNET_CASES["tiny2d"][0], compute_dtype="fp32"), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T).to(DEV)
    with pytest.raises(ValueError, match="timestep 19"):
        zero.reverse_process(x, num_steps=5)
    assert zero._noise_offset == 0
    out = zero.reverse_process(x, num_steps=range(0, 19, 3))["denoised"]      # an explicit sequence that stops below it is taken
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0 and zero._noise_offset == (out.numel() + 3) // 4


def test_reproducible_from_the_philox_seed_and_step_count_matters():
    outs = []
    for steps in (5, 5, 20):
        ddpm, xshape = _tiny_ddpm("tiny2d", sampling_batch_size=UNET_CASES["tiny2d"][1][0], sampling_steps=steps, sampling_eta=0.5)
        out = ddpm.generate()
        assert tuple(out.shape) == tuple(xshape) and out.device.type == "cuda"
        assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
        assert ddpm.hip_graph_sampling
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    assert rel_l2(outs[0], outs[2]) > 1e-2
