"""-m gpu: DDPM(prediction_type=, snr_gamma=) end to end - the training step against the oracle, the defaults bit for bit, and sampling
on the spaced walk of a v / x0 model: analytic chain, graph replay against the eager loop, the all-T walk and a schedule whose
alpha_bar reaches 0.

Networks: tiny2d_multi / tiny2d with their golden-template weights (fp32 engine) as test_gpu_cfg_train.py and
test_gpu_spaced_sampling.py build them, T = 50, LinearSchedule(50, 1e-3, 0.02) (alpha_bar strictly positive), and an analytic
backbone without an engine.  Training bars: those of test_gpu_cfg_train.py - forward rel-L2 1e-4, loss within 2e-4 max(1, |ref|),
parameter gradients through that file's digest comparison."""
import math

import pytest
import torch
from torch import nn

from helpers import PARAM_SPACE, UNET_CASES, case_inputs, det_normal, det_state_dict, golden_template, load_golden, rel_l2
from gpu_util import DEV
from oracle import ref_torch as R
from test_gpu_cfg_train import CASE, KEEP, _compare_grads, _injected, _tiny_ddpm as _train_ddpm

pytestmark = pytest.mark.gpu

T = 50
BETAS = (1e-3, 0.02)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _schedule(steps=T):
    from rho_diffusion_amd.diffusion import LinearSchedule
    return LinearSchedule(steps, *BETAS)


def _tiny_ddpm(case="tiny2d", schedule=None, **kw):
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    g4 = load_golden("g4_unet.npz")
    cfg, xshape, ykind = UNET_CASES[case]
    schedule = _schedule() if schedule is None else schedule
    steps = len(schedule["alpha_bar_t"])
    ddpm = DDPM(UNet, dict(cfg, compute_dtype="fp32"), schedule, nn.MSELoss, timesteps=steps, **kw)
    if ykind == "multi":
        ddpm.backbone.cond_fn = MultiEmbeddings(parameter_space=PARAM_SPACE, embedding_dim=4 * cfg["model_channels"])
    ddpm.backbone.load_state_dict(det_state_dict(golden_template(g4, case), case))
    return ddpm.to(DEV), xshape


# ----------------------------------------------------------------------------- 1. training step against the oracle
def _weights64(ab: torch.Tensor, kind: str, gamma) -> torch.Tensor:
    """min-SNR-gamma in float64 on the float32 alpha_bar (0 < alpha_bar < 1 on this schedule); gamma None: ones."""
    ab = ab.float().double()
    if gamma is None:
        return torch.ones_like(ab)
    snr = ab / (1.0 - ab)
    capped = snr.clamp_max(gamma)
    return {"epsilon": capped / snr, "v": capped / (snr + 1.0), "sample": capped}[kind]


def _oracle(x0, eps, tq, kind, gamma, y_emb_of):
    """Loss, prediction and state-dict gradients of the oracle: R.q_sample + R.unet_forward + the weighted loss in torch."""
    g4 = load_golden("g4_unet.npz")
    cfg = dict(UNET_CASES[CASE][0])
    sd = {k: v.clone().requires_grad_(True) for k, v in det_state_dict(golden_template(g4, CASE), CASE).items()}
    ab = R.linear_schedule(T, *BETAS)["alpha_bar_t"]
    x_t = R.q_sample(x0, tq, eps, ab)
    pred = R.unet_forward(sd, cfg, x_t, tq, y_emb_of(sd))
    a = ab.float()[tq].view(-1, 1, 1, 1)
    target = {"epsilon": eps, "sample": x0, "v": a.sqrt() * eps - (1.0 - a).sqrt() * x0}[kind]
    w = _weights64(ab, kind, gamma)[tq].float().view(-1, 1, 1, 1)
    loss = (w * (pred - target) ** 2).mean()
    loss.backward()
    return loss.detach(), pred.detach(), sd


def _train_case(ops, kind, gamma, det=False, keep=None):
    _, _, _, y = case_inputs(CASE)
    old = ops.set_deterministic(det)
    try:
        ddpm, xshape = _train_ddpm(prediction_type=kind, snr_gamma=gamma, cond_drop_prob=0.5 if keep is not None else 0.0)
        x0, eps, tq = _injected(ddpm, xshape, keep=keep if keep is not None else [1, 1, 1])
        off0 = ddpm._noise_offset
        loss = ddpm.training_step([x0.to(DEV), y.to(DEV)])
        assert ddpm._noise_offset == off0                                   # everything random was injected
        loss.backward()
        pred = ddpm.backbone.engine()._last_train_plan.out.clone()
    finally:
        ops.set_deterministic(old)
    ddpm._check_nan(force=True)                                             # no bad timestep, no NaN
    mask = torch.tensor(keep if keep is not None else [1, 1, 1], dtype=torch.float32)
    ref_loss, ref_pred, sd = _oracle(x0, eps, tq, kind, gamma, lambda sd: R.multi_embeddings(y, PARAM_SPACE, sd) * mask[:, None])
    print(f"{kind} gamma={gamma} det={det} keep={keep}: forward rel_l2 {rel_l2(pred, ref_pred):.3e}, loss {loss.item():.6f} "
          f"ref {ref_loss.item():.6f} diff {abs(loss.item() - ref_loss.item()):.3e}")
    assert rel_l2(pred, ref_pred) < 1e-4
    assert abs(loss.item() - ref_loss.item()) < 2e-4 * max(1.0, abs(ref_loss.item()))
    _compare_grads(ddpm.backbone.named_parameters(), sd)
    return loss.item()


@pytest.mark.parametrize("kind,gamma", [("v", None), ("v", 5.0), ("sample", None), ("sample", 5.0), ("epsilon", 5.0), ("epsilon", 1.0),
                                        ("v", 1.0)])
def test_training_step_vs_oracle(ops, kind, gamma):
    """gamma = 5 is above the snr of all three injected timesteps (2.1, 0.07, 3e-4 at t = 7, 23, 41 of this schedule): the epsilon
    table is all ones there, the v and sample tables are not.  gamma = 1 caps the first of them."""
    ab = _schedule()["alpha_bar_t"].float().double()[torch.tensor([7, 23, 41])]
    snr = ab / (1.0 - ab)
    assert 1.0 < float(snr[0]) < 5.0 and float(snr[1]) < 1.0
    _train_case(ops, kind, gamma)


def test_training_step_vs_oracle_deterministic(ops):
    _train_case(ops, "v", 5.0, det=True)


def test_training_step_with_label_dropout_and_v_prediction(ops):
    _train_case(ops, "v", None, keep=KEEP)


def test_objectives_differ(ops):
    """The three objectives and the weighting give different losses on the same injected step (the switch is not ignored)."""
    losses = {(k, g): _loss_only(k, g) for k, g in (("epsilon", None), ("epsilon", 1.0), ("v", None), ("v", 5.0), ("sample", None))}
    vals = list(losses.values())
    assert len({round(v, 6) for v in vals}) == len(vals), losses


def _loss_only(kind, gamma):
    _, _, _, y = case_inputs(CASE)
    ddpm, xshape = _train_ddpm(prediction_type=kind, snr_gamma=gamma)
    x0, _, _ = _injected(ddpm, xshape, keep=[1, 1, 1])
    with torch.no_grad():
        return ddpm.training_step([x0.to(DEV), y.to(DEV)]).item()


def test_timestep_outside_the_table_raises_index_error(ops):
    """t on the device beyond the schedule: the loss kernel (and q_sample) set bit 2 of the polled flag; _check_nan raises."""
    _, _, _, y = case_inputs(CASE)
    ddpm, xshape = _train_ddpm(prediction_type="v", snr_gamma=5.0)
    x0, _, _ = _injected(ddpm, xshape, keep=[1, 1, 1])
    ddpm._draw_timesteps = lambda bs, device: torch.tensor([7, T + 3, 41], device=device)
    loss = ddpm.training_step([x0.to(DEV), y.to(DEV)])
    assert math.isfinite(loss.item())                                        # the clamped row was read
    with pytest.raises(IndexError):
        ddpm._check_nan(force=True)


# ----------------------------------------------------------------------------- 2. defaults unchanged
def test_defaults_issue_the_launches_of_before(ops, monkeypatch):
    """DDPM(...) and DDPM(..., prediction_type="epsilon", snr_gamma=None): the same bits in loss, gradients and a 5-step
    reverse_process, the same Philox offsets - and neither new entry point is called."""
    _, _, _, y = case_inputs(CASE)

    def boom(*a, **k):
        raise AssertionError("the default path reached a prediction-type kernel")

    monkeypatch.setattr(ops, "pred_loss", boom)
    monkeypatch.setattr(ops, "p_sample_step_spaced_pred", boom)
    old = ops.set_deterministic(True)                                        # ordered gradient sums: bits are comparable
    try:
        outs = []
        for kw in (dict(), dict(prediction_type="epsilon", snr_gamma=None)):
            ddpm, xshape = _train_ddpm(**kw)
            torch.manual_seed(1234)                                          # the CPU draw of the timesteps
            x0 = det_normal(xshape, "preddef_x0")
            loss = ddpm.training_step([x0.to(DEV), y.to(DEV)])
            off_train = ddpm._noise_offset
            loss.backward()
            grads = {n: p.grad.clone() for n, p in ddpm.backbone.named_parameters() if p.grad is not None}
            ddpm.eval()
            res = ddpm.reverse_process(torch.zeros(xshape, device=DEV), y.to(DEV), num_steps=5, eta=0.5)
            outs.append((loss.detach().clone(), grads, res["denoised"].clone(), off_train, ddpm._noise_offset))
    finally:
        ops.set_deterministic(old)
    a, b = outs
    assert torch.equal(a[0], b[0]) and a[3] == b[3] > 0 and a[4] == b[4] > a[3]
    assert a[1].keys() == b[1].keys() and len(a[1]) > 20 and all(torch.equal(a[1][n], b[1][n]) for n in a[1])
    assert torch.equal(a[2], b[2]) and torch.isfinite(a[2]).all()


# ----------------------------------------------------------------------------- 3. analytic backbone
class _Analytic(nn.Module):
    """The optimal v- or x0-prediction for iid N(0, s^2) data, a known multiple of x: with D = ab s^2 + 1 - ab,
    x0 = sqrt(ab) s^2 x / D and eps = sqrt(1 - ab) x / D, so v = sqrt(ab) eps - sqrt(1 - ab) x0 = sqrt(ab (1 - ab)) (1 - s^2) x / D.
    float64 cast to float32.  No engine: reverse_process calls it with a [B] tensor of the timestep."""

    def __init__(self, s: float, kind: str, steps: int = T):
        super().__init__()
        self.s2, self.kind = s * s, kind
        self.ab = _schedule(steps)["alpha_bar_t"].float().double()
        self.calls = []

    def gain(self, t: int) -> float:
        ab = float(self.ab[t])
        D = ab * self.s2 + 1.0 - ab
        return math.sqrt(ab) * self.s2 / D if self.kind == "sample" else math.sqrt(ab * (1.0 - ab)) * (1.0 - self.s2) / D

    def forward(self, x, t, c=None):
        ts = t.tolist()
        assert len(set(ts)) == 1 and len(ts) == x.shape[0] and t.dtype == torch.long and t.device == x.device
        self.calls.append(ts[0])
        return (self.gain(ts[0]) * x.double()).float()


def _taus(S):
    return [T - 1] if S == 1 else [(2 * i * (T - 1) + (S - 1)) // (2 * (S - 1)) for i in range(S)]


@pytest.mark.parametrize("kind", ["v", "sample"])
@pytest.mark.parametrize("S", [1, 2, 5, 20])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_analytic_backbone_chain_is_the_float64_recursion(S, eta, kind):
    """With clip_denoised=False the chain is linear in the noise tape: per step x' = M_k x + sigma_k z_k, g_k the backbone's gain at
    tau_k.  The same recursion runs here in float64 on the float32 rows.  The bound is set the way
    test_gpu_spaced_sampling.py::test_analytic_backbone_chain_is_the_float64_recursion sets its own, per element and not chosen by
    trial: a step adds the first-order bound of test_gpu_pred_step.py without clip, with |p| standing for the cast of the
    prediction to float32 (Ep = |p|), each rounding at most U = 2^-24 of its value -
        v:       d_k = U [ (ce sa + sp sb) |p| + sp (|m| + |x0|) + ce (|u| + |ep|) + |w| + |t| + |r| ],   M_k = sp (sa - sb g) + ce (sb + sa g)
        sample:  d_k = U [ (sp + ce iv sa) |p| + ce iv |q| + ce |ep| + |w| + |t| + |r| ],                   M_k = sp g + ce iv (1 - sa g)
        row 0:   d_0 = U [ sp E0 + |r| ],  E0 = sb |p| + |m| + |x0| (v) or |p| (sample),                    M_0 = sp (sa - sb g) or sp g
    - and carries the error it received through |M_k|:  E <- |M_k| E + d_k, S times, from E = 0 at the tape's x_T.  The factor
    1.001 covers the second-order terms."""
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.diffusion.prediction import spaced_pred_coefficients
    shape = (2, 1, 8, 8)
    ddpm = DDPM(_Analytic, dict(s=0.5, kind=kind), _schedule(), nn.MSELoss, timesteps=T, prediction_type=kind)
    net = ddpm.backbone
    assert not hasattr(net, "engine")
    tape = [det_normal(shape, f"predtape_{i}") for i in range(S)]
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

    rows = spaced_pred_coefficients(_schedule()["alpha_bar_t"], taus, eta, kind).double()
    x = tape[0].double()
    err = torch.zeros_like(x)
    zi = 1
    for k in range(S - 1, -1, -1):
        sa, sb, iv, sp, sg, ce = (float(v) for v in rows[k][:6])
        g = net.gain(taus[k])
        p = g * x
        if eta > 0 and k >= 1:
            w = sg * tape[zi].double()
            zi += 1
        else:
            w = torch.zeros_like(x)
        if kind == "v":
            m = sb * p
            x0 = sa * x - m
            E0 = sb * p.abs() + m.abs() + x0.abs()
        else:
            x0 = p
            E0 = p.abs()
        if ce == 0.0 and sg == 0.0:                                   # row 0: the x0 estimate itself
            r = sp * x0
            step = sp * E0 + r.abs()
            M = sp * (sa - sb * g) if kind == "v" else sp * g
        elif kind == "v":
            u = sa * p
            ep = sb * x + u
            t = ce * ep + w
            r = sp * x0 + t
            step = (ce * sa + sp * sb) * p.abs() + sp * (m.abs() + x0.abs()) + ce * (u.abs() + ep.abs()) + w.abs() + t.abs() + r.abs()
            M = sp * (sa - sb * g) + ce * (sb + sa * g)
        else:
            q = x - sa * x0
            ep = q * iv
            t = ce * ep + w
            r = sp * x0 + t
            step = (sp + ce * iv * sa) * p.abs() + ce * iv * q.abs() + ce * ep.abs() + w.abs() + t.abs() + r.abs()
            M = sp * g + ce * iv * (1.0 - sa * g)
        err = abs(M) * err + 1.001 * U * step
        x = r
    got = res["denoised"].double().cpu()
    excess = (got - x).abs() - err
    print(f"analytic chain {kind} S={S} eta={eta}: max err {float((got - x).abs().max()):.3e}, max bound {float(err.max()):.3e}, "
          f"max |x| {float(x.abs().max()):.3e}")
    assert torch.isfinite(got).all() and float(excess.max()) <= 0.0, (S, eta, float(excess.max()))
    assert float(err.max()) < 1e-2 * float(x.abs().max())              # the bound stays far below the result's own scale


# ----------------------------------------------------------------------------- 4. graph against eager
@pytest.mark.parametrize("env", ["0", "1"])
@pytest.mark.parametrize("eta,scale", [(0.0, None), (0.5, None), (0.0, 3.0), (0.5, 3.0)])
def test_graph_replay_matches_eager_loop(monkeypatch, env, eta, scale):
    """The captured step (Philox draw when eta > 0, forward, rho_p_sample_step_spaced_pred, spaced advance) replayed S - 1 times is the
    eager loop bit for bit, checkpoints and RNG bookkeeping included - whatever RHO_HIP_GRAPH the pipelines were built under."""
    monkeypatch.setenv("RHO_HIP_GRAPH", env)
    B = UNET_CASES[CASE][1][0]
    y = R.discrete_parameter_rows(PARAM_SPACE, B).to(DEV)
    outs = {}
    for mode in (True, False):
        ddpm, xshape = _tiny_ddpm(CASE, prediction_type="v")
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
    # the same walk read as an epsilon model is another result: the kernel follows the attribute
    other, xshape = _tiny_ddpm(CASE)
    ro = other.reverse_process(torch.zeros(xshape, device=DEV), y, guidance_scale=scale, num_steps=5, eta=eta)
    assert not torch.equal(ro["denoised"], outs[True][0])


# ----------------------------------------------------------------------------- 5. the all-T walk
def test_no_num_steps_walks_every_timestep():
    """prediction_type "v": num_steps None is taus = range(T) on the spaced walk, bit for bit, with eta from sampling_eta; the
    backbone is evaluated at T-1 .. 0; clip_denoised=False is accepted; generate() follows the attribute."""
    from rho_diffusion_amd.diffusion import DDPM
    shape = (2, 1, 8, 8)
    outs = []
    for kw in (dict(), dict(num_steps=range(T)), dict(clip_denoised=False)):
        ddpm = DDPM(_Analytic, dict(s=0.5, kind="v"), _schedule(), nn.MSELoss, timesteps=T, prediction_type="v", sampling_eta=0.5)
        res = ddpm.reverse_process(torch.zeros(shape, device=DEV), **kw)
        assert ddpm.backbone.calls == list(range(T - 1, -1, -1))
        assert ddpm._noise_offset == ((res["denoised"].numel() + 3) // 4) * T          # x_T and one z per k >= 1
        assert torch.isfinite(res["denoised"]).all()
        outs.append(res["denoised"].clone())
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) <= 1.0
    # with the engine and the captured graph
    a, xshape = _tiny_ddpm("tiny2d", prediction_type="v", sampling_batch_size=UNET_CASES["tiny2d"][1][0])
    out = a.generate()
    b, _ = _tiny_ddpm("tiny2d", prediction_type="v")
    rb = b.reverse_process(torch.zeros(xshape, device=DEV), num_steps=range(T), eta=0.0)
    assert torch.equal(out, rb["denoised"]) and a._noise_offset == b._noise_offset == (out.numel() + 3) // 4
    assert a.hip_graph_sampling and b.hip_graph_sampling and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
    assert [k[2] for k in a._spaced_cache] == ["v"]


# ----------------------------------------------------------------------------- 6. a schedule that ends without signal
def test_alpha_bar_zero_is_sampled_by_v_and_refused_by_epsilon():
    from rho_diffusion_amd.diffusion import LinearSchedule
    sched = LinearSchedule(20, 1e-3, 0.02)
    ab = sched["alpha_bar_t"].float()
    assert float(ab[19]) == 0.0 and float(ab[18]) > 0.0                       # checked here on the CPU: exactly 0 at t = 19
    eps, xshape = _tiny_ddpm("tiny2d", schedule=LinearSchedule(20, 1e-3, 0.02))
    x = torch.zeros(xshape, device=DEV)
    with pytest.raises(ValueError, match="timestep 19"):
        eps.reverse_process(x, num_steps=20)
    assert eps._noise_offset == 0
    for kind in ("v", "sample"):
        for kw in (dict(), dict(num_steps=5, eta=0.5), dict(num_steps=20, eta=1.0, clip_denoised=False)):
            ddpm, _ = _tiny_ddpm("tiny2d", schedule=LinearSchedule(20, 1e-3, 0.02), prediction_type=kind)
            out = ddpm.reverse_process(x, **kw)["denoised"]
            assert torch.isfinite(out).all(), (kind, kw)
            if kw.get("clip_denoised", True):
                assert float(out.abs().max()) <= 1.0, (kind, kw)
