"""-m gpu: DDPM(sampler="dpmpp_2m") / reverse_process_with(sampler="dpmpp_2m") end to end - the analytic chain against the float64 two-term recursion, the
accuracy it buys over the first-order walk on the device, graph replay against the eager loop, checkpoints, the defaults bit for
bit, the refusals and a schedule whose alpha_bar reaches 0.

Networks: tiny2d_multi / tiny2d with their golden-template weights (fp32 engine) as test_gpu_pred_pipeline.py builds them, T = 50,
LinearSchedule(50, 1e-3, 0.02) (alpha_bar strictly positive), and an analytic backbone without an engine."""
import math

import pytest
import torch
from torch import nn

from helpers import PARAM_SPACE, UNET_CASES, det_normal, det_state_dict, golden_template, load_golden
from gpu_util import DEV
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

T = 50
BETAS = (1e-3, 0.02)
U = 2.0 ** -24
CASE = "tiny2d_multi"


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _schedule(steps=T, betas=BETAS):
    from rho_diffusion_amd.diffusion import LinearSchedule
    return LinearSchedule(steps, *betas) if betas else LinearSchedule(steps)


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


class _Analytic(nn.Module):
    """The optimal prediction for iid N(0, s^2) data, a known multiple of x: with D = ab s^2 + 1 - ab, x0 = sqrt(ab) s^2 x / D,
    eps = sqrt(1 - ab) x / D and v = sqrt(ab) eps - sqrt(1 - ab) x0 = sqrt(ab (1 - ab)) (1 - s^2) x / D.  float64 cast to float32.
    No engine: reverse_process calls it with a [B] tensor of the timestep.  ``inputs`` keeps a copy of every x it was given."""

    def __init__(self, s: float, kind: str, steps: int = T, betas=BETAS):
        super().__init__()
        self.s2, self.kind = s * s, kind
        self.ab = _schedule(steps, betas)["alpha_bar_t"].float().double()
        self.calls, self.inputs = [], []

    def D(self, t: int) -> float:
        ab = float(self.ab[t])
        return ab * self.s2 + 1.0 - ab

    def gain(self, t: int) -> float:
        ab = float(self.ab[t])
        if self.kind == "sample":
            return math.sqrt(ab) * self.s2 / self.D(t)
        if self.kind == "epsilon":
            return math.sqrt(1.0 - ab) / self.D(t)
        return math.sqrt(ab * (1.0 - ab)) * (1.0 - self.s2) / self.D(t)

    def forward(self, x, t, c=None):
        ts = t.tolist()
        assert len(set(ts)) == 1 and len(ts) == x.shape[0] and t.dtype == torch.long and t.device == x.device
        self.calls.append(ts[0])
        self.inputs.append(x.detach().clone())
        return (self.gain(ts[0]) * x.double()).float()


# ----------------------------------------------------------------------------- 1. analytic backbone
@pytest.mark.parametrize("kind", ["epsilon", "v", "sample"])
@pytest.mark.parametrize("S", [1, 2, 5, 20])
def test_analytic_backbone_chain_is_the_float64_recursion(S, kind):
    """With clip_denoised=False the chain is linear in x_T: per step, with g_k the backbone's gain at tau_k and G_k = a_x - a_p g_k
    (g_k for "sample") the gain of the x0 estimate,
        x0_k = G_k x,    x' = c_x x + c_d0 x0_k + c_d1 x0_{k+1},    hist <- x0_k.
    The same two-term recursion runs here in float64 on the float32 rows.  The bound is built the way
    test_gpu_pred_pipeline.py::test_analytic_backbone_chain_is_the_float64_recursion builds its own, per element and not chosen by
    trial: a step adds the first-order bound of test_gpu_dpmpp_step.py, with |p| standing for the cast of the prediction to float32
    (Ep = |p|), each rounding at most U = 2^-24 of its value, and carries the errors it received - Ex of x, Eh of hist - through the
    absolute values of the coefficients of the recurrence:
        E0  = a_p |p| + |m| + |x0|   (epsilon, v)        E0 = |p|   (sample)
        Ex0 = |G_k| Ex + U E0
        Ex' = |c_x| Ex + |c_d0| Ex0 + |c_d1| Eh + U (|w| + |t| + |r|)      second order
        Ex' = |c_x| Ex + |c_d0| Ex0 + U (|u| + |r|)                          first order;  |c_d0| Ex0 + U |r| where c_x == 0
        Eh' = Ex0
    from Ex = 0 at the tape's x_T.  The factor 1.001 covers the second-order terms."""
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients, logsnr_timesteps
    shape = (2, 1, 8, 8)
    ddpm = DDPM(_Analytic, dict(s=0.5, kind=kind), _schedule(), nn.MSELoss, timesteps=T, prediction_type=kind, sampler="dpmpp_2m")
    net = ddpm.backbone
    assert not hasattr(net, "engine")
    x_T = det_normal(shape, "dpmpptape_0")
    drawn = []

    def noise(data):
        drawn.append(tuple(data.shape))
        assert len(drawn) == 1                                    # the only draw is x_T
        return x_T.to(DEV).clone()

    ddpm.noise = noise
    res = ddpm.reverse_process(torch.zeros(shape, device=DEV), num_steps=S, clip_denoised=False)
    ab32 = _schedule()["alpha_bar_t"].float()
    taus = logsnr_timesteps(ab32, S)
    assert net.calls == taus[::-1]
    assert drawn == [shape] and res["buffer"] is None

    rows = dpmpp_2m_coefficients(ab32, taus, kind).double()
    x = x_T.double()
    hist = torch.zeros_like(x)
    Ex, Eh = torch.zeros_like(x), torch.zeros_like(x)
    for k in range(S - 1, -1, -1):
        ax, ap, cx, d0, d1 = (float(v) for v in rows[k][:5])
        g = net.gain(taus[k])
        p = g * x
        if kind == "sample":
            x0, E0, G = p, p.abs(), g
        else:
            m = ap * p
            x0 = ax * x - m
            E0 = ap * p.abs() + m.abs() + x0.abs()
            G = ax - ap * g
        Ex0 = abs(G) * Ex + 1.001 * U * E0
        if d1 != 0.0:
            assert 0 < k < S - 1
            w = d1 * hist
            t = d0 * x0 + w
            r = cx * x + t
            Ex = abs(cx) * Ex + abs(d0) * Ex0 + abs(d1) * Eh + 1.001 * U * (w.abs() + t.abs() + r.abs())
        elif cx != 0.0:
            u = d0 * x0
            r = cx * x + u
            Ex = abs(cx) * Ex + abs(d0) * Ex0 + 1.001 * U * (u.abs() + r.abs())
        else:
            assert k == 0
            r = d0 * x0
            Ex = abs(d0) * Ex0 + 1.001 * U * r.abs()
        Eh, hist, x = Ex0, x0, r
    got = res["denoised"].double().cpu()
    excess = (got - x).abs() - Ex
    print(f"analytic chain {kind} S={S}: max err {float((got - x).abs().max()):.3e}, max bound {float(Ex.max()):.3e}, "
          f"max |x| {float(x.abs().max()):.3e}")
    assert torch.isfinite(got).all() and float(excess.max()) <= 0.0, (S, kind, float(excess.max()))
    # The bound is not vacuous: it stays far below the scale of the sample the walk started from.  (Not of the result: at S <= 2 the
    # epsilon walk takes x0 = a_x x - a_p p at the noisiest timestep, where a_x and a_p are about 1 / sqrt(alpha_bar) = 200 and the
    # two terms cancel to a result of 1e-3; its rounding error, and so its bound, is 200 |x| U whatever the result's size.)
    assert float(Ex.max()) < 1e-3 * float(x_T.abs().max())
    if S >= 5:
        assert (rows[1:S - 1, 4] != 0).all()                            # the interior steps were second order


# ----------------------------------------------------------------------------- 2. accuracy on the device
@pytest.mark.parametrize("S", [10, 20])
def test_second_order_walk_is_at_least_four_times_as_accurate(S):
    """The analytic epsilon model of iid N(0, 0.25) data on LinearSchedule(1000): the probability-flow ODE has the closed form
    x_t = x_T sqrt(D_t / D_T).  x as the backbone receives it at its last call (t = taus[0]) against that form: the relative error of
    sampler="dpmpp_2m" is at most a quarter of that of sampler="ddim", eta=0 on the same log-SNR spaced timesteps - the condition of
    test_multistep_host.py, where float64 gives ratios of 6 and above; float32 rounding is about 1e-6 against errors of 1e-2."""
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    shape = (2, 1, 8, 8)
    sched = _schedule(1000, None)
    taus = logsnr_timesteps(sched["alpha_bar_t"].float(), S)
    errs = {}
    for sampler in ("dpmpp_2m", "ddim"):
        ddpm = DDPM(_Analytic, dict(s=0.5, kind="epsilon", steps=1000, betas=None), _schedule(1000, None), nn.MSELoss, timesteps=1000)
        res = ddpm.reverse_process_with(torch.zeros(shape, device=DEV), num_steps=S, eta=0.0, clip_denoised=False, sampler=sampler,
                                   spacing="logsnr")
        net = ddpm.backbone
        assert net.calls == taus[::-1] and ddpm._noise_offset == (res["denoised"].numel() + 3) // 4
        x_T, x_last = net.inputs[0].double().cpu(), net.inputs[-1].double().cpu()
        exact = x_T * math.sqrt(net.D(taus[0]) / net.D(taus[-1]))
        errs[sampler] = float((x_last - exact).norm() / exact.norm())
        errs[sampler + "_xT"] = x_T
    assert torch.equal(errs["dpmpp_2m_xT"], errs["ddim_xT"])           # the same draw of x_T
    print(f"S={S}: ddim {errs['ddim']:.3e}, dpmpp_2m {errs['dpmpp_2m']:.3e}, ratio {errs['ddim'] / errs['dpmpp_2m']:.2f}")
    assert errs["ddim"] > 1e-2 and errs["dpmpp_2m"] <= 0.25 * errs["ddim"], errs


# ----------------------------------------------------------------------------- 3. graph against eager
@pytest.mark.parametrize("env", ["0", "1"])
@pytest.mark.parametrize("kind,scale", [("epsilon", None), ("epsilon", 3.0), ("v", None), ("v", 3.0)])
def test_graph_replay_matches_eager_loop(monkeypatch, env, kind, scale):
    """The captured step (forward, rho_dpmpp_2m_step on x and the history, spaced advance; no Philox kernel) replayed S - 1 times is
    the eager loop bit for bit, checkpoints and RNG bookkeeping included - whatever RHO_HIP_GRAPH the pipelines were built under."""
    monkeypatch.setenv("RHO_HIP_GRAPH", env)
    B = UNET_CASES[CASE][1][0]
    y = R.discrete_parameter_rows(PARAM_SPACE, B).to(DEV)
    outs = {}
    for mode in (True, False):
        ddpm, xshape = _tiny_ddpm(CASE, prediction_type=kind, sampler="dpmpp_2m")
        assert ddpm.hip_graph_sampling == (env == "1")
        ddpm.hip_graph_sampling = mode
        res = ddpm.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=scale, num_steps=5)
        assert ddpm.hip_graph_sampling == mode             # the capture did not fall back
        if scale is not None:                              # both halves of the doubled batch stay equal
            x_all = res["denoised"]._base
            assert x_all is not None and x_all.shape[0] == 2 * B and torch.equal(x_all[:B], x_all[B:])
        outs[mode] = (res["denoised"].clone(), res["buffer"].clone(), ddpm._noise_offset)
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1], outs[False][1])
    assert outs[True][2] == outs[False][2] == (outs[True][0].numel() + 3) // 4      # the draw of x_T and nothing else
    assert torch.isfinite(outs[True][0]).all() and float(outs[True][0].abs().max()) <= 1.0
    assert float(outs[True][1].abs().sum()) > 0
    # the first-order walk on the same timesteps is another result: the sampler is not ignored
    other, xshape = _tiny_ddpm(CASE, prediction_type=kind)
    ro = other.reverse_process_with(torch.zeros(xshape, device=DEV), y, guidance_scale=scale, num_steps=5, spacing="logsnr")
    assert not torch.equal(ro["denoised"], outs[True][0])


# ----------------------------------------------------------------------------- 4. checkpoints
def test_checkpoints_follow_spaced_checkpoints():
    """t_checkpoints fills ``buffer`` as the DDIM walk does: slot i is x after the step of the i-th visited timestep (from the top)
    that spaced_checkpoints names - read back here as what the backbone received at its next call, or the result after step 0."""
    from rho_diffusion_amd.diffusion import DDPM
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    from rho_diffusion_amd.diffusion.spaced import spaced_checkpoints
    shape, S = (2, 1, 8, 8), 20
    ddpm = DDPM(_Analytic, dict(s=0.5, kind="v"), _schedule(), nn.MSELoss, timesteps=T, prediction_type="v", sampler="dpmpp_2m")
    res = ddpm.reverse_process(torch.zeros(shape, device=DEV), t_checkpoints=list(range(10)), num_steps=S)
    taus = logsnr_timesteps(_schedule()["alpha_bar_t"].float(), S)
    ckpt = spaced_checkpoints(T, taus)
    assert 0 < len(ckpt) <= 10 and len(ckpt) < S
    after = ddpm.backbone.inputs[1:] + [res["denoised"]]                # x after step k = S-1 .. 0
    want = [after[S - 1 - k] for k in range(S - 1, -1, -1) if taus[k] in ckpt]
    assert tuple(res["buffer"].shape) == (2, 10) + shape[1:]
    for i, w in enumerate(want):
        assert torch.equal(res["buffer"][:, i], w), i
    assert float(res["buffer"][:, len(want):].abs().sum()) == 0.0


# ----------------------------------------------------------------------------- 5. defaults unchanged
def test_defaults_issue_the_launches_of_before(ops, monkeypatch):
    """DDPM(...), DDPM(..., sampler="ddim", sampling_spacing=None) and spacing="uniform": a default reverse_process(num_steps=5) gives
    the bits of the launches the walk issued before the solver existed - written out here on the ops: Philox x_T, then per step the
    engine forward, rho_p_sample_step_spaced on the rows of spaced_timesteps, rho_spaced_advance - and never reaches the new wrapper."""
    from rho_diffusion_amd.diffusion.prediction import spaced_pred_coefficients
    from rho_diffusion_amd.diffusion.spaced import spaced_timesteps
    real = ops.dpmpp_2m_step

    def boom(*a, **k):
        raise AssertionError("the default path reached the multistep kernel")

    monkeypatch.setattr(ops, "dpmpp_2m_step", boom)
    outs = []
    for kw, call in ((dict(), dict()), (dict(sampler="ddim", sampling_spacing=None), dict()), (dict(), dict(sampler="ddim", spacing="uniform")),
                     (dict(sampling_spacing="uniform"), dict())):
        ddpm, xshape = _tiny_ddpm("tiny2d", **kw)
        res = ddpm.reverse_process_with(torch.zeros(xshape, device=DEV), num_steps=5, **call)
        outs.append((res["denoised"].clone(), ddpm._noise_offset))
        assert [k[3] for k in ddpm._spaced_cache] == ["ddim"]
    assert all(torch.equal(o[0], outs[0][0]) and o[1] == outs[0][1] for o in outs)
    # the walk of before, launch by launch
    ddpm, xshape = _tiny_ddpm("tiny2d")
    taus = spaced_timesteps(T, 5)
    rows = spaced_pred_coefficients(_schedule()["alpha_bar_t"].float(), taus, 0.0, "epsilon").to(DEV)
    taus_dev = torch.tensor(taus, dtype=torch.int32, device=DEV)
    x = torch.empty(xshape, dtype=torch.float32, device=DEV)
    ops.philox_normal(x, ddpm.noise_seed, 0)
    k_dev = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    t_dev = torch.full((1,), taus[-1], dtype=torch.int32, device=DEV)
    engine = ddpm.backbone.engine()
    with torch.no_grad():
        for _ in range(5):
            pred = engine.forward(x, None, None, t_scalar_dev=t_dev)
            ops.p_sample_step_spaced(x, pred.contiguous(), None, rows, k_dev, None, True)
            ops.spaced_advance(k_dev, t_dev, taus_dev, None, 0)
    assert torch.equal(x, outs[0][0]) and outs[0][1] == (x.numel() + 3) // 4
    # and with the trap lifted the solver gives another result
    monkeypatch.setattr(ops, "dpmpp_2m_step", real)
    other, _ = _tiny_ddpm("tiny2d", sampler="dpmpp_2m")
    assert not torch.equal(other.reverse_process(torch.zeros(xshape, device=DEV), num_steps=5)["denoised"], outs[0][0])


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_come_before_any_draw():
    ddpm, xshape = _tiny_ddpm("tiny2d")
    x = torch.zeros(xshape, device=DEV)
    with pytest.raises(ValueError, match="eta"):
        ddpm.reverse_process_with(x, num_steps=5, sampler="dpmpp_2m", eta=0.3)
    with pytest.raises(ValueError, match="num_steps"):
        ddpm.reverse_process_with(x, sampler="dpmpp_2m")                         # epsilon: the full loop is the reference's parity code
    with pytest.raises(ValueError, match="spacing"):
        ddpm.reverse_process_with(x, num_steps=[0, 10, 20, 49], sampler="dpmpp_2m", spacing="logsnr")
    with pytest.raises(ValueError, match="spacing"):
        ddpm.reverse_process_with(x, num_steps=[0, 10, 20, 49], spacing="uniform")
    with pytest.raises(ValueError, match="sampler"):
        ddpm.reverse_process_with(x, num_steps=5, sampler="unipc")
    assert ddpm._noise_offset == 0
    out = ddpm.reverse_process_with(x, num_steps=[0, 10, 20, 49], sampler="dpmpp_2m")["denoised"]     # an explicit sequence is legal
    assert torch.isfinite(out).all() and ddpm._noise_offset == (out.numel() + 3) // 4
    v, _ = _tiny_ddpm("tiny2d", prediction_type="v", sampler="dpmpp_2m")    # v: num_steps None still means range(T)
    out = v.reverse_process(x)["denoised"]
    assert torch.isfinite(out).all() and [k[0] for k in v._spaced_cache] == [tuple(range(T))]


# ----------------------------------------------------------------------------- 7. a schedule that ends without signal
def test_alpha_bar_zero_is_sampled_by_v_and_refused_by_epsilon():
    from rho_diffusion_amd.diffusion import LinearSchedule
    ab = LinearSchedule(20, 1e-3, 0.02)["alpha_bar_t"].float()
    assert float(ab[19]) == 0.0 and float(ab[18]) > 0.0                       # checked here on the CPU: exactly 0 at t = 19
    eps, xshape = _tiny_ddpm("tiny2d", schedule=LinearSchedule(20, 1e-3, 0.02), sampler="dpmpp_2m")
    x = torch.zeros(xshape, device=DEV)
    with pytest.raises(ValueError, match="timestep 19"):
        eps.reverse_process(x, num_steps=range(20))
    assert eps._noise_offset == 0
    for kind in ("v", "sample"):
        for kw in (dict(num_steps=range(20)), dict(num_steps=range(20), clip_denoised=False), dict()):
            ddpm, _ = _tiny_ddpm("tiny2d", schedule=LinearSchedule(20, 1e-3, 0.02), prediction_type=kind, sampler="dpmpp_2m")
            out = ddpm.reverse_process(x, **kw)["denoised"]
            assert torch.isfinite(out).all(), (kind, kw)
            if kw.get("clip_denoised", True):
                assert float(out.abs().max()) <= 1.0, (kind, kw)
