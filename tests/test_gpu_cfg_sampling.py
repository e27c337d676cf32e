"""-m gpu: DDPM sampling with classifier-free guidance - the doubled batch, the null condition as the zero row and the fused
guided update, in the eager loop and in the captured HIP graph.

Network: case tiny2d_multi with its golden-template weights (fp32 engine), LinearSchedule(20), labels = the first rows of the
parameter-space product, the noise tape of test_generate_shapes_labels_and_values_vs_reference.  These weights separate the two
branches well: on the oracle rel_l2(e_c, e_u) at the first step is 0.28 (asserted below at > 1e-2), so a chain that ignored the
null branch could not pass."""
import pytest
import torch
from torch import nn

from helpers import PARAM_SPACE, UNET_CASES, det_normal, det_state_dict, golden_template, load_golden, rel_l2
from gpu_util import DEV
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

CASE = "tiny2d_multi"
T = 20
CHAIN_BAR = 2e-3                   # the unguided chain's bar (test_gpu_round2.py, same network, schedule and tape)


def _tiny_ddpm(case=CASE, **kw):
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    g4 = load_golden("g4_unet.npz")
    cfg, xshape, ykind = UNET_CASES[case]
    ddpm = DDPM(UNet, dict(cfg, compute_dtype="fp32"), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T, **kw)
    if ykind == "multi":
        ddpm.backbone.cond_fn = MultiEmbeddings(parameter_space=PARAM_SPACE, embedding_dim=4 * cfg["model_channels"])
    ddpm.backbone.load_state_dict(det_state_dict(golden_template(g4, case), case))
    return ddpm.to(DEV), xshape


def _labels(B):
    return R.discrete_parameter_rows(PARAM_SPACE, B)


def test_guided_chain_vs_oracle():
    """generate() with guidance_scale = 3 against R.reverse_process whose model evaluates R.unet_forward on the labels and on the
    zero condition and combines the two in float32.  Bar: the unguided chain's 2e-3 times |s| + |1 - s| = 5, because
    g = s * e_c + (1 - s) * e_u adds the two predictions' errors with those weights."""
    s = 3.0
    g4 = load_golden("g4_unet.npz")
    cfg = dict(UNET_CASES[CASE][0])
    sd = det_state_dict(golden_template(g4, CASE), CASE)
    gshape = UNET_CASES[CASE][1]
    B = gshape[0]
    tape = [det_normal(gshape, f"gentape_{i}") for i in range(T)]
    labels = _labels(B)
    null = torch.zeros(B, 4 * cfg["model_channels"])
    first = {}

    def model(x, t, c):
        e_c = R.unet_forward(sd, cfg, x, t, c, PARAM_SPACE)
        e_u = R.unet_forward(sd, cfg, x, t, null)
        first.setdefault("sep", rel_l2(e_c, e_u))
        return e_u + torch.tensor(s) * (e_c - e_u)

    with torch.no_grad():
        ref, ref_buf = R.reverse_process(model, tape[0], R.linear_schedule(T, 1e-3, 0.02), tape[1:], labels, num_checkpoints=3)
        plain, _ = R.reverse_process(lambda x, t, c: R.unet_forward(sd, cfg, x, t, c, PARAM_SPACE), tape[0],
                                     R.linear_schedule(T, 1e-3, 0.02), tape[1:], labels)
    assert first["sep"] > 1e-2, first                     # the fixture weights tell the two branches apart
    assert rel_l2(ref, plain) > 10 * CHAIN_BAR * 5         # and the guided chain ends somewhere else than the conditional one

    ddpm, _ = _tiny_ddpm(sampling_batch_size=B, sample_parameter_space=PARAM_SPACE, guidance_scale=s, t_checkpoints=[0, 1, 2])
    it = iter([t.to(DEV) for t in tape])
    drawn = []

    def noise(data):
        drawn.append(tuple(data.shape))
        return next(it).clone()

    ddpm.noise = noise
    out = ddpm.generate()
    den, buf = ddpm.last_samples["denoised"], ddpm.last_samples["buffer"]
    assert out is den and tuple(den.shape) == gshape
    bar = CHAIN_BAR * (abs(s) + abs(1 - s))
    print(f"guided chain rel_l2 {rel_l2(den, ref):.3e} (bar {bar:.1e}), buffer {rel_l2(buf, ref_buf):.3e}")
    assert rel_l2(den, ref) < bar
    assert rel_l2(buf, ref_buf) < bar
    assert drawn == [gshape] * (T - 1)                      # x_T and one z per t > 1, each for B samples: as unguided


@pytest.mark.parametrize("env", ["0", "1"])
def test_guided_graph_replay_matches_eager_loop(monkeypatch, env):
    """The captured step (Philox draw, 2B forward, guided update, step advance) replayed is the eager loop bit for bit, checkpoints
    and RNG bookkeeping included - whatever RHO_HIP_GRAPH the pipelines were built under."""
    monkeypatch.setenv("RHO_HIP_GRAPH", env)
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    outs = {}
    for mode in (True, False):
        ddpm, xshape = _tiny_ddpm()
        assert ddpm.hip_graph_sampling == (env == "1")
        ddpm.hip_graph_sampling = mode
        res = ddpm.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=3.0)
        assert ddpm.hip_graph_sampling == mode             # the capture did not fall back
        outs[mode] = (res["denoised"].clone(), res["buffer"].clone(), ddpm._noise_offset)
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1], outs[False][1])
    assert outs[True][2] == outs[False][2]
    assert torch.isfinite(outs[True][0]).all() and float(outs[True][0].abs().max()) <= 1.0
    assert float(outs[True][1].abs().sum()) > 0


def test_no_scale_is_the_unguided_path_and_shapes_agree():
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    a, xshape = _tiny_ddpm()
    ra = a.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2])
    b, _ = _tiny_ddpm()
    rb = b.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=None)
    assert torch.equal(ra["denoised"], rb["denoised"]) and torch.equal(ra["buffer"], rb["buffer"])
    assert a._noise_offset == b._noise_offset
    eng = b.backbone.engine()
    assert eng._plans and all(k[0][0] == B for k in eng._plans)             # no plan of the doubled batch
    # the per-call value overrides the attribute; the guided call returns what the unguided one does, shape and device
    rg = b.reverse_process(torch.zeros(xshape, device=DEV), y, t_checkpoints=[0, 1, 2], guidance_scale=3.0)
    assert any(k[0][0] == 2 * B for k in eng._plans)
    for key in ("denoised", "buffer"):
        assert rg[key].shape == ra[key].shape and rg[key].device == ra[key].device and rg[key].dtype == ra[key].dtype
    assert b._noise_offset == 2 * a._noise_offset                            # the same draws again: z for B samples, not 2B
    assert rel_l2(rg["denoised"], ra["denoised"]) > 1e-2
    # scale 1 (and 0) are ordinary scales: they take the guided path
    r1 = b.reverse_process(torch.zeros(xshape, device=DEV), y, guidance_scale=1.0)
    assert torch.isfinite(r1["denoised"]).all() and r1["buffer"] is None and b._noise_offset == 3 * a._noise_offset


class _NarrowCond(nn.Module):
    """A cond_fn whose output is not the [B, 4 * mc] form."""

    def forward(self, y):
        return torch.zeros(y.shape[0], 7, device=y.device)


def test_refusals():
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models.vit import VisionTransformer
    B = UNET_CASES[CASE][1][0]
    y = _labels(B).to(DEV)
    ddpm, xshape = _tiny_ddpm(guidance_scale=2.0)
    x = torch.zeros(xshape, device=DEV)
    off = ddpm._noise_offset
    with pytest.raises(ValueError, match="conditions"):
        ddpm.reverse_process(x)
    assert ddpm._noise_offset == off                                         # refused before anything was drawn
    ddpm.backbone.cond_fn = _NarrowCond()
    with pytest.raises(ValueError, match="model_channels"):
        ddpm.reverse_process(x, y)
    plain, pshape = _tiny_ddpm("tiny2d")
    with pytest.raises(ValueError, match="num_classes"):
        plain.reverse_process(torch.zeros(pshape, device=DEV), y[:pshape[0]], guidance_scale=2.0)
    kw = dict(patch_size=4, input_shapes=[16, 16], num_channels=1, embedding_dim=64, hidden_dim=64, activation="GELU",
              transformer_depth=1, num_heads=2)
    vit = DDPM(VisionTransformer, kw, LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T).to(DEV)
    with pytest.raises(ValueError, match="unconditional"):
        vit.reverse_process(torch.zeros(2, 1, 16, 16, device=DEV), y[:2], guidance_scale=2.0)


def test_generate_with_guidance_is_reproducible_from_the_philox_seed():
    outs = []
    for scale in (2.0, 2.0, None):
        ddpm, xshape = _tiny_ddpm(sampling_batch_size=3, sample_parameter_space=PARAM_SPACE, guidance_scale=scale)
        out = ddpm.generate()
        assert tuple(out.shape) == tuple(xshape) and out.device.type == "cuda"
        assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
        assert ddpm.hip_graph_sampling                                       # the captured graph served the guided chain
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    assert rel_l2(outs[0], outs[2]) > 1e-2                                   # and guidance changed the samples
