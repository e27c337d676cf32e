"""-m gpu: label dropout of classifier-free guidance training - the two kernels (rho_cond_keep_mask draws the mask, rho_cond_drop
applies it to what rho_multi_embed wrote), the engine's three condition paths and DDPM.training_step.

Network: case tiny2d_multi (batch 3, labels from PARAM_SPACE), fp32 engine, golden-template weights.  Oracle: R.unet_forward with the
pre-embedded condition y = multi_embeddings(labels) * keep[:, None] and stock autograd on the state dict.  Bars: the fp32 bars of the
repository's gradient tests (test_gpu_round2.py, test_gpu_training.py): forward rel-L2 1e-4, loss 2e-4 absolute, per-parameter
gradient norm within 2e-3 relative (+1e-6), leading values within 2e-3 of ten times the tensor's rms."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import philox_ref
from helpers import PARAM_SPACE, UNET_CASES, case_inputs, det_normal, det_state_dict, det_uniform, golden_template, grad_digest_of, load_golden, rel_l2
from gpu_util import DEV
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

CASE = "tiny2d_multi"
T = 50
KEEP = [1, 0, 1]
SENT = -776.0


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _tiny_ddpm(**kw):
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    g4 = load_golden("g4_unet.npz")
    cfg, xshape, _ = UNET_CASES[CASE]
    ddpm = DDPM(UNet, dict(cfg, compute_dtype="fp32"), LinearSchedule(T, 1e-3, 0.02), nn.MSELoss, timesteps=T, **kw)
    ddpm.backbone.cond_fn = MultiEmbeddings(parameter_space=PARAM_SPACE, embedding_dim=4 * cfg["model_channels"])
    ddpm.backbone.load_state_dict(det_state_dict(golden_template(g4, CASE), CASE))
    return ddpm.to(DEV).train(), xshape


def _injected(ddpm, xshape, keep=KEEP):
    """Inject t, the noise and the keep mask; returns (x0, eps, t) on the CPU."""
    eps, tq = det_normal(xshape, "cfg_eps"), torch.tensor([7, 23, 41])
    ddpm.noise = lambda data: eps.to(DEV)
    ddpm.random_timesteps = lambda bs: tq
    ddpm._draw_cond_keep = lambda bs, device: torch.tensor(keep, dtype=torch.uint8, device=device)
    return det_uniform(xshape, "cfg_x0", 0.0, 1.0), eps, tq


def _oracle(x0, eps, tq, y_emb_of):
    """Loss, prediction and state-dict gradients of the oracle; ``y_emb_of(sd)`` builds the [B, 4*mc] condition."""
    g4 = load_golden("g4_unet.npz")
    cfg = dict(UNET_CASES[CASE][0])
    sd = {k: v.clone().requires_grad_(True) for k, v in det_state_dict(golden_template(g4, CASE), CASE).items()}
    x_t = R.q_sample(x0, tq, eps, R.linear_schedule(T, 1e-3, 0.02)["alpha_bar_t"])
    pred = R.unet_forward(sd, cfg, x_t, tq, y_emb_of(sd))
    loss = torch.nn.functional.mse_loss(pred, eps)
    loss.backward()
    return loss.detach(), pred.detach(), sd


def _compare_grads(named_params, sd, skip=()):
    bad, n = [], 0
    for name, p in named_params:
        if name in skip:
            continue
        ref = sd[name].grad
        ref = torch.zeros_like(sd[name]) if ref is None else ref
        assert p.grad is not None, name
        d, r = grad_digest_of(p.grad), grad_digest_of(ref)
        n += 1
        rms = r[0] / np.sqrt(p.numel())
        if abs(d[0] - r[0]) > 2e-3 * r[0] + 1e-6:
            bad.append((name, "norm", d[0], r[0]))
        elif np.max(np.abs(d[2:] - r[2:])) > 2e-3 * max(rms, 1e-7) * 10 + 1e-6:
            bad.append((name, "head", d[2:4], r[2:4]))
    assert n > 20
    assert not bad, bad[:6]


# ----------------------------------------------------------------------------- rho_cond_drop alone
@pytest.mark.parametrize("dim", [64, 128])
@pytest.mark.parametrize("B", [1, 3, 64, 257])
def test_cond_drop_zeroes_dropped_rows_and_leaves_the_rest(ops, B, dim):
    nkeys = 2
    cond0 = det_normal((B, dim), f"drop_cond_{B}_{dim}")
    idx0 = (torch.arange(B * nkeys, dtype=torch.int32).view(B, nkeys) * 7) % 5
    keep = torch.tensor([(b * 5 + 1) % 3 != 0 for b in range(B)], dtype=torch.uint8)       # sample 1 is dropped, then every third
    if B == 1:
        keep[0] = 0
    pad = 64
    cbuf = torch.full((pad + B * dim + pad,), SENT, device=DEV)
    ibuf = torch.full((pad + B * nkeys + pad,), -77, dtype=torch.int32, device=DEV)
    cond, idx = cbuf[pad:pad + B * dim].view(B, dim), ibuf[pad:pad + B * nkeys].view(B, nkeys)
    cond.copy_(cond0)
    idx.copy_(idx0)
    out = ops.cond_drop(cond, idx, keep.to(DEV), nkeys)
    assert out is cond
    k = keep.bool()
    c, i = cond.cpu(), idx.cpu()
    assert (~k).any() and (c[~k] == 0).all() and (i[~k] == -1).all()
    assert torch.equal(c[k].view(torch.int32), cond0[k].view(torch.int32)) and torch.equal(i[k], idx0[k])       # bit for bit
    for buf, n, s in ((cbuf, B * dim, SENT), (ibuf, B * nkeys, -77)):
        assert bool((buf[:pad] == s).all()) and bool((buf[pad + n:] == s).all())
    # without category indices (pre-embedded conditions): the rows alone
    cond.copy_(cond0)
    ops.cond_drop(cond, None, keep.to(DEV))
    assert (cond.cpu()[~k] == 0).all() and torch.equal(cond.cpu()[k], cond0[k]) and torch.equal(idx.cpu(), i)


# ----------------------------------------------------------------------------- rho_cond_keep_mask
def test_keep_mask_is_the_philox_stream_and_reproducible(ops):
    """One word per sample in rho_randint's counter layout against the dropout threshold - tests/philox_ref.py restates both; the
    offset read from the device gives the same mask, another offset or seed another one."""
    seed, off, n, p = 0x1234_5678_9ABC_DEF0, 1_000_003, 257, 0.25
    a = ops.cond_keep_mask(n, p, seed, off, device=DEV).cpu()
    assert a.dtype == torch.uint8
    assert np.array_equal(a.numpy(), philox_ref.dropout_keep(seed, off, n, p))
    assert torch.equal(ops.cond_keep_mask(n, p, seed, off, device=DEV).cpu(), a)
    off_dev = torch.tensor([off], dtype=torch.int64, device=DEV)
    assert torch.equal(ops.cond_keep_mask(n, p, seed, 0, offset_dev=off_dev, device=DEV).cpu(), a)
    assert not torch.equal(ops.cond_keep_mask(n, p, seed, off + 1, device=DEV).cpu(), a)
    assert not torch.equal(ops.cond_keep_mask(n, p, seed ^ 1, off, device=DEV).cpu(), a)
    # launch geometry: a prefix of a longer draw is the shorter draw
    assert torch.equal(ops.cond_keep_mask(3, p, seed, off, device=DEV).cpu(), a[:3])


def test_keep_mask_statistics(ops):
    N, p = 65536, 0.25
    kept = float(ops.cond_keep_mask(N, p, 777, 12345, device=DEV).float().mean())
    sigma = math.sqrt(p * (1 - p) / N)
    print(f"kept fraction {kept:.5f}, expected {1 - p}, sigma {sigma:.5f}")
    assert abs(kept - (1 - p)) <= 5 * sigma
    assert bool(ops.cond_keep_mask(N, 0.0, 777, 12345, device=DEV).all())                 # p = 0 keeps all
    from rho_diffusion_amd import hip
    buf = torch.zeros(4, dtype=torch.uint8, device=DEV)
    for bad in (1.0, -0.25, float("nan")):
        assert hip.lib().rho_cond_keep_mask(buf.data_ptr(), 4, bad, 1, 0, None, hip.stream()) == -1           # RHO_E_ARG


def test_draw_cond_keep_uses_its_own_stream_and_advances_the_offset():
    ddpm, _ = _tiny_ddpm(cond_drop_prob=0.25)
    ddpm._noise_offset = 40
    a = ddpm._draw_cond_keep(257, DEV)
    assert ddpm._noise_offset == 40 + 65 and a.dtype == torch.uint8 and a.is_cuda
    seed = (ddpm.noise_seed ^ 0x2545F4914F6CDD1D) & philox_ref.U64
    assert np.array_equal(a.cpu().numpy(), philox_ref.dropout_keep(seed, 40, 257, 0.25))
    assert seed not in (ddpm.noise_seed, ddpm.noise_seed ^ 0x5DEECE66D)                    # the noise and the timestep streams


# ----------------------------------------------------------------------------- training step
@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
def test_training_step_with_dropped_labels_vs_oracle(ops, det):
    """keep = [1, 0, 1]: forward, loss and every parameter gradient against the oracle run on the masked embedding; the table rows
    that only the dropped sample looked up get exactly zero gradient."""
    _, _, _, y = case_inputs(CASE)
    old = ops.set_deterministic(det)
    try:
        ddpm, xshape = _tiny_ddpm(cond_drop_prob=0.5)
        x0, eps, tq = _injected(ddpm, xshape)
        off0 = ddpm._noise_offset
        loss = ddpm.training_step([x0.to(DEV), y.to(DEV)])
        assert ddpm._noise_offset == off0                                   # everything random was injected
        loss.backward()
        eng = ddpm.backbone.engine()
        pred = eng._last_train_plan.out.clone()
        assert eng._cond_keep is None                                       # consumed
    finally:
        ops.set_deterministic(old)
    keep = torch.tensor(KEEP, dtype=torch.float32)
    ref_loss, ref_pred, sd = _oracle(x0, eps, tq, lambda sd: R.multi_embeddings(y, PARAM_SPACE, sd) * keep[:, None])
    print(f"det={det}: forward rel_l2 {rel_l2(pred, ref_pred):.3e}, loss diff {abs(loss.item() - ref_loss.item()):.3e}")
    assert rel_l2(pred, ref_pred) < 1e-4
    assert abs(loss.item() - ref_loss.item()) < 2e-4
    _compare_grads(ddpm.backbone.named_parameters(), sd)
    # sample 1 has labels (l, m) = (-1.0, 2.5): rows 1 of "l" and 2 of "m", looked up by no other sample; row 3 of "l" by none
    y_l, y_m = [float(v) for v in y[:, 0]], [float(v) for v in y[:, 1]]
    assert (y_l[1], y_m[1]) == (PARAM_SPACE["l"][1], PARAM_SPACE["m"][2]) and y_l.count(y_l[1]) == 1 and y_m.count(y_m[1]) == 1
    gl = ddpm.backbone.cond_fn.embedding_layers["l"].weight.grad.cpu()
    gm = ddpm.backbone.cond_fn.embedding_layers["m"].weight.grad.cpu()
    assert (gl[1] == 0).all() and (gl[3] == 0).all() and (gm[2] == 0).all()
    assert (gl[0] != 0).any() and (gl[2] != 0).any() and (gm[1] != 0).any() and (gm[0] != 0).any()
    # and the mask mattered: the same step with every label kept predicts something else for sample 1 only
    ddpm2, _ = _tiny_ddpm(cond_drop_prob=0.5)
    _injected(ddpm2, xshape, keep=[1, 1, 1])
    ddpm2.training_step([x0.to(DEV), y.to(DEV)])
    full = ddpm2.backbone.engine()._last_train_plan.out
    assert rel_l2(pred[1], full[1]) > 1e-3 and rel_l2(pred[0], full[0]) < 1e-6 and rel_l2(pred[2], full[2]) < 1e-6


def test_training_step_without_dropout_draws_nothing_and_hands_no_mask():
    """cond_drop_prob = 0 (the default): _draw_cond_keep is never called, the engine sees no mask."""
    _, _, _, y = case_inputs(CASE)
    ddpm, xshape = _tiny_ddpm()
    x0, _, _ = _injected(ddpm, xshape)

    def boom(bs, device):
        raise AssertionError("drawn")

    ddpm._draw_cond_keep = boom
    ddpm.training_step([x0.to(DEV), y.to(DEV)])
    plan = ddpm.backbone.engine()._last_train_plan
    assert (plan.cond.abs().sum(1) > 0).all() and (plan.cond_idx.view(-1)[:2 * xshape[0]] >= 0).all()        # [B, nkeys] packed at the head of the buffer


def test_training_step_with_preembedded_conditions_zeroes_masked_rows():
    mc = UNET_CASES[CASE][0]["model_channels"]
    ddpm, xshape = _tiny_ddpm(cond_drop_prob=0.5)
    x0, eps, tq = _injected(ddpm, xshape)
    y_pre = det_normal((xshape[0], 4 * mc), "cfg_preemb")
    yd = y_pre.to(DEV)
    loss = ddpm.training_step([x0.to(DEV), yd])
    plan = ddpm.backbone.engine()._last_train_plan
    cond = plan.cond.cpu()
    assert (cond[1] == 0).all() and torch.equal(cond[0], y_pre[0]) and torch.equal(cond[2], y_pre[2])
    assert torch.equal(yd.cpu(), y_pre)                                     # the caller's tensor is not written
    keep = torch.tensor(KEEP, dtype=torch.float32)
    ref_loss, ref_pred, _ = _oracle(x0, eps, tq, lambda sd: y_pre * keep[:, None])
    assert rel_l2(plan.out, ref_pred) < 1e-4 and abs(loss.item() - ref_loss.item()) < 2e-4


class _TableCond(nn.Module):
    """A cond_fn that is not MultiEmbeddings: integer class -> one embedding row."""

    def __init__(self, n, dim):
        super().__init__()
        self.table = nn.Embedding(n, dim)

    def forward(self, y):
        return self.table(y.long())


def test_training_step_with_a_user_cond_fn_masks_under_autograd():
    mc = UNET_CASES[CASE][0]["model_channels"]
    ddpm, xshape = _tiny_ddpm(cond_drop_prob=0.5)
    fn = _TableCond(5, 4 * mc)
    with torch.no_grad():
        fn.table.weight.copy_(det_normal((5, 4 * mc), "cfg_table") * 0.1)
    ddpm.backbone.cond_fn = fn.to(DEV)
    x0, eps, tq = _injected(ddpm, xshape)
    labels = torch.tensor([0, 3, 0])                                        # row 3 is looked up by the dropped sample only
    loss = ddpm.training_step([x0.to(DEV), labels.to(DEV)])
    loss.backward()
    w = fn.table.weight.detach().cpu()
    keep = torch.tensor(KEEP, dtype=torch.float32)
    wr = w.clone().requires_grad_(True)
    ref_loss, ref_pred, sd = _oracle(x0, eps, tq, lambda sd: wr[labels] * keep[:, None])
    assert rel_l2(ddpm.backbone.engine()._last_train_plan.out, ref_pred) < 1e-4 and abs(loss.item() - ref_loss.item()) < 2e-4
    g = fn.table.weight.grad.cpu()
    assert (g[3] == 0).all() and (g[1] == 0).all() and (g[0] != 0).any()
    assert abs(float(g.double().norm()) - float(wr.grad.double().norm())) <= 2e-3 * float(wr.grad.double().norm()) + 1e-6
    _compare_grads(ddpm.backbone.named_parameters(), sd, skip=("cond_fn.table.weight",))


# ----------------------------------------------------------------------------- engine: who sees the mask
def test_mask_is_consumed_by_one_training_forward_and_never_by_inference():
    from rho_diffusion_amd.hip import RhoHipError
    cfg, x, t, y = case_inputs(CASE)
    ddpm, _ = _tiny_ddpm()
    model, eng = ddpm.backbone, ddpm.backbone.engine()
    xd, td, yd = x.to(DEV), t.to(DEV), y.to(DEV)
    eng.set_cond_keep(torch.tensor(KEEP, device=DEV))                       # any integer / bool mask is taken
    model.eval()
    with torch.no_grad():
        ref = model(xd, td, yd)                                             # inference plan: sees nothing, consumes nothing
    assert eng._cond_keep is not None
    n_inf = len(eng._plans)
    model.train()
    a = model(xd, td, yd).detach()
    assert eng._cond_keep is None and len(eng._plans) == n_inf + 1          # one training plan, keyed as ever
    b = model(xd, td, yd).detach()                                          # the next forward keeps every label
    assert len(eng._plans) == n_inf + 1
    assert rel_l2(b, ref) < 1e-5 and rel_l2(a[0], b[0]) < 1e-6 and rel_l2(a[2], b[2]) < 1e-6 and rel_l2(a[1], b[1]) > 1e-3
    eng.set_cond_keep(torch.ones(5, device=DEV))
    with pytest.raises(RhoHipError, match="keep mask"):
        model(xd, td, yd)
    assert eng._cond_keep is None
