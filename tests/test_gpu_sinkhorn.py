"""-m gpu: the Sinkhorn divergence behind WassersteinWrapper (metrics/geom.py:28-37) and PeakSignalNoiseRatio
(abstract_diffusion.py:79) on the device, against the float64 restatement of tests/sinkhorn_ref.py.  The float32 mode of that
restatement (costs summed left to right, loop in float32) only measures what float32 costs: its distance from float64 sizes the
bounds, it is never the code under test."""
import functools
import math

import numpy as np
import pytest
import torch
from torch import nn

import sinkhorn_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
CHUNK = 512                      # floats of D per partial (SK_CHUNK of csrc/sinkhorn.hip)
# D = 1000 keeps every row 16-byte aligned (the 16-byte loads); 3, 1, 5, 4099, 1025 and 33 do not (the scalar loads).  (5,7,1000),
# (8,8,4099) and (2,2,2*chunk+1) end in chunk tails; (128,128,33) is the size limit (several rounds of pair blocks); (32,32,4096)
# is the workload's batch with whole chunks, (64,64,257) three rounds of pair blocks and four lanes per softmin row.
SHAPES = [(4, 4, 3), (5, 7, 1000), (1, 1, 1), (3, 1, 5), (8, 8, 4099), (2, 2, 2 * CHUNK + 1), (128, 128, 33), (32, 32, 4096),
          (64, 64, 257)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def data(n, m, d):
    g = torch.Generator().manual_seed(1000 * n + 10 * m + d)
    return torch.randn(n, d, generator=g), torch.randn(m, d, generator=g) + 0.5


@functools.lru_cache(maxsize=None)
def d2_refs(n, m, d):
    """((d2 float64, |sequential float32 sum - float64|) for xy, xx, yy)."""
    x, y = data(n, m, d)
    out = []
    for u, v in ((x, y), (x, x), (y, y)):
        ref = SR.sq_dists(u, v)
        out.append((ref, (SR.sq_dists(u, v, fp32=True).double() - ref).abs()))
    return out


@functools.lru_cache(maxsize=None)
def ref(n, m, d, p, debias, fp32, grad=False):
    x, y = data(n, m, d)
    return SR.sinkhorn(x, y, p=p, debias=debias, fp32=fp32, want_grad=grad, upstream=2.5)


def dev(n, m, d):
    x, y = data(n, m, d)
    return x.to(DEV), y.to(DEV)


# ----------------------------------------------------------------------------- cost kernel
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pairwise_cost_against_float64(shape, p):
    """Per entry |d2 - d2_64| <= 2 e_seq + 4 * 2^-24 d2, e_seq the error of the left-to-right float32 sum of that entry.  p = 2
    returns d2 / 2 (an exact scaling); p = 1 returns sqrt(d2), whose error is that of d2 divided by 2 sqrt(d2) plus the square
    root's own rounding (at most one ulp <= 2^-23 C)."""
    from rho_diffusion_amd.engine import ops
    x, y = dev(*shape)
    got = ops.pairwise_cost(x, y, p)
    again = ops.pairwise_cost(x, y, p)
    for c, c2, (d2, e_seq) in zip(got, again, d2_refs(*shape)):
        assert torch.equal(c, c2)                                    # fixed summation order: the same bits
        c = c.double().cpu()
        bound = 2.0 * e_seq + 4.0 * U * d2
        if p == 2:
            err = (2.0 * c - d2).abs()
        else:
            clamped = d2 <= 1e-8
            cref = torch.sqrt(torch.clamp(d2, min=1e-8))
            err = torch.where(clamped, torch.zeros_like(c), (c - cref).abs())
            bound = bound / (2.0 * cref) + 2.0 * U * cref
            assert bool((c[clamped] == float(np.float32(1e-4))).all())
        worst = float((err / bound.clamp(min=1e-300)).max())
        print(f"{shape} p={p}: max err/bound {worst:.3f}, max err {float(err.max()):.3e}")
        assert bool((err <= bound).all())
    n, m, _ = shape
    diag = float(np.float32(1e-4)) if p == 1 else 0.0
    assert bool((got[1].diagonal() == diag).all()) and bool((got[2].diagonal() == diag).all())      # exactly
    assert torch.equal(got[1], got[1].T) and torch.equal(got[2], got[2].T)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_max_diameter(shape):
    from rho_diffusion_amd.engine import ops
    x, y = dev(*shape)
    want = SR.diameter_of(*data(*shape))
    got = float(ops.max_diameter(x, y).item())
    print(f"{shape}: diameter {got!r} vs {want!r}")
    assert abs(got - want) <= 4.0 * U * want
    assert torch.equal(ops.max_diameter(x, y), ops.max_diameter(x, y))


# ----------------------------------------------------------------------------- loss and potentials
@pytest.mark.parametrize("debias", [True, False], ids=["debias", "biased"])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_loss_and_potentials_against_float64(shape, p, debias):
    """|loss - loss_64| <= 4 |loss_32 - loss_64| + 16 * 2^-24 max C: the floor is a few float32 ulps at the size of the potentials.
    Every entry of the potentials keeps the same bound (with that entry's own float32 error)."""
    from rho_diffusion_amd.metrics import SinkhornDivergence
    x, y = dev(*shape)
    r64, r32 = ref(*shape, p, debias, False), ref(*shape, p, debias, True)
    metric = SinkhornDivergence(p=p, blur=0.01, debias=debias)
    loss = metric(x, y) if x.shape == y.shape else metric.samples_loss(x, y)      # forward asserts equal shapes, as the reference
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    floor = 16.0 * U * r64["c_max"]
    err, bound = abs(float(loss) - float(r64["loss"])), 4.0 * abs(float(r32["loss"]) - float(r64["loss"])) + floor
    print(f"{shape} p={p} debias={debias}: loss {float(loss)!r} ref {float(r64['loss'])!r} err {err:.3e} bound {bound:.3e} "
          f"(fp32 ref err {abs(float(r32['loss']) - float(r64['loss'])):.3e}, floor {floor:.3e})")
    assert err <= bound
    f, g = metric.potentials(x, y)
    for name, got, k in (("f", f, "f"), ("g", g, "g")):
        e = (got.double().cpu() - r64[k]).abs()
        b = 4.0 * (r32[k].double() - r64[k]).abs() + floor
        print(f"    {name}: max err/bound {float((e / b).max()):.3f}")
        assert bool((e <= b).all())


@pytest.mark.parametrize("p", [1, 2])
def test_loss_of_a_set_with_itself_is_zero(p):
    from rho_diffusion_amd.metrics import SinkhornDivergence
    x, _ = dev(8, 8, 4099)
    loss = float(SinkhornDivergence(p=p)(x, x.clone()))
    c_max = ref(8, 8, 4099, p, True, False)["c_max"]
    print(f"p={p}: loss(x, x) = {loss!r}, 8 * 2^-24 max C = {8.0 * U * c_max:.3e}")
    assert abs(loss) <= 8.0 * U * c_max


def test_all_rows_equal_gives_zero_loss_and_gradient():
    from rho_diffusion_amd.metrics import SinkhornDivergence
    x = torch.full((3, 2, 5), 0.25, device=DEV, requires_grad=True)
    loss = SinkhornDivergence()(x, x.detach().clone())
    loss.backward()
    assert float(loss) == 0.0 and x.grad.shape == x.shape and float(x.grad.abs().max()) == 0.0


# ----------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("shape,view", [((5, 7, 1000), (2, 500)), ((8, 8, 4099), (1, 4099))], ids=["5x7x1000", "8x8x4099"])
def test_gradient_against_autograd_of_the_restatement(shape, view, p):
    """(2.5 * loss).backward(): per element |g - g_64| <= 4 |g_32 - g_64| + 16 * 2^-24 max |g_64|.  (At blur 0.01 one ulp of a
    float32 cost moves a softmin exponent by 5e-4, so with float32 cost sums the plan of a row whose mass is split carries a
    relative noise of ~1e-4 and the p = 1 cases miss this bound; the kernels sum the costs and run the loop in float64.)"""
    from rho_diffusion_amd.metrics import SinkhornDivergence
    n, m, d = shape
    x, y = dev(*shape)
    pred = x.view(n, *view).clone().requires_grad_(True)
    metric = SinkhornDivergence(p=p, blur=0.01)
    loss = metric(pred, y.view(m, *view)) if n == m else metric.samples_loss(pred, y.view(m, *view))
    (2.5 * loss).backward()
    assert pred.grad.shape == pred.shape
    r64, r32 = ref(*shape, p, True, False, True), ref(*shape, p, True, True, True)
    g64 = r64["grad"]
    e = (pred.grad.double().cpu().view(n, d) - g64).abs()
    b = 4.0 * (r32["grad"].double() - g64).abs() + 16.0 * U * float(g64.abs().max())
    print(f"{shape} p={p}: max |grad| {float(g64.abs().max()):.3e}, max err {float(e.max()):.3e}, max err/bound {float((e / b).max()):.3f}, "
          f"max fp32-ref err {float((r32['grad'].double() - g64).abs().max()):.3e}, {int((e > b).sum())} of {e.numel()} elements over")
    assert bool((e <= b).all())


# ----------------------------------------------------------------------------- WassersteinWrapper
def test_wasserstein_wrapper_is_the_p1_blur001_divergence_of_the_flattened_pair():
    from rho_diffusion_amd.metrics import SinkhornDivergence, WassersteinWrapper
    from rho_diffusion_amd.registry import registry
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(4, 1, 8, 8, 8, generator=g).to(DEV), (torch.randn(4, 1, 8, 8, 8, generator=g) + 0.5).to(DEV)
    w = registry.get("layers", "WassersteinWrapper")()
    assert isinstance(w, WassersteinWrapper)
    got = w(a, b)
    assert torch.equal(got, SinkhornDivergence(p=1, blur=0.01)(a.flatten(1), b.flatten(1)))
    r = SR.sinkhorn(a.cpu(), b.cpu(), p=1)
    assert abs(float(got) - float(r["loss"])) <= 1e-5 * float(r["loss"])


def test_wasserstein_wrapper_with_a_given_diameter_neither_syncs_nor_breaks_a_graph_capture():
    from rho_diffusion_amd.metrics import WassersteinWrapper
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn(4, 1, 8, 8, 8, generator=g).to(DEV), (torch.randn(4, 1, 8, 8, 8, generator=g) + 0.5).to(DEV)
    dia = SR.diameter_of(a.flatten(1).cpu(), b.flatten(1).cpu())
    w = WassersteinWrapper(diameter=dia)
    eager = w(a, b).clone()                                # also uploads the schedule, once
    r = SR.sinkhorn(a.cpu(), b.cpu(), p=1)
    assert abs(float(eager) - float(r["loss"])) <= 1e-5 * float(r["loss"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = w(a, b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again, eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            out = w(a, b)
    except RuntimeError as exc:                            # not retried
        pytest.skip(f"graph capture refused: {exc}")
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ----------------------------------------------------------------------------- PSNR
@pytest.mark.parametrize("data_range", [None, 3.0], ids=["inferred", "given"])
@pytest.mark.parametrize("n", [1_000_003, 5])
def test_psnr_against_float64(n, data_range):
    from rho_diffusion_amd.metrics import PeakSignalNoiseRatio
    g = torch.Generator().manual_seed(n)
    target = torch.rand(n, generator=g) * 2.0 - 0.5
    pred = target + 0.1 * torch.randn(n, generator=g)
    got = PeakSignalNoiseRatio(data_range=data_range)(pred.to(DEV), target.to(DEV))
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    t64, p64 = target.double(), pred.double()
    rng = float(t64.max() - t64.min()) if data_range is None else data_range
    want = 10.0 * math.log10(rng ** 2 / float(((p64 - t64) ** 2).mean()))
    print(f"n={n} range={data_range}: {float(got)!r} vs {want!r}")
    assert abs(float(got) - want) <= 1e-5 * abs(want)


def test_training_step_logs_the_metrics_a_user_adds_and_leaves_the_loss_alone():
    from detdata import det_normal, det_state_dict, det_uniform
    from golden_cfg import UNET_CASES
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.metrics import PeakSignalNoiseRatio
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES["tiny2d"]
    x0 = det_uniform(xshape, "x0", 0.0, 1.0).to(DEV)
    eps = det_normal(xshape, "eps").to(DEV)
    tq = torch.tensor([3, 41])
    losses, logged = [], []
    for with_metric in (False, True):
        ddpm = DDPM(UNet, dict(kw, compute_dtype="fp32"), LinearSchedule(50, 1e-3, 0.02), nn.MSELoss, timesteps=50)
        ddpm.backbone.load_state_dict(det_state_dict(ddpm.backbone.state_dict(), "tiny2d"))
        ddpm = ddpm.to(DEV).train()
        assert len(ddpm.metrics) == 0
        if with_metric:
            ddpm.metrics["snr"] = PeakSignalNoiseRatio()
        ddpm.noise = lambda data: eps
        ddpm.random_timesteps = lambda bs: tq
        losses.append(ddpm.training_step(x0).detach().clone())
        logged.append(dict(ddpm._logged))
    assert torch.equal(losses[0], losses[1])
    assert "train_snr" not in logged[0] and torch.equal(logged[1]["train_loss"].detach(), losses[1])
    xt, _ = ddpm.forward_process(x0, tq)
    t64, p64 = x0.double().cpu(), xt.double().cpu()
    want = 10.0 * math.log10(float(t64.max() - t64.min()) ** 2 / float(((p64 - t64) ** 2).mean()))
    assert abs(float(logged[1]["train_snr"]) - want) <= 1e-5 * abs(want)
