"""-m gpu: the VisionTransformer kernels of csrc/vit.hip against float64 torch on the same (rounded) inputs.

Bounds: float32 rel_l2 < 1e-5, bf16 < 1e-2 against the reference evaluated on the bf16-rounded inputs (the project's kernel-level
bounds, as in test_gpu_kernels.py's attention tests); LayerNorm of rows offset by +100 in float32 < 3e-5 (a stable float32 evaluation
sits at 3e-6, the E[x^2] - E[x]^2 form at 4e-4); the patch gather / scatter are bit-exact."""
import pytest
import torch
import torch.nn.functional as F

from helpers import det_normal, det_uniform, rel_l2
from gpu_util import DEV, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
ROWS = {1: 1, 7: 7, 64: 4, 333: 3}          # R -> the B of the `add` cases (B divides R)
WIDTHS = [32, 96, 256, 1024]


def tolk(dtype):
    return 1e-2 if dtype == torch.bfloat16 else 1e-5


def _ln_inputs(R, E, add, dtype, offset=0.0):
    x = rnd(det_normal((R, E), f"lnx{R}_{E}") + offset, dtype)
    a = 0.5 * det_normal((ROWS[R], E), f"lna{R}_{E}") if add else None
    gamma = 1.0 + 0.2 * det_uniform((E,), f"lng{E}")
    beta = 0.1 * det_uniform((E,), f"lnb{E}")
    return x, a, gamma, beta


def _ln_ref(x, a, gamma, beta):
    xx = x.double()
    if a is not None:
        xx = xx + a.double().repeat_interleave(x.shape[0] // a.shape[0], 0)
    y = F.layer_norm(xx, (x.shape[1],), gamma.double(), beta.double(), 1e-5)
    mean = xx.mean(1)
    rstd = 1.0 / torch.sqrt(xx.var(1, unbiased=False) + 1e-5)
    return y, torch.stack([mean, rstd], 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
def test_layernorm_forward(dtype, add):
    from rho_diffusion_amd.engine import ops
    for R in ROWS:
        for E in WIDTHS:
            x, a, gamma, beta = _ln_inputs(R, E, add, dtype)
            y, stats = ops.layernorm(x.to(DEV).to(dtype), gamma.to(DEV), beta.to(DEV), add=a.to(DEV) if add else None)
            yr, sr = _ln_ref(x, a, gamma, beta)
            e, es = rel_l2(y, yr), rel_l2(stats, sr)
            print(f"layernorm fwd R={R} E={E} add={add} {dtype}: y {e:.2e} stats {es:.2e}")
            assert y.dtype == dtype and tuple(y.shape) == (R, E)
            assert e < tolk(dtype), (R, E, e)
            assert es < 1e-5, (R, E, es)


def test_layernorm_forward_offset_rows():
    from rho_diffusion_amd.engine import ops
    for R in ROWS:
        for E in WIDTHS:
            x, a, gamma, beta = _ln_inputs(R, E, False, torch.float32, offset=100.0)
            y, _ = ops.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV))
            e = rel_l2(y, _ln_ref(x, None, gamma, beta)[0])
            print(f"layernorm offset rows R={R} E={E}: {e:.2e}")
            assert e < 3e-5, (R, E, e)


def test_layernorm_refuses_unsupported_widths():
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    for E in (16, 40, 4096):
        with pytest.raises(RhoHipError):
            ops.layernorm(torch.zeros(4, E, device=DEV), torch.ones(E, device=DEV), torch.zeros(E, device=DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
def test_layernorm_backward(dtype, add):
    from rho_diffusion_amd.engine import ops
    t = tolk(dtype)
    for R in ROWS:
        for E in WIDTHS:
            x, a, gamma, beta = _ln_inputs(R, E, add, dtype)
            dy = rnd(det_normal((R, E), f"lndy{R}_{E}"), dtype)
            xr = x.double().requires_grad_(True)
            ar = a.double().requires_grad_(True) if add else None
            gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
            xx = xr + ar.repeat_interleave(R // ar.shape[0], 0) if add else xr
            F.layer_norm(xx, (E,), gr, br, 1e-5).backward(dy.double())

            xd, dyd, gd = x.to(DEV).to(dtype), dy.to(DEV).to(dtype), gamma.to(DEV)
            ad = a.to(DEV) if add else None
            _, stats = ops.layernorm(xd, gd, beta.to(DEV), add=ad)
            dg, db = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
            dx, dadd = ops.layernorm_bwd(dyd, xd, stats, gd, dg, db, add=ad)
            errs = dict(dx=rel_l2(dx, xr.grad), dgamma=rel_l2(dg, gr.grad), dbeta=rel_l2(db, br.grad))
            if add:
                errs["dadd"] = rel_l2(dadd, ar.grad)
            print(f"layernorm bwd R={R} E={E} add={add} {dtype}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            for k, v in errs.items():
                assert v < t, (R, E, k, v)
            # two runs give the same bits
            dg2, db2 = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
            dx2, dadd2 = ops.layernorm_bwd(dyd, xd, stats, gd, dg2, db2, add=ad)
            assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
            if add:
                assert torch.equal(dadd, dadd2)
            # accumulate mode: on top of its own result it doubles it (float32 buffers: exactly)
            dxa, dga, dba = dx.clone(), dg.clone(), db.clone()
            _, dadd3 = ops.layernorm_bwd(dyd, xd, stats, gd, dga, dba, add=ad, dx=dxa, acc_dx=True, acc_params=True)
            assert torch.equal(dga, 2 * dg) and torch.equal(dba, 2 * db)
            if dtype == torch.float32:
                assert torch.equal(dxa, 2 * dx)
            else:                       # the sum is rounded to bf16 once more
                assert rel_l2(dxa, 2 * dx.float()) < t
            if add:
                assert torch.equal(dadd3, dadd)            # the sample sums are of the gradient computed here, not of the buffer


def _ref_patchify(x, p):
    """[B, C, *S] -> [B, N, K] by reshape / permute: tokens in row-major patch order, k = (c, offsets in memory order)."""
    B, C = x.shape[:2]
    d = x.dim() - 2
    grid = [s // p for s in x.shape[2:]]
    v = x.reshape(B, C, *[q for g in grid for q in (g, p)])
    perm = [0] + [2 + 2 * i for i in range(d)] + [1] + [3 + 2 * i for i in range(d)]
    N = 1
    for g in grid:
        N *= g
    return v.permute(perm).reshape(B, N, C * p ** d)


def _ref_unpatchify(tok, shape, p):
    B, C = shape[:2]
    d = len(shape) - 2
    grid = [s // p for s in shape[2:]]
    v = tok.reshape(B, *grid, C, *([p] * d))
    perm = [0, 1 + d] + [q for i in range(d) for q in (1 + i, 2 + d + i)]
    return v.permute(perm).reshape(shape)


PATCH_SHAPES = [(2, 1, 24), (3, 2, 8, 12), (2, 3, 8, 4, 12), (1, 3, 4, 4), (2, 2, 4, 8, 4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_patchify_unpatchify_bit_exact(dtype):
    from rho_diffusion_amd.engine import ops
    for shape in PATCH_SHAPES:
        for p in (1, 2, 4):
            x = det_normal(shape, f"px{shape}")
            B, C = shape[:2]
            d = len(shape) - 2
            K = C * p ** d
            kp = ops.vit_kpad(K)
            tok = ops.patchify(x.to(DEV), p, dtype)
            ref = _ref_patchify(x, p).to(dtype)
            assert tuple(tok.shape) == (B, ref.shape[1], kp) and tok.dtype == dtype
            assert torch.equal(tok[..., :K].cpu(), ref), (shape, p)
            assert kp == K or float(tok[..., K:].float().abs().max()) == 0.0            # pad lanes exactly zero
            # the conv_shaper GEMM operand: unfold gives the same columns
            if d == 2:
                uf = F.unfold(x, kernel_size=p, stride=p).transpose(1, 2).to(dtype)
                assert torch.equal(tok[..., :K].cpu(), uf)
            back = ops.unpatchify(tok, shape, p)
            assert torch.equal(back.cpu(), x.to(dtype).float()), (shape, p)
            # scatter of arbitrary tokens (pad lanes are ignored) + bias, and the bias gradient
            tk = rnd(det_normal((B, ref.shape[1], kp), f"pt{shape}{p}"), dtype)
            bias = 0.3 * det_uniform((C,), f"pb{C}")
            out = ops.unpatchify(tk.to(DEV).to(dtype), shape, p, bias=bias.to(DEV))
            want = _ref_unpatchify(tk[..., :K], shape, p) + bias.view(1, C, *([1] * d))
            assert torch.equal(out.cpu(), want), (shape, p)
            dbias = torch.ones(C, device=DEV)
            ops.patchify(x.to(DEV), p, dtype, dbias=dbias)
            s = x.double().sum(dim=[0] + list(range(2, x.dim())))
            assert float((dbias.double().cpu() - s).abs().max()) < 1e-5 * float(x.double().abs().sum(dim=[0] + list(range(2, x.dim()))).max())
            ops.patchify(x.to(DEV), p, dtype, dbias=dbias, acc_dbias=True)
            assert float((dbias.double().cpu() - 2 * s).abs().max()) < 2e-5 * float(x.double().abs().sum(dim=[0] + list(range(2, x.dim()))).max())


def test_patch_kernels_refuse_bad_geometry():
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    with pytest.raises(RhoHipError):
        ops.patchify(torch.zeros(1, 1, 10, device=DEV), 4, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_bias_act_and_pos_add(dtype):
    from rho_diffusion_amd.engine import ops
    t = tolk(dtype)
    acts = {"SiLU": F.silu, "ReLU": F.relu, "GELU": F.gelu, "Tanh": torch.tanh, "Sigmoid": torch.sigmoid, "ELU": F.elu}
    R, C = 37, 96
    x = rnd(det_normal((R, C), "bax"), dtype)
    dy = rnd(det_normal((R, C), "bady"), dtype)
    bias = 0.5 * det_uniform((C,), "bab")
    for name, fn in acts.items():
        for b in (None, bias):
            xr = x.double().requires_grad_(True)
            yr = fn(xr + b.double() if b is not None else xr)
            yr.backward(dy.double())
            xd = x.to(DEV).to(dtype)
            y = ops.bias_act(xd, ops.ACT_CODES[name], bias=b.to(DEV) if b is not None else None)
            dx = ops.bias_act_bwd(xd, dy.to(DEV).to(dtype), ops.ACT_CODES[name], bias=b.to(DEV) if b is not None else None)
            assert rel_l2(y, yr) < t, name
            assert rel_l2(dx, xr.grad) < t, name
    B, N, E = 3, 7, 32
    h = rnd(det_normal((B, N, E), "pah"), dtype)
    pos = det_normal((N, E), "pap")
    got = ops.pos_add(h.to(DEV).to(dtype).clone(), pos.to(DEV))
    assert rel_l2(got, h.double() + pos.double()) < t
    dpos = ops.pos_add_bwd(h.to(DEV).to(dtype))
    assert rel_l2(dpos, h.double().sum(0)) < 1e-5


def test_layernorm_backward_one_row_per_sample_at_the_grid_limit():
    """rows_per_sample = 1 with 65535 samples fills gridDim.y of the row pass and of the dadd finalize; one sample more is refused
    before anything is launched."""
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    B, E = 65535, 32
    x, dy = det_normal((B, E), "lnlim_x").to(DEV), det_normal((B, E), "lnlim_dy").to(DEV)
    a = 0.5 * det_normal((B, E), "lnlim_a").to(DEV)
    gamma, beta = (1.0 + 0.2 * det_uniform((E,), "lnlim_g")).to(DEV), torch.zeros(E, device=DEV)
    _, stats = ops.layernorm(x, gamma, beta, add=a)
    dg, db = torch.empty(E, device=DEV), torch.empty(E, device=DEV)
    dx, dadd = ops.layernorm_bwd(dy, x, stats, gamma, dg, db, add=a)
    xr = x.double().cpu().requires_grad_(True)
    gr = gamma.double().cpu().requires_grad_(True)
    F.layer_norm(xr + a.double().cpu(), (E,), gr, beta.double().cpu(), 1e-5).backward(dy.double().cpu())
    assert rel_l2(dx, xr.grad) < 1e-5 and rel_l2(dg, gr.grad) < 1e-5
    assert torch.equal(dadd, dx)                               # one row per sample: its sum is the row
    x1 = torch.zeros(B + 1, E, device=DEV)
    with pytest.raises(RhoHipError):
        ops.layernorm_bwd(x1, x1, torch.ones(B + 1, 2, device=DEV), gamma, dg, db, add=x1.clone())


def test_patchify_bias_gradient_two_level_sum():
    """More 256-element tiles than partial blocks (3 * ceil(60000 / 256) = 705 > 256) and a ragged last tile per row."""
    from rho_diffusion_amd.engine import ops
    shape = (3, 2, 200, 300)
    x = det_normal(shape, "pbias_big")
    want = x.double().sum(dim=(0, 2, 3))
    scale = float(x.double().abs().sum(dim=(0, 2, 3)).max())
    d1, d2 = torch.full((2,), 7.0, device=DEV), torch.full((2,), 7.0, device=DEV)
    ops.patchify(x.to(DEV), 4, torch.bfloat16, dbias=d1)
    ops.patchify(x.to(DEV), 4, torch.bfloat16, dbias=d2)
    assert float((d1.double().cpu() - want).abs().max()) < 1e-5 * scale
    assert torch.equal(d1, d2)                                  # fixed order: the same bits
    ops.patchify(x.to(DEV), 4, torch.bfloat16, dbias=d2, acc_dbias=True)
    assert torch.equal(d2, 2 * d1)
