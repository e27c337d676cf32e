"""-m gpu: the 1-channel ends of the 3-D UNet as single launches (csrc/ends.hip: rho_stem_conv3d, rho_head_conv3d) against the CPU
oracle (oracle/ref_torch.py conv_nd on bf16-rounded operands; tolerance of the bf16 kernels: rel-L2 <= 6e-3) and against the GEMM-form
launches they replace in inference plans (rho_im2col_taps + 1x1x1 conv; 1x1x1 conv + rho_tap_gather_sum); below those, the exact
forms: integer operands bit for bit against fp64 (every template instance, per-tile statistics, the stem kernel as the head's data
gradient, an affine prologue without SiLU, no bias, no statistics) and a per-element bound behind SiLU."""
import math

import pytest
import torch
import torch.nn.functional as F

import weight_table_cases as X
from exact_util import assert_bit_equal, assert_within_abs, guarded, guards_intact
from helpers import det_normal, rel_l2
from gpu_util import DEV, bf16_round, from_cl, to_cl
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("shape", [(2, 8, 16, 16), (1, 5, 9, 11), (1, 64, 64, 64)], ids=["even", "ragged", "c3_64cube"])
def test_stem_conv3d_vs_oracle_and_statistics(ops, cout, shape):
    N, D, H, W = shape
    x = det_normal((N, 1, D, H, W), f"stem_x{D}")
    w = det_normal((cout, 1, 3, 3, 3), f"stem_w{cout}") / math.sqrt(27.0)
    b = det_normal((cout,), "stem_b") * 0.1
    ref = R.conv_nd(3, bf16_round(x), bf16_round(w), b, stride=1, padding=1)                  # [N, cout, D, H, W]
    wp = ops.prep_conv_weight(w.reshape(cout, 27, 1, 1, 1).to(DEV), BF16)                       # [1, coutp, 32]: the im2col form
    assert tuple(wp.shape) == (1, cout, 32), tuple(wp.shape)
    y = torch.full((N, D, H, W, cout), float("nan"), dtype=BF16, device=DEV)
    tiles = ops.stem_conv3d_tiles(D, H, W)
    assert tiles == -(-D // 4) * -(-H // 8) * -(-W // 8)
    st = torch.full((N, tiles, 2, cout), float("nan"), device=DEV)
    xd, bd = x.to(DEV), b.to(DEV)
    ops.stem_conv3d(xd, wp, bd, y, st)
    torch.cuda.synchronize()
    got = from_cl(y, 3)
    assert torch.isfinite(got).all()
    assert rel_l2(got, ref) < 6e-3, rel_l2(got, ref)
    yy = y.float().reshape(N, -1, cout)
    assert rel_l2(st[:, :, 0].sum(1), yy.sum(1)) < 1e-3 and rel_l2(st[:, :, 1].sum(1), (yy * yy).sum(1)) < 1e-3
    # the two launches it replaces (im2col to [pos][32], then the 1x1x1 GEMM): same operands, same rounding points
    from rho_diffusion_amd import hip
    xc = torch.empty(N, D, H, W, 32, dtype=BF16, device=DEV)
    hip.check(hip.lib().rho_im2col_taps(xd.data_ptr(), xc.data_ptr(), 1, N, 1, D, H, W, 3, 3, 3, 32, hip.stream()), "rho_im2col_taps")
    y2, _ = ops.conv(xc, None, wp, bd, kernel=(1, 1, 1), cout=cout)
    assert rel_l2(got, from_cl(y2, 3)) < 3e-3


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("shape", [(2, 8, 16, 16), (1, 5, 9, 11)], ids=["even", "ragged"])
@pytest.mark.parametrize("prologue", [True, False], ids=["gn_silu", "raw"])
def test_head_conv3d_vs_oracle(ops, C, shape, prologue):
    N, D, H, W = shape
    x = bf16_round(det_normal((N, C, D, H, W), f"head_x{C}"))
    w = bf16_round(det_normal((1, C, 3, 3, 3), f"head_w{C}") / math.sqrt(27.0 * C))
    b = det_normal((1,), "head_b") * 0.1
    pre = (1 + 0.3 * det_normal((N, C), "head_a"), 0.2 * det_normal((N, C), "head_pb")) if prologue else None
    xa = x
    if pre is not None:
        xa = bf16_round(F.silu(pre[0].reshape(N, C, 1, 1, 1) * x + pre[1].reshape(N, C, 1, 1, 1)))
    ref = R.conv_nd(3, xa, w, b, stride=1, padding=1)                                          # [N, 1, D, H, W]
    # taps as rows: W[tap][c], prepared like a 1x1x1 conv with 32 output channels (the _HeadAsGemm form)
    wt = torch.zeros(32, C, 1, 1, 1)
    wt[:27, :, 0, 0, 0] = w[0].reshape(C, 27).t()
    wp = ops.prep_conv_weight(wt.to(DEV), BF16)
    assert tuple(wp.shape) == (1, 32, C)
    out = torch.full((N, 1, D, H, W), float("nan"), device=DEV)
    pa, pb = (pre[0].to(DEV), pre[1].to(DEV)) if pre else (None, None)
    ops.head_conv3d(to_cl(x, BF16), pa, pb, True, wp, b.to(DEV), out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isfinite(got).all()
    # (the 27 partial sums are rounded to bf16 before they are added: the round-2 launches' rounding point)
    assert rel_l2(got, ref) < 6e-3, rel_l2(got, ref)


def test_head_conv3d_at_bench_size_matches_the_gemm_form(ops):
    """c3's head (64 channels at 64^3, one sample): against the two launches of the GEMM form on the same operands."""
    from rho_diffusion_amd import hip
    N, C, D, H, W = 1, 64, 64, 64, 64
    x = to_cl(bf16_round(det_normal((N, C, D, H, W), "headb_x")), BF16)
    w = bf16_round(det_normal((1, C, 3, 3, 3), "headb_w") / math.sqrt(27.0 * C))
    wt = torch.zeros(32, C, 1, 1, 1)
    wt[:27, :, 0, 0, 0] = w[0].reshape(C, 27).t()
    wp = ops.prep_conv_weight(wt.to(DEV), BF16)
    pa = (1 + 0.3 * det_normal((N, C), "headb_a")).to(DEV)
    pb = (0.2 * det_normal((N, C), "headb_pb")).to(DEV)
    bias = torch.full((1,), 0.25, device=DEV)
    out = torch.empty(N, 1, D, H, W, device=DEV)
    ops.head_conv3d(x, pa, pb, True, wp, bias, out)
    tt, _ = ops.conv(x, None, wp, torch.zeros(32, device=DEV), kernel=(1, 1, 1), cout=32, pre_a=pa, pre_b=pb, pre_silu=True)
    ref = torch.empty(N, 1, D * H * W, device=DEV)
    hip.check(hip.lib().rho_tap_gather_sum(tt.data_ptr(), 1, N, D, H, W, 3, 3, 3, 32, bias.data_ptr(), ref.data_ptr(), hip.stream()),
              "rho_tap_gather_sum")
    torch.cuda.synchronize()
    assert rel_l2(out.reshape(-1).cpu(), ref.reshape(-1).cpu()) < 2e-3


def test_ends_refuse_what_they_do_not_cover(ops):
    from rho_diffusion_amd.hip import RhoHipError
    x = torch.zeros(1, 1, 8, 8, 8, device=DEV)
    w = torch.zeros(1, 96, 32, dtype=BF16, device=DEV)
    with pytest.raises(RhoHipError):
        ops.stem_conv3d(x, w, torch.zeros(96, device=DEV), torch.empty(1, 8, 8, 8, 96, dtype=BF16, device=DEV))
    xh = torch.zeros(1, 8, 8, 8, 48, dtype=BF16, device=DEV)
    with pytest.raises(RhoHipError):
        ops.head_conv3d(xh, None, None, False, torch.zeros(1, 32, 48, dtype=BF16, device=DEV), None, torch.empty(1, 1, 8, 8, 8, device=DEV))


# ================================================================================================ exact forms
# Integer operands (weight_table_cases.py; test_weight_table_cases_host.py proves every reference value representable): the kernels
# must equal the fp64 reference bit for bit, every output sits in a NaN-prefilled buffer between guard bands.


@pytest.mark.parametrize("cout", X.STEM_COUTS)
@pytest.mark.parametrize("shape", X.STEM_SHAPES, ids=str)
def test_stem_conv3d_exact_with_per_tile_statistics(ops, shape, cout):
    """y bit-equal to the fp64 conv3d; the statistics row of EVERY [n][tile] bit-equal to the sum / sum of squares over that tile's
    positions inside the volume; without a statistics buffer the same y."""
    N, D, H, W = shape
    c = X.stem_case(shape, cout)
    wp = X.stem_weight_layout(c["w"]).to(DEV).to(BF16)
    xd, bd = c["x"].to(DEV), c["b"].to(DEV)
    tiles = ops.stem_conv3d_tiles(D, H, W)
    assert tiles == X.ends_tiles(D, H, W)
    yflat, y = guarded((N, D, H, W, cout), BF16)
    sflat, st = guarded((N, tiles, 2, cout), torch.float32)
    ops.stem_conv3d(xd, wp, bd, y, st)
    torch.cuda.synchronize()
    assert_bit_equal(from_cl(y, 3), c["y"], f"stem {shape} cout {cout}: y")
    assert_bit_equal(st.cpu(), c["stats"], f"stem {shape} cout {cout}: statistics rows [n][tile][sum, sumsq][channel]")
    assert guards_intact(yflat) and guards_intact(sflat)
    y2flat, y2 = guarded((N, D, H, W, cout), BF16)
    ops.stem_conv3d(xd, wp, bd, y2, None)
    torch.cuda.synchronize()
    assert_bit_equal(from_cl(y2, 3), c["y"], f"stem {shape} cout {cout}: y without statistics")
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16)) and guards_intact(y2flat)


@pytest.mark.parametrize("C", X.HEAD_DGRAD_CS)
def test_stem_kernel_as_head_data_gradient_exact(ops, C):
    """The stem kernel in its second job (backward_plan.head_direct): dact = rho_stem_conv3d(dpred) with the mirrored-tap weights of
    _HeadDgradW equals the fp64 autograd of the head conv with respect to its input."""
    from torch import nn
    from rho_diffusion_amd.engine.weights import _HeadDgradW
    N, D, H, W = X.RAGGED
    c = X.head_dgrad_case(C)
    hd = _HeadDgradW(nn.Parameter(c["w"].to(DEV)), BF16)
    assert tuple(hd.w.shape) == (1, C, 32) and torch.equal(hd._perm.cpu(), X.head_dgrad_perm(C))
    flat, dact = guarded((N, D, H, W, C), BF16)
    ops.stem_conv3d(c["dpred"].to(DEV), hd.w, hd.zero_bias, dact)
    torch.cuda.synchronize()
    assert_bit_equal(from_cl(dact, 3), c["dact"], f"head data gradient C {C}")
    assert guards_intact(flat)


@pytest.mark.parametrize("prologue", X.HEAD_PROLOGUES, ids=["raw", "affine"])
@pytest.mark.parametrize("C", X.HEAD_CS)
@pytest.mark.parametrize("shape", X.HEAD_SHAPES, ids=str)
def test_head_conv3d_exact(ops, shape, C, prologue):
    """Integer operands, every per-tap partial within bf16: out bit-equal to the fp64 conv3d of the (affinely) activated input, with
    and without the bias.  The affine's b is non-zero everywhere: the conv pads the ACTIVATED tensor, so a kernel that pads before
    it activates is wrong on every face."""
    N, D, H, W = shape
    c = X.head_case(C, shape, prologue)
    xd = to_cl(c["x"], BF16)
    wp = X.head_weight_layout(c["w"]).to(DEV).to(BF16)
    pa, pb = (c["pre_a"].to(DEV), c["pre_b"].to(DEV)) if prologue else (None, None)
    for bias, want in ((c["bias"].to(DEV), c["out"]), (None, c["out_nobias"])):
        flat, out = guarded((N, 1, D, H, W), torch.float32)
        ops.head_conv3d(xd, pa, pb, False, wp, bias, out)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), want, f"head {shape} C {C} {prologue} bias {bias is not None}")
        assert guards_intact(flat)


@pytest.mark.parametrize("C", X.HEAD_CS)
def test_head_conv3d_silu_per_element_bound(ops, C):
    """Real-valued operands behind GroupNorm's affine and SiLU on the ragged shape, every element against the fp64 reference:
        |got - ref| <= 2^-9 (sum_tap sum_c |w act| + sum_tap |T|) (1 + slack) + 27 * 2^-24 sum_tap |T|
    from the kernel's rounding points: the activation is rounded to bf16 (the MFMA operand), each per-tap partial T to bf16 (its LDS
    form), 27 fp32 adds follow.  slack = 55 * 2^-15 covers silu_f (csrc/common.h) against fp64 before that first rounding, counted
    in weight_table_cases.py (SILU_SLACK: (7 + 3 |v|) 2^-24 relative at |v| <= 16), not measured.  (2^-9 is half of bf16's worst-case
    unit roundoff 2^-8: the bar holds because it multiplies the SUM of the magnitudes of 27 C independently rounded terms.)"""
    N, D, H, W = X.RAGGED
    c = X.head_silu_case(C)
    flat, out = guarded((N, 1, D, H, W), torch.float32)
    ops.head_conv3d(to_cl(c["x"], BF16), c["pre_a"].to(DEV), c["pre_b"].to(DEV), True, X.head_weight_layout(c["w"]).to(DEV).to(BF16),
                    c["bias"].to(DEV), out)
    torch.cuda.synchronize()
    worst = assert_within_abs(out.cpu(), c["out"], X.head_silu_bound(c), f"head SiLU C {C}")
    print(f"head SiLU C {C}: worst |got - ref| {worst:.3e}, smallest bound {float(X.head_silu_bound(c).min()):.3e}")
    assert guards_intact(flat)


def test_ends_dispatch_exactly_the_widths_the_exact_cases_cover(ops):
    """Every width the entry points accept is in the exact case tables; every other multiple of the channel granule is refused."""
    from rho_diffusion_amd.hip import RhoHipError
    x = torch.zeros(1, 1, 4, 8, 8, device=DEV)
    for cout in (96, 128):
        assert cout not in X.STEM_COUTS
        with pytest.raises(RhoHipError):
            ops.stem_conv3d(x, torch.zeros(1, cout, 32, dtype=BF16, device=DEV), torch.zeros(cout, device=DEV),
                            torch.empty(1, 4, 8, 8, cout, dtype=BF16, device=DEV))
    for C in (16, 48, 80, 112, 144, 160):
        assert C not in X.HEAD_CS
        with pytest.raises(RhoHipError):
            ops.head_conv3d(torch.zeros(1, 4, 8, 8, C, dtype=BF16, device=DEV), None, None, False, torch.zeros(1, 32, C, dtype=BF16, device=DEV),
                            None, torch.empty(1, 1, 4, 8, 8, device=DEV))
