"""-m gpu: forward convolution launches on small-integer operands, bit-equal to an fp64 reference.

The tolerance tests (test_gpu_kernels.py, test_gpu_bench_shapes.py, test_gpu_gemm1x1.py, test_gpu_splitk.py) bound a global rel-L2
and so cannot see one wrong element.  Here x in [-2, 2], w in [-1, 1], bias, residual, the additive row and the AFFINE prologue
(integer a, b per (sample, channel), no SiLU, applied before the zero padding) are integers: every product and every fp32 partial
sum is exact in any order, every stored value is an integer of at most 256, and the kernel must reproduce the reference exactly -
the failure names the index.  Every output (and statistics buffer, and k-split workspace) is prefilled with NaN and lies between
guard bands: an unwritten element and an out-of-range store both fail without faulting.  tests/exact_cases.py holds the cases;
tests/test_exact_cases_host.py proves on the CPU that the references stay inside the representability caps.

SiLU inside the conv loaders (pre_silu = 1) runs on integer u = a x + b, where the bf16 operand is uniquely bf16(silu64(u)):
test_forward_launch_with_silu_in_the_loader (gnb_silu = 1: test_gpu_exact_groupnorm.py).  The +gn_apply
epilogue and the fused GroupNorm-backward reduction (gnb_*) take their coefficients as inputs, so integer ones pin them bit for bit:
test_gpu_exact_groupnorm.py, next to the GroupNorm passes themselves."""
import pytest
import torch

import exact_cases as X
from exact_cases import BF16, F32
from exact_util import assert_bit_equal, assert_within_abs, bf16_round, check_bf16_exact, check_f32_exact, guarded, guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
_SEEN = set()             # variant names the launches of this module dispatched


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


def cl(t, dtype, dev=DEV):
    """[N, C, D, H, W] on the CPU -> channels-last [N, D, H, W, C] in the engine dtype on the device."""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dev).to(dtype)


def from_cl(y):
    return y.float().cpu().permute(0, 4, 1, 2, 3)


def padded_bias(b, coutp, dev=DEV):
    out = torch.zeros(coutp, device=dev)
    out[:b.numel()] = b.to(dev)
    return out


# variant each (case, dtype) must dispatch - asserted before the launch, so the coverage of the families cannot drift
EXPECT = {
    ("3d_basic", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("3d_basic", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("3d_bm128", "f32"): "k_conv<f32,3,3,3,BM=128,MAXP=5,NW=8,M16=0>",
    ("3d_bm128", "bf16"): "k_conv<bf16,3,3,3,BM=128,MAXP=5,NW=8,M16=1>",
    ("3d_ragged", "f32"): "k_conv<f32,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("3d_ragged", "bf16"): "k_conv<bf16,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("3d_tile512_ragged", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("3d_tile512_ragged", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("concat_straddle_bf16", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("concat_straddle_f32", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("3d_down_odd", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=28,NW=4,M16=0>",
    ("3d_down_odd", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=28,NW=4,M16=0>",
    ("3d_down_odd_bm128", "f32"): "k_conv<f32,3,3,3,BM=128,MAXP=14,NW=8,M16=0>",
    ("3d_down_odd_bm128", "bf16"): "k_conv<bf16,3,3,3,BM=128,MAXP=14,NW=8,M16=0>",
    ("2d_down", "f32"): "k_conv<f32,1,3,3,BM=64,MAXP=28,NW=4,M16=0>",
    ("2d_down", "bf16"): "k_conv<bf16,1,3,3,BM=64,MAXP=28,NW=4,M16=0>",
    ("1d_down", "f32"): "k_conv<f32,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("1d_down", "bf16"): "k_conv<bf16,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("3d_up", "f32"): "k_conv<f32,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("3d_up", "bf16"): "k_conv<bf16,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("2d_up", "f32"): "k_conv<f32,1,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("2d_up", "bf16"): "k_conv<bf16,1,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("1d_up", "f32"): "k_conv<f32,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("1d_up", "bf16"): "k_conv<bf16,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("2d_basic", "f32"): "k_conv<f32,1,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("2d_basic", "bf16"): "k_conv<bf16,1,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("1d_basic", "f32"): "k_conv<f32,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("1d_basic", "bf16"): "k_conv<bf16,1,1,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("3d_1x1", "f32"): "k_conv<f32,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("3d_1x1", "bf16"): "k_conv<bf16,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("1d_1x1", "f32"): "k_conv<f32,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("1d_1x1", "bf16"): "k_conv<bf16,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("2d_1x1_concat", "f32"): "k_conv<f32,1,1,1,BM=32,MAXP=10,NW=4,M16=0>",
    ("2d_1x1_concat", "bf16"): "k_conv<bf16,1,1,1,BM=32,MAXP=10,NW=4,M16=0>",
    ("1x1_stats", "f32"): "k_conv<f32,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("1x1_stats", "bf16"): "k_conv<bf16,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("split_y2", "f32"): "k_conv<f32,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("split_y2", "bf16"): "k_conv<bf16,1,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    ("split_two_y2_tiles", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("split_two_y2_tiles", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("head_f32", "f32"): "k_conv<f32,1,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("head_f32", "bf16"): "k_conv<bf16,1,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("y2_cl_res2", "f32"): "k_conv<f32,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("y2_cl_res2", "bf16"): "k_conv<bf16,3,3,3,BM=32,MAXP=10,NW=4,M16=0>",
    ("fold_ragged", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>+skip",
    ("fold_bm128", "bf16"): "k_conv<bf16,3,3,3,BM=128,MAXP=5,NW=8,M16=1>+skip",
    ("c32_one_tile", "bf16"): "k_conv32<bf16>",
    ("c32_n3_ragged", "bf16"): "k_conv32<bf16>",
    ("c32_plain", "bf16"): "k_conv32<bf16>",
    ("c32_n5", "bf16"): "k_conv32<bf16>",
    ("gemm_one_tile_one_kstep", "bf16"): "k_gemm1x1<bf16,256x128>",
    ("gemm_split_both_orientations", "bf16"): "k_gemm1x1<bf16,256x128>",
    ("gemm_res_stats_odd", "bf16"): "k_gemm1x1<bf16,256x128>",
    ("gemm_two_y2_tiles", "bf16"): "k_gemm1x1<bf16,256x128>",
    ("ksplit_ragged_2d", "f32"): "k_conv<f32,1,3,3,BM=128,MAXP=5,NW=8,M16=0>",
    ("ksplit_ragged_2d", "bf16"): "k_conv<bf16,1,3,3,BM=128,MAXP=5,NW=8,M16=1>",
    ("ksplit_1d_long_k", "f32"): "k_conv<f32,1,1,3,BM=128,MAXP=5,NW=8,M16=0>",
    ("ksplit_1d_long_k", "bf16"): "k_conv<bf16,1,1,3,BM=128,MAXP=5,NW=8,M16=1>",
    ("ksplit_1x1_pre_ragged", "f32"): "k_conv<f32,1,1,1,BM=128,MAXP=5,NW=8,M16=0>",
    ("ksplit_1x1_pre_ragged", "bf16"): "k_conv<bf16,1,1,1,BM=128,MAXP=5,NW=8,M16=0>",
}
# ... and the sub-pixel phase / parity-split launches
PHASE_VARIANTS = {
    "k_conv<bf16,1,1,2,BM=32,MAXP=10,NW=4,M16=0>",
    "k_conv<bf16,1,2,2,BM=64,MAXP=10,NW=4,M16=0>",
    "k_conv<bf16,3,1,1,BM=64,MAXP=10,NW=4,M16=1>",
    "k_conv<bf16,3,1,2,BM=64,MAXP=10,NW=4,M16=1>",
    "k_conv<bf16,3,2,1,BM=64,MAXP=10,NW=4,M16=1>",
    "k_conv<bf16,3,2,2,BM=32,MAXP=10,NW=4,M16=0>",
    "k_conv<bf16,3,2,2,BM=64,MAXP=10,NW=4,M16=1>",
    "k_conv<f32,1,1,2,BM=32,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,1,2,2,BM=64,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,3,1,1,BM=64,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,3,1,2,BM=64,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,3,2,1,BM=64,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,3,2,2,BM=32,MAXP=10,NW=4,M16=0>",
    "k_conv<f32,3,2,2,BM=64,MAXP=10,NW=4,M16=0>",
}


def build_launch(ops, c, dtype, dev=DEV, N=None, prep=True, silu=False):
    """Operands, NaN-prefilled guarded outputs and the descriptor of one forward case.  prep=False: weights are left uninitialised
    (for variant queries).  silu: the prologue coefficients of exact_cases.silu_fwd_operands and pre_silu = 1."""
    o = X.silu_fwd_operands(c) if silu else X.fwd_operands(c, N)
    N = o["N"]
    c1, c2, cout, split = c["c1"], c["c2"], c["cout"], c["split"]
    coutp = ((cout + 31) // 32) * 32

    def prepw(w):
        if prep:
            return ops.prep_conv_weight(w.to(dev), dtype)
        ck = ops.elem_chunk(dtype)
        return torch.empty(w[0, 0].numel(), ((w.shape[0] + 31) // 32) * 32, ((w.shape[1] + ck - 1) // ck) * ck, dtype=dtype, device=dev)

    L = dict(o=o, N=N)
    L["x1"] = cl(o["x"][:, :c1], dtype, dev)
    L["x2"] = cl(o["x"][:, c1:], dtype, dev) if c2 else None
    L["w"], L["b"] = prepw(o["w"]), padded_bias(o["b"], coutp, dev)
    L["pa"], L["pb"] = (o["pa"].to(dev), o["pb"].to(dev)) if c["pre"] else (None, None)
    Do, Ho, Wo = X.fwd_out_spatial(c)
    L["yflat"], L["y"] = guarded((N, Do, Ho, Wo, split), dtype, dev) if split > 0 else (None, None)
    L["y2flat"] = L["y2"] = None
    if split < cout:
        if c["y2"] == "cl":
            L["y2flat"], L["y2"] = guarded((N, Do, Ho, Wo, cout - split), dtype, dev)
        else:
            L["y2flat"], L["y2"] = guarded((N, cout - split, Do * Ho * Wo), F32 if c["y2"] == "cm_f32" else dtype, dev)
    L["res"] = cl(o["res"], dtype, dev) if c["res"] else None
    L["res2"] = cl(o["res2"], dtype, dev) if c["res2"] else None
    L["add"] = o["add"].to(dev).contiguous() if c["add"] else None
    skip = None
    if c["skip"]:
        s1 = c["skip"][0]
        L["sx1"], L["sx2"] = cl(o["sx"][:, :s1], dtype, dev), (cl(o["sx"][:, s1:], dtype, dev) if c["skip"][1] else None)
        L["sw"], L["sb"] = prepw(o["sw"]), padded_bias(o["sb"], coutp, dev)
        skip = (L["sx1"], L["sx2"], L["sw"], L["sb"])
    L["d"] = ops.make_conv_desc(L["x1"], L["x2"], L["w"], L["b"], kernel=c["kernel"], cout=cout, split=split, y=L["y"], y2=L["y2"],
                                stride_hw=c["stride"], up_hw=c["up"], pre_a=L["pa"], pre_b=L["pb"], pre_silu=bool(silu), res=L["res"],
                                res_add=L["add"], res_add_stride=cout if c["add"] else 0, y2_cl=c["y2"] == "cl", res2=L["res2"], skip=skip)
    return L


def check_outputs(c, L, ref, what):
    N, split, cout = L["N"], c["split"], c["cout"]
    if L["y"] is not None:
        assert_bit_equal(from_cl(L["y"]), ref[:, :split], f"{what}: y")
        assert guards_intact(L["yflat"]), f"{what}: store outside y"
    if L["y2"] is not None:
        got2 = from_cl(L["y2"]) if c["y2"] == "cl" else L["y2"].float().cpu().reshape(N, cout - split, *ref.shape[2:])
        assert_bit_equal(got2, ref[:, split:], f"{what}: y2")
        assert guards_intact(L["y2flat"]), f"{what}: store outside y2"


def stats_kind(variant):
    return "conv32" if variant.startswith("k_conv32") else "gemm" if variant.startswith("k_gemm1x1") else "k_conv"


FWD_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.FWD_CASES if not c["ksplit"] for dt in c["dtypes"]]


@pytest.mark.parametrize("c,dtype", FWD_PARAMS)
def test_forward_launch_is_bit_exact(ops, c, dtype):
    L = build_launch(ops, c, dtype)
    d = L["d"]
    sflat = sbuf = ids = None
    if c["stats"]:
        tiles = ops.conv_stats_tiles(d)
        assert tiles > 0
        sflat, sbuf = guarded((L["N"], tiles, 2, c["split"]), F32)
        d.stats = sbuf.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == EXPECT[(c["name"], _dn(dtype))], variant
    _SEEN.add(variant)
    _, ref = X.fwd_reference(c, L["o"])
    (check_bf16_exact if dtype == BF16 else check_f32_exact)(ref)
    if c["stats"]:
        ids = X.tile_ids(c, stats_kind(variant))
        assert tiles == int(ids.max()) + 1, (tiles, int(ids.max()) + 1)
    ops.conv_launch(d)
    torch.cuda.synchronize()
    check_outputs(c, L, ref, f"{c['name']} {variant}")
    if c["stats"]:
        # per tile row: channel sums and sums of squares of the stored outputs - exact integers below 2^24 in any summation order
        want = X.stats_reference(ref, ids)
        check_f32_exact(want, "statistics reference")
        assert_bit_equal(sbuf, want, f"{c['name']} {variant}: fused statistics [N, tile, (sum, sumsq), C]")
        assert guards_intact(sflat), "store outside the statistics buffer"


# the pre_silu cases that must take the compile-time-geometry form (whole 4 x 8 x 8 tiles of a stride-1 bf16 3x3x3 layer on the
# 16x16x32 layout, channels-last outputs, coefficients staged in LDS): apply_pre_regs<true>
SILU_GEO = {("3d_bm128", "bf16"), ("concat_straddle_bf16", "bf16"), ("fold_bm128", "bf16")}
# (every other k_conv case must report geo=0: ragged volumes, BM = 32, a channel-major y2, float32, the 2-D / 1-D / 1x1x1 layers)
SILU_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.SILU_FWD_CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("c,dtype", SILU_PARAMS)
def test_forward_launch_with_silu_in_the_loader(ops, c, dtype):
    """Every prologue case again with pre_silu = 1 and u = a x + b an integer in [-2, 6] (exact_cases.py, "SiLU in the conv loaders").
    bf16: the loader's operand is exactly bf16(silu64(u)) and every partial sum is exact, so each stored output equals the fp64
    reference after one rounding to its storage type (bf16 y / y2; the fp32 head exactly).  float32: the operand is silu_f(u), and
    every output element stays inside sum |w| (silu_f bound at u) + n 2^-24 sum |w s| (exact_cases.silu_fwd_bound).  The loader
    form is asserted from the detail string of rho_conv_variant: SILU_GEO names the bf16 3x3x3 cases that run the compile-time
    4 x 8 x 8 form, whose straight-line staging is the only caller of apply_pre_regs<true>; every other k_conv case must report
    geo=0 - the 3-D ones read per-batch coefficient rows from LDS through apply_pre<T>, the 2-D / 1-D / 1x1x1 ones read pre_a /
    pre_b per (sample, channel).  Virtual concat, the folded skip and k_conv32 (conv32.h) are among the cases."""
    L = build_launch(ops, c, dtype, silu=True)
    d = L["d"]
    detail = ops.conv_variant_detail(d)
    if EXPECT[(c["name"], _dn(dtype))].startswith("k_conv<"):
        want_detail = "geo=1" if (c["name"], _dn(dtype)) in SILU_GEO else "geo=0"
        assert detail == want_detail, f"{c['name']} {_dn(dtype)}: {detail}, the case exists for {want_detail}"
    sflat = None
    if c["stats"]:                                   # the launch keeps its statistics output (not integers here: only its guards count)
        sflat, sbuf = guarded((L["N"], ops.conv_stats_tiles(d), 2, c["split"]), F32)
        d.stats = sbuf.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == EXPECT[(c["name"], _dn(dtype))], variant
    _, ref = X.silu_fwd_reference(c, L["o"], dtype)
    ops.conv_launch(d)
    torch.cuda.synchronize()
    what = f"{c['name']} {variant} pre_silu"
    assert sflat is None or guards_intact(sflat), what + ": store outside the statistics buffer"
    if dtype == BF16:
        want = ref.clone()
        split = c["split"]
        want[:, :split] = bf16_round(ref[:, :split])
        if c["y2"] != "cm_f32":
            want[:, split:] = bf16_round(ref[:, split:])
        check_outputs(c, L, want, what)
    else:
        N, split, cout = L["N"], c["split"], c["cout"]
        bound = X.silu_fwd_bound(c, L["o"])
        worst = 0.0
        if L["y"] is not None:
            assert guards_intact(L["yflat"]), what + ": store outside y"
            worst = max(worst, float(((from_cl(L["y"]).double() - ref[:, :split]).abs() / bound[:, :split]).max()))
            assert_within_abs(from_cl(L["y"]), ref[:, :split], bound[:, :split], what + ": y")
        if L["y2"] is not None:
            assert guards_intact(L["y2flat"]), what + ": store outside y2"
            got2 = from_cl(L["y2"]) if c["y2"] == "cl" else L["y2"].float().cpu().reshape(N, cout - split, *ref.shape[2:])
            worst = max(worst, float(((got2.double() - ref[:, split:]).abs() / bound[:, split:]).max()))
            assert_within_abs(got2, ref[:, split:], bound[:, split:], what + ": y2")
        print(f"measured: {what}: worst error {worst:.3f} of the derived bound")


KSPLIT_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.FWD_CASES if c["ksplit"] for dt in c["dtypes"]]


@pytest.mark.parametrize("c,dtype", KSPLIT_PARAMS)
def test_ksplit_launch_equals_the_reference_and_the_unsplit_launch(ops, c, dtype):
    """The k-split with an attached workspace (fp32 slabs, reduced in slab order) at the smallest batch at which the launch is
    offered one; the workspace is prefilled with NaN bit patterns.  Integer partial sums are exact, so split and unsplit launches
    are EQUAL, not close."""
    N = None
    for n in range(1, 17):
        if ops.conv_workspace_bytes(build_launch(ops, c, dtype, N=n, prep=False)["d"]) > 0:
            N = n
            break
    assert N is not None, "no batch up to 16 splits"
    N = max(N, 3)                                  # (three samples: tiles and slabs straddle sample boundaries)
    outs = []
    for with_ws in (True, False):
        L = build_launch(ops, c, dtype, N=N)
        d = L["d"]
        want = ops.conv_workspace_bytes(d)
        assert want >= 2 * L["y"].numel() * 4 and want % (L["y"].numel() * 4) == 0, want
        variant = ops.conv_variant(d)
        assert variant == EXPECT[(c["name"], _dn(dtype))], variant
        _SEEN.add(variant + "+ksplit" if with_ws else variant)
        if with_ws:
            ws = ops.attach_conv_workspace([d], DEV)
            assert ws is not None and d.ws_bytes == want
            ws.fill_(0xFF)
        _, ref = X.fwd_reference(c, L["o"])
        (check_bf16_exact if dtype == BF16 else check_f32_exact)(ref)
        ops.conv_launch(d)
        torch.cuda.synchronize()
        check_outputs(c, L, ref, f"{c['name']} {variant} {'split' if with_ws else 'unsplit'}")
        outs.append(L["y"].clone())
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))


# ----------------------------------------------------------------------------- sub-pixel phases
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("kernel,shape,up,cin,cout", X.PHASE_CASES, ids=["3x2x2", "1x2x2", "1x1x2"])
def test_upsample_conv_as_subpixel_phases_is_bit_exact(ops, dtype, kernel, shape, up, cin, cout):
    """Upsample + conv as one 2-tap launch per output parity: all parities write one NaN-prefilled output.  The phase weights are
    sums of two / four integer taps - still integers."""
    N, D, H, W = shape
    o = X.phase_operands(kernel, shape, cin, cout)
    ref = X.conv5(o["x"].double(), o["w"].double(), o["b"].double(), up=up)
    (check_bf16_exact if dtype == BF16 else check_f32_exact)(ref)
    x, wt, b = cl(o["x"], dtype), o["w"].to(DEV), padded_bias(o["b"], ((cout + 31) // 32) * 32)
    yflat, y = guarded((N, D, H * (2 if up[0] else 1), W * (2 if up[1] else 1), cout), dtype)
    keep = []
    for a in ((1, 2) if up[0] else (0,)):
        for c in ((1, 2) if up[1] else (0,)):
            wp = ops.prep_conv_weight_phase(wt, dtype, (a, c))
            kk = (kernel[0], 2 if a else kernel[1], 2 if c else kernel[2])
            d = ops.make_conv_desc(x, None, wp, b, kernel=kk, cout=cout, split=cout, y=y, y2=None, phase_hw=(a, c))
            variant = ops.conv_variant(d)
            assert variant.startswith(f"k_conv<{_dn(dtype)},{kk[0]},{kk[1]},{kk[2]},") and variant in PHASE_VARIANTS, variant
            _SEEN.add(variant)
            keep.append((wp, d))
            ops.conv_launch(d)
    torch.cuda.synchronize()
    assert_bit_equal(from_cl(y), ref, f"phases {kernel} {_dn(dtype)}")
    assert guards_intact(yflat)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("shape,cin,cout", X.S2_CASES, ids=["32to64"])
def test_stride2_conv_as_parity_split_is_bit_exact(ops, dtype, shape, cin, cout):
    """Downsample's conv as four stride-1 launches (3x1x1, 3x1x2, 3x2x1, 3x2x2), accumulated in place through the stored output:
    every running sum is an integer of at most 256 (host test), so the result equals the strided conv exactly."""
    N, D, H, W = shape
    o = X.phase_operands((3, 3, 3), shape, cin, cout, tag="s2")
    ref = X.conv5(o["x"].double(), o["w"].double(), o["b"].double(), stride=(2, 2))
    x, wt = cl(o["x"], dtype), o["w"].to(DEV)
    coutp = ((cout + 31) // 32) * 32
    bp, zb = padded_bias(o["b"], coutp), torch.zeros(coutp, device=DEV)
    yflat, y = guarded((N, D, H // 2, W // 2, cout), dtype)
    keep, kernels, i = [], set(), 0
    for a in (0, 1):
        for c in (0, 1):
            sel = (X.S2_FWD_SEL[a], X.S2_FWD_SEL[c])
            ws = ops.prep_conv_weight_sel(wt, dtype, sel)
            kk = (3, len(sel[0]), len(sel[1]))
            d = ops.make_conv_desc(x, None, ws, bp if i == 0 else zb, kernel=kk, cout=cout, split=cout, y=y, y2=None,
                                   res=y if i > 0 else None, phase_dgrad_hw=(a + 1, c + 1))
            variant = ops.conv_variant(d)
            assert variant.startswith(f"k_conv<{_dn(dtype)},{kk[0]},{kk[1]},{kk[2]},") and variant in PHASE_VARIANTS, variant
            _SEEN.add(variant)
            kernels.add(kk)
            keep.append((ws, d))
            ops.conv_launch(d)
            i += 1
    torch.cuda.synchronize()
    assert kernels == {(3, 1, 1), (3, 1, 2), (3, 2, 1), (3, 2, 2)}
    assert_bit_equal(from_cl(y), ref, f"parity split {_dn(dtype)}")
    assert guards_intact(yflat)


# ----------------------------------------------------------------------------- coverage
FAMILIES = {
    "k_conv bf16 M16=1 BM=64": lambda v: v.startswith("k_conv<bf16,3,3,3,BM=64,") and v.endswith("M16=1>"),
    "k_conv bf16 M16=1 BM=128": lambda v: v.startswith("k_conv<bf16,3,3,3,BM=128,") and v.endswith("M16=1>"),
    "+skip BM=64": lambda v: "BM=64," in v and v.endswith("M16=1>+skip"),
    "+skip BM=128": lambda v: "BM=128," in v and v.endswith("M16=1>+skip"),
    "k_conv32": lambda v: v == "k_conv32<bf16>",
    "k_gemm1x1": lambda v: v == "k_gemm1x1<bf16,256x128>",
    "k-split": lambda v: v.endswith("+ksplit"),
}
for _dt in ("f32", "bf16"):
    for _bm in (32, 64, 128):
        FAMILIES[f"k_conv {_dt} M16=0 BM={_bm}"] = lambda v, dt=_dt, bm=_bm: v.startswith(f"k_conv<{dt},") and f"BM={bm}," in v and "M16=0>" in v
    for _mp in ("MAXP=10", "MAXP=5", "MAXP=14", "MAXP=28"):
        FAMILIES[f"k_conv {_dt} M16=0 {_mp}"] = lambda v, dt=_dt, mp=_mp: v.startswith(f"k_conv<{dt},") and mp + "," in v and "M16=0>" in v
    for _k in ("3,3,3", "1,3,3", "1,1,3", "1,1,1", "3,2,2", "1,2,2", "1,1,2", "3,1,1", "3,1,2", "3,2,1"):
        FAMILIES[f"k_conv {_dt} {_k}"] = lambda v, dt=_dt, k=_k: v.startswith(f"k_conv<{dt},{k},")


def test_the_exact_forward_cases_cover_every_kernel_family(ops):
    """The set of variant names this module's launches dispatch (collected from rho_conv_variant; '+ksplit' marks a launch that ran
    with a workspace) holds one member of every family of forward kernels."""
    want = set(EXPECT.values()) | PHASE_VARIANTS | {EXPECT[(c["name"], _dn(dt))] + "+ksplit" for c in X.FWD_CASES if c["ksplit"] for dt in c["dtypes"]}
    assert _SEEN <= want, sorted(_SEEN - want)              # (every launch asserted its own pinned name before it ran)
    missing = [f for f, pred in FAMILIES.items() if not any(pred(v) for v in want)]
    assert not missing, missing

