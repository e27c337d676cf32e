"""-m gpu: data gradient, weight gradient and the pooling / channel-sum helpers on small-integer operands, bit-equal to fp64
autograd (see test_gpu_exact_conv.py for the idea; tests/exact_cases.py for the cases, tests/test_exact_cases_host.py for the proof
that the references are exactly representable).  dY is sparse with |dy| <= 1; dX passes through the engine dtype (integers of at
most 256), dW and dbias stay in fp32 (integers far below 2^24), so neither the atomic flush nor the ordered-slab flush of the weight
gradient may differ from the reference in a single bit.  Every output lies between guard bands; outputs that are written (not
accumulated into) are prefilled with NaN.

Left out on purpose: SiLU in the prologue.  The fused GroupNorm-backward reduction / apply epilogues (gnb_* / gna_*) are pinned with
integer coefficients in test_gpu_exact_groupnorm.py."""
import pytest
import torch
import torch.nn.functional as F

import exact_cases as X
from exact_cases import BF16, F32
from exact_util import assert_bit_equal, assert_within_abs, check_bf16_exact, check_f32_exact, guarded, guarded_copy, guards_intact, int_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
_SEEN = set()


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


@pytest.fixture(scope="module")
def refs():
    """name -> (operands, fp64 autograd reference), computed once per case and left unchanged."""
    cache = {}

    def get(c):
        if c["name"] not in cache:
            o = X.bwd_operands(c)
            cache[c["name"]] = (o, X.bwd_reference(c, o))
        return cache[c["name"]]
    return get


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


def cl(t, dtype, dev=DEV):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(dev).to(dtype)


def from_cl(y):
    return y.float().cpu().permute(0, 4, 1, 2, 3)


def _exact(dtype):
    return check_bf16_exact if dtype == BF16 else check_f32_exact


BWD_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.BWD_CASES for dt in c["dtypes"]]
# (a data-gradient launch writes whole 32-channel tiles and reads dY rows of whole K chunks)
DGRAD_PARAMS = [p for p in BWD_PARAMS if (p.values[0]["c1"] + p.values[0]["c2"]) % 32 == 0 and p.values[0]["cout"] % 32 == 0]


# ----------------------------------------------------------------------------- data gradient
@pytest.mark.parametrize("c,dtype", DGRAD_PARAMS)
def test_data_gradient_is_bit_exact(ops, refs, c, dtype):
    """The forward kernel on dY with flipped / transposed weights (rho_prep_conv_weight_dgrad): plain; zero-stuffed (zs_hw) for the
    strided cases; two channels-last outputs for a concatenated input, the second accumulated onto an integer base; the gradient
    w.r.t. the upsampled input followed by rho_pool2x_sum."""
    o, r = refs(c)
    N, c1, c2 = c["N"], c["c1"], c["c2"]
    cin = c1 + c2
    D, H, W = c["spatial"]
    _exact(dtype)(r["dx"], "dX")
    dy = cl(o["dy"], dtype)
    wd = ops.prep_conv_weight_dgrad(o["w"].to(DEV), dtype)
    zb = torch.zeros(wd.shape[1], device=DEV)
    what = f"dgrad {c['name']} {_dn(dtype)}"
    if any(c["up"]):
        Do, Ho, Wo = X.fwd_out_spatial(c)
        uflat, du = guarded((N, Do, Ho, Wo, cin), dtype)
        d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=cin, split=cin, y=du, y2=None)
        _SEEN.add(ops.conv_variant(d))
        ops.conv_launch(d)
        xflat, dx = guarded((N, D, H, W, cin), dtype)
        ops.pool2x_sum(du, dx, c["up"])
        torch.cuda.synchronize()
        assert guards_intact(uflat) and guards_intact(xflat)
        assert_bit_equal(from_cl(dx), r["dx"], what + " (upsample form + pool2x_sum)")
    elif c["stride"] != (1, 1):
        xflat, dx = guarded((N, D, H, W, cin), dtype)
        zs = (int(c["stride"][0] == 2), int(c["stride"][1] == 2))
        d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=cin, split=cin, y=dx, y2=None, zs_hw=zs, out_hw=(H, W))
        _SEEN.add(ops.conv_variant(d))
        ops.conv_launch(d)
        torch.cuda.synchronize()
        assert guards_intact(xflat)
        assert_bit_equal(from_cl(dx), r["dx"], what + " (zero-stuffed)")
    elif "base" in o:
        f1, dx1 = guarded((N, D, H, W, c1), dtype)
        f2, dx2 = guarded_copy(o["base"].permute(0, 2, 3, 4, 1), dtype)
        d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=cin, split=c1, y=dx1, y2=dx2, y2_cl=True, res2=dx2)
        _SEEN.add(ops.conv_variant(d))
        ops.conv_launch(d)
        torch.cuda.synchronize()
        assert guards_intact(f1) and guards_intact(f2)
        assert_bit_equal(from_cl(dx1), r["dx"][:, :c1], what + " (first source)")
        assert_bit_equal(from_cl(dx2), r["dx"][:, c1:] + o["base"].double(), what + " (second source, accumulated onto its base)")
    else:
        xflat, dx = guarded((N, D, H, W, cin), dtype)
        d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=cin, split=cin, y=dx, y2=None)
        _SEEN.add(ops.conv_variant(d))
        ops.conv_launch(d)
        torch.cuda.synchronize()
        assert guards_intact(xflat)
        assert_bit_equal(from_cl(dx), r["dx"], what)


# ----------------------------------------------------------------------------- weight gradient
# the k_wgrad / k_wgrad1 instantiation each (case, dtype) must dispatch
EXPECT_W = {
    ("3d_basic", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_basic", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("3d_ragged", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_ragged", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("3d_concat", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_concat", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("3d_multi_ragged", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_multi_ragged", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("3d_multi_whole", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_multi_whole", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("2d_multi_ragged", "f32"): "k_wgrad<f32,1,3,3,MAXP=10,PRE=0>",
    ("2d_multi_ragged", "bf16"): "k_wgrad<bf16,1,3,3,MAXP=10,PRE=0>",
    ("3d_pre", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=1>",
    ("3d_pre", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=1>",
    ("3d_down", "f32"): "k_wgrad<f32,3,3,3,MAXP=28,PRE=0>",
    ("3d_down", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=28,PRE=0>",
    ("3d_down_odd", "f32"): "k_wgrad<f32,3,3,3,MAXP=28,PRE=0>",
    ("3d_down_odd", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=28,PRE=0>",
    ("2d_down", "f32"): "k_wgrad<f32,1,3,3,MAXP=28,PRE=0>",
    ("2d_down", "bf16"): "k_wgrad<bf16,1,3,3,MAXP=28,PRE=0>",
    ("3d_up", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_up", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("2d_basic", "f32"): "k_wgrad<f32,1,3,3,MAXP=10,PRE=0>",
    ("2d_basic", "bf16"): "k_wgrad<bf16,1,3,3,MAXP=10,PRE=0>",
    ("1d_basic", "f32"): "k_wgrad<f32,1,1,3,MAXP=10,PRE=0>",
    ("1d_basic", "bf16"): "k_wgrad<bf16,1,1,3,MAXP=10,PRE=0>",
    ("3d_1x1", "f32"): "k_wgrad<f32,1,1,1,MAXP=10,PRE=0>",
    ("3d_1x1", "bf16"): "k_wgrad1<bf16>",
    ("1x1_straddle_odd", "f32"): "k_wgrad<f32,1,1,1,MAXP=10,PRE=0>",
    ("1x1_single_chunk", "f32"): "k_wgrad<f32,1,1,1,MAXP=10,PRE=0>",
    ("1x1_straddle_odd_pre", "f32"): "k_wgrad<f32,1,1,1,MAXP=10,PRE=1>",
    ("3d_cout48", "f32"): "k_wgrad<f32,3,3,3,MAXP=10,PRE=0>",
    ("3d_cout48", "bf16"): "k_wgrad<bf16,3,3,3,MAXP=10,PRE=0,GEO=1>",
    ("1x1_wgrad1_wide", "bf16"): "k_wgrad1<bf16>",
}


def _wgrad_launch(ops, c, dtype, o, deterministic, silu=False):
    """conv_wgrad of one case into guarded, zeroed fp32 buffers; returns (dw buffer, dbias, variant).  silu: pre_silu = 1."""
    c1, c2, cout = c["c1"], c["c2"], c["cout"]
    act_in = o["x"]                                     # the prologue (if any) is recomputed by the kernel's loader
    x1, x2 = cl(act_in[:, :c1], dtype), (cl(act_in[:, c1:], dtype) if c2 else None)
    if any(c["up"]):
        x1 = ops.upsample2x(x1, c["up"])
    dy = cl(o["dy"], dtype)
    wf = ops.prep_conv_weight(o["w"].to(DEV), dtype)            # (only its shape matters to the descriptor)
    zb = torch.zeros(wf.shape[1], device=DEV)
    pa, pb = (o["pa"].to(DEV), o["pb"].to(DEV)) if c["pre"] else (None, None)
    d = ops.make_conv_desc(x1, x2, wf, zb, kernel=c["kernel"], cout=cout, split=cout, y=dy, y2=None, stride_hw=c["stride"],
                           pre_a=pa, pre_b=pb, pre_silu=bool(silu))
    variant = ops.conv_wgrad_variant(d, dy.shape[-1])
    assert variant == EXPECT_W[(c["name"], _dn(dtype))], variant
    _SEEN.add(variant)
    wflat, dwbuf = guarded_copy(torch.zeros(tuple(wf.shape)), F32)
    bflat, dbias = guarded_copy(torch.zeros(wf.shape[1]), F32)
    was = ops.deterministic()
    ops.set_deterministic(deterministic)
    try:
        ops.conv_wgrad(d, dy, dwbuf, dbias)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert guards_intact(wflat), "store outside the dW buffer"
    assert guards_intact(bflat), "store outside dbias"
    return dwbuf, dbias, variant, (x1, x2, dy, wf, zb, pa, pb)


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "slabs"])
@pytest.mark.parametrize("c,dtype", BWD_PARAMS)
def test_weight_gradient_is_bit_exact(ops, refs, c, dtype, deterministic):
    """rho_conv_nd_wgrad (fp32 atomics) and rho_conv_nd_wgrad_ws (ordered slabs) + rho_wgrad_finalize: dW equals fp64 autograd bit
    for bit, dbias equals the channel sums of dY and its padded tail [cout:coutp] is exactly 0."""
    o, r = refs(c)
    check_f32_exact(r["dw"], "dW")
    dwbuf, dbias, variant, keep = _wgrad_launch(ops, c, dtype, o, deterministic)
    cout = c["cout"]
    gflat, grad = guarded(tuple(o["w"].shape), F32)
    ops.wgrad_finalize(dwbuf, grad)
    torch.cuda.synchronize()
    what = f"wgrad {c['name']} {variant} {'slabs' if deterministic else 'atomic'}"
    assert guards_intact(gflat)
    assert_bit_equal(grad, r["dw"], what + ": dW [cout, cin, kd, kh, kw]")
    assert_bit_equal(dbias[:cout], r["db"], what + ": dbias")
    assert_bit_equal(dbias[:cout], o["dy"].double().sum((0, 2, 3, 4)), what + ": dbias vs channel sums")
    if dbias.numel() > cout:
        assert bool((dbias[cout:] == 0).all()), what + ": padded dbias tail"


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "slabs"])
@pytest.mark.parametrize("c,dtype", [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.SILU_BWD_CASES for dt in c["dtypes"]])
def test_weight_gradient_with_silu_in_the_loader(ops, c, dtype, deterministic):
    """The prologue cases with pre_silu = 1, integer u = a x + b in [-2, 6] and dY in +-1 (exact_cases.py): the bf16 loader hands
    the MFMA exactly bf16(silu64(u)), every sum is exact on the 2^-10 grid and dW after rho_wgrad_finalize equals fp64 bit for
    bit, through the atomics and the ordered slabs; the float32 kernel is held per element to sum |dY| (silu_f bound at u) +
    n 2^-24 sum |dY s|."""
    o = X.silu_bwd_operands(c)
    dw, mag, bound = X.silu_wgrad_reference(c, o, dtype)
    dwbuf, dbias, variant, keep = _wgrad_launch(ops, c, dtype, o, deterministic, silu=True)
    gflat, grad = guarded(tuple(o["w"].shape), F32)
    ops.wgrad_finalize(dwbuf, grad)
    torch.cuda.synchronize()
    assert guards_intact(gflat)
    what = f"wgrad {c['name']} {variant} pre_silu {'slabs' if deterministic else 'atomic'}: dW [cout, cin, kd, kh, kw]"
    if dtype == BF16:
        assert_bit_equal(grad, dw, what)
    else:
        worst = assert_within_abs(grad, dw, bound, what)
        print(f"measured: {what}: worst error {worst:.3e}, bound from {float(bound.min()):.3e}")
    assert_bit_equal(dbias[:c["cout"]], o["dy"].double().sum((0, 2, 3, 4)), what + ": dbias")


@pytest.mark.parametrize("name,dtype", [("3d_pre", BF16), ("3d_pre", F32), ("3d_1x1", BF16), ("1x1_straddle_odd", F32)],
                         ids=["3d_pre-bf16", "3d_pre-f32", "1x1-bf16", "1x1-f32"])
def test_wgrad_finalize_row_permutation_and_accumulate(ops, refs, name, dtype):
    """rho_wgrad_finalize with row_src (buffer row r -> parameter row row_src[r]) accumulating onto an integer-valued gradient."""
    c = X.BWD_BY_NAME[name]
    o, r = refs(c)
    dwbuf, _, _, keep = _wgrad_launch(ops, c, dtype, o, False)
    cout = c["cout"]
    perm = torch.tensor([(5 * i + 3) % cout for i in range(cout)])
    assert sorted(perm.tolist()) == list(range(cout))
    base = int_tensor(tuple(o["w"].shape), "fin_base" + name, 5.0, 16)
    gflat, grad = guarded_copy(base, F32)
    ops.wgrad_finalize(dwbuf, grad, row_src=perm.to(torch.int32).to(DEV), accumulate=True)
    torch.cuda.synchronize()
    want = base.double()
    want[perm] += r["dw"]
    check_f32_exact(want)
    assert guards_intact(gflat)
    assert_bit_equal(grad, want, f"finalize {name} {_dn(dtype)}: permuted rows accumulated onto a gradient")
    ops.wgrad_finalize(dwbuf, grad, accumulate=True)
    torch.cuda.synchronize()
    assert_bit_equal(grad, want + r["dw"], f"finalize {name} {_dn(dtype)}: accumulated a second time, identity rows")


# ----------------------------------------------------------------------------- sub-pixel phases: data and weight gradient
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("kernel,shape,up,cin,cout", X.PHASE_CASES, ids=["3x2x2", "1x2x2", "1x1x2"])
def test_phase_data_and_weight_gradient_are_bit_exact(ops, dtype, kernel, shape, up, cin, cout):
    """Upsample + conv as sub-pixel phases: each phase's data gradient is a 2-tap conv of its parity of dY (phase_dgrad_hw),
    accumulated in place; each phase's weight gradient is a 2-tap k_wgrad routed to the 3-tap parameter (rho_wgrad_finalize_phase)."""
    from rho_diffusion_amd import hip
    N, D, H, W = shape
    o = X.phase_operands(kernel, shape, cin, cout)
    xr = o["x"].double().requires_grad_(True)
    wr = o["w"].double().requires_grad_(True)
    br = o["b"].double().requires_grad_(True)
    ref = X.conv5(xr, wr, br, up=up)
    dyc = int_tensor(tuple(ref.shape), "ph_dy", 0.45, 1)
    ref.backward(dyc.double())
    _exact(dtype)(xr.grad, "dX")
    check_f32_exact(wr.grad, "dW")
    x, wt, dy = cl(o["x"], dtype), o["w"].to(DEV), cl(dyc, dtype)
    xflat, dx = guarded((N, D, H, W, cin), dtype)
    zb = torch.zeros(((cin + 31) // 32) * 32, device=DEV)
    coutp = ((cout + 31) // 32) * 32
    gflat, grad = guarded_copy(torch.zeros(tuple(o["w"].shape)), F32)
    bflat, dbias = guarded_copy(torch.zeros(coutp), F32)
    keep, i = [], 0
    for a in ((1, 2) if up[0] else (0,)):
        for c in ((1, 2) if up[1] else (0,)):
            kk = (kernel[0], 2 if a else kernel[1], 2 if c else kernel[2])
            wd = ops.prep_conv_weight_phase(wt, dtype, (a, c), dgrad=True)
            dd = ops.make_conv_desc(dy, None, wd, zb, kernel=kk, cout=cin, split=cin, y=dx, y2=None, res=dx if i > 0 else None,
                                    phase_dgrad_hw=(a, c))
            _SEEN.add(ops.conv_variant(dd))
            ops.conv_launch(dd)
            wp = ops.prep_conv_weight_phase(wt, dtype, (a, c))
            df = ops.make_conv_desc(x, None, wp, torch.zeros(coutp, device=DEV), kernel=kk, cout=cout, split=cout, y=dy, y2=None, phase_hw=(a, c))
            variant = ops.conv_wgrad_variant(df, dy.shape[-1])
            assert variant == f"k_wgrad<{_dn(dtype)},{kk[0]},{kk[1]},{kk[2]},MAXP=10,PRE=0>", variant
            _SEEN.add(variant)
            wflat, dwb = guarded_copy(torch.zeros(tuple(wp.shape)), F32)
            ops.conv_wgrad(df, dy, dwb, dbias)
            hip.check(hip.lib().rho_wgrad_finalize_phase(dwb.data_ptr(), grad.data_ptr(), cout, cin, kernel[0], kernel[1], kernel[2], a, c,
                                                         wp.shape[1], wp.shape[2], 1, hip.stream()), "rho_wgrad_finalize_phase")
            keep.append((wd, dd, wp, df, wflat, dwb))
            i += 1
    torch.cuda.synchronize()
    assert guards_intact(xflat) and guards_intact(gflat) and guards_intact(bflat) and all(guards_intact(k[4]) for k in keep)
    assert_bit_equal(from_cl(dx), xr.grad, f"phase dgrad {kernel} {_dn(dtype)}")
    assert_bit_equal(grad, wr.grad, f"phase wgrad {kernel} {_dn(dtype)}")
    assert_bit_equal(dbias[:cout], br.grad, f"phase dbias {kernel} {_dn(dtype)}")
    assert bool((dbias[cout:] == 0).all())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("shape,cin,cout", X.S2_CASES, ids=["32to64"])
def test_stride2_parity_split_data_gradient_is_bit_exact(ops, dtype, shape, cin, cout):
    """Data gradient of the stride-(1, 2, 2) conv as one launch per parity of dX (phase_hw; disjoint rows of one NaN-prefilled dX)."""
    N, D, H, W = shape
    o = X.phase_operands((3, 3, 3), shape, cin, cout, tag="s2")
    xr = o["x"].double().requires_grad_(True)
    ref = X.conv5(xr, o["w"].double(), None, stride=(2, 2))
    dyc = int_tensor(tuple(ref.shape), "s2_dy", 0.45, 1)
    ref.backward(dyc.double())
    _exact(dtype)(xr.grad, "dX")
    dy, wt = cl(dyc, dtype), o["w"].to(DEV)
    xflat, dx = guarded((N, D, H, W, cin), dtype)
    zb = torch.zeros(((cin + 31) // 32) * 32, device=DEV)
    keep = []
    for a in (0, 1):
        for c in (0, 1):
            sel = (X.S2_BWD_SEL[a], X.S2_BWD_SEL[c])
            wd = ops.prep_conv_weight_sel(wt, dtype, sel, flip_d=True, dgrad=True)
            dd = ops.make_conv_desc(dy, None, wd, zb, kernel=(3, len(sel[0]), len(sel[1])), cout=cin, split=cin, y=dx, y2=None,
                                    phase_hw=(a + 1, c + 1))
            _SEEN.add(ops.conv_variant(dd))
            keep.append((wd, dd))
            ops.conv_launch(dd)
    torch.cuda.synchronize()
    assert guards_intact(xflat)
    assert_bit_equal(from_cl(dx), xr.grad, f"parity-split dgrad {_dn(dtype)}")


# ----------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
def test_chan_sum_pool_and_avgpool_helpers_are_bit_exact(ops, dtype):
    """rho_chan_sum (both outputs, acc_c), rho_pool2x_sum, rho_avgpool2x and rho_avgpool2x_bwd on integers (multiples of 4 for the
    two average-pool ops, so the x 1/4 is exact)."""
    N, C, D, H, W = 3, 64, 4, 6, 8
    x = int_tensor((N, C, D, H, W), "hx", 0.75, 2)
    xc = cl(x, dtype)
    # chan_sum: per (sample, channel) into a strided row, per channel accumulated onto ones
    nflat, out_nc = guarded_copy(torch.zeros(N, 80), F32)
    cflat, out_c = guarded_copy(torch.ones(C), F32)
    ops.chan_sum(xc, out_nc[:, 8:].data_ptr(), None, nc_stride=80)
    nc = torch.full((N, C), float("nan"), device=DEV)
    ops.chan_sum(xc, nc, out_c, acc_c=True)
    torch.cuda.synchronize()
    assert guards_intact(nflat) and guards_intact(cflat)
    assert_bit_equal(out_nc[:, 8:72], x.double().sum((2, 3, 4)), "chan_sum out_nc (strided)")
    assert bool((out_nc[:, :8] == 0).all()) and bool((out_nc[:, 72:] == 0).all())
    assert_bit_equal(nc, x.double().sum((2, 3, 4)), "chan_sum out_nc")
    assert_bit_equal(out_c, 1 + x.double().sum((0, 2, 3, 4)), "chan_sum out_c accumulated")
    for hw in ((1, 1), (0, 1)):
        kh, kw = (2 if hw[0] else 1), (2 if hw[1] else 1)
        # pool2x_sum: the backward of the nearest upsample, plain and accumulated
        g = int_tensor((N, C, D, H * kh, W * kw), f"hg{hw}", 0.75, 2)
        want = F.avg_pool3d(g.double(), (1, kh, kw)) * (kh * kw)
        pflat, dx = guarded((N, D, H, W, C), dtype)
        ops.pool2x_sum(cl(g, dtype), dx, hw)
        torch.cuda.synchronize()
        assert guards_intact(pflat)
        assert_bit_equal(from_cl(dx), want, f"pool2x_sum {hw}")
        ops.pool2x_sum(cl(g, dtype), dx, hw, accumulate=True)
        torch.cuda.synchronize()
        assert_bit_equal(from_cl(dx), 2 * want, f"pool2x_sum {hw} accumulated")
        # avgpool2x and its backward on multiples of 4; odd extents: floor output, the last row / column gets no gradient
        Hh, Ww = H + 1, W + 1
        a = 4 * int_tensor((N, C, D, Hh, Ww), f"ha{hw}", 0.75, 2)
        ar = a.double().requires_grad_(True)
        pooled = F.avg_pool3d(ar, (1, kh, kw))
        aflat, y = guarded((N, D, Hh // kh, Ww // kw, C), dtype)
        ops.avgpool2x(cl(a, dtype), hw, out=y)
        torch.cuda.synchronize()
        assert guards_intact(aflat)
        assert_bit_equal(from_cl(y), pooled.detach(), f"avgpool2x {hw}")
        gy = 4 * int_tensor(tuple(pooled.shape), f"hgy{hw}", 0.75, 2)
        pooled.backward(gy.double())
        bflat, dxa = guarded((N, D, Hh, Ww, C), dtype)
        ops.avgpool2x_bwd(cl(gy, dtype), dxa, hw)
        torch.cuda.synchronize()
        assert guards_intact(bflat)
        assert_bit_equal(from_cl(dxa), ar.grad, f"avgpool2x_bwd {hw}")
        ops.avgpool2x_bwd(cl(gy, dtype), dxa, hw, accumulate=True)
        torch.cuda.synchronize()
        assert_bit_equal(from_cl(dxa), 2 * ar.grad, f"avgpool2x_bwd {hw} accumulated")


# ----------------------------------------------------------------------------- coverage
W_FAMILIES = {}
for _dt in ("f32", "bf16"):
    for _k in ("3,3,3", "1,3,3", "1,1,3", "3,2,2", "1,2,2", "1,1,2"):
        W_FAMILIES[f"k_wgrad {_dt} {_k}"] = lambda v, dt=_dt, k=_k: v.startswith(f"k_wgrad<{dt},{k},")
    W_FAMILIES[f"k_wgrad {_dt} MAXP=10"] = lambda v, dt=_dt: v.startswith(f"k_wgrad<{dt},") and "MAXP=10," in v
    W_FAMILIES[f"k_wgrad {_dt} MAXP=28"] = lambda v, dt=_dt: v.startswith(f"k_wgrad<{dt},") and "MAXP=28," in v
    W_FAMILIES[f"k_wgrad {_dt} PRE=1"] = lambda v, dt=_dt: v.startswith(f"k_wgrad<{dt},") and "PRE=1" in v
W_FAMILIES["k_wgrad f32 1,1,1"] = lambda v: v.startswith("k_wgrad<f32,1,1,1,")
W_FAMILIES["k_wgrad bf16 GEO=1"] = lambda v: v.startswith("k_wgrad<bf16,3,3,3,") and v.endswith(",GEO=1>")
W_FAMILIES["k_wgrad1 bf16"] = lambda v: v == "k_wgrad1<bf16>"
PHASE_W = {f"k_wgrad<{dt},{k},MAXP=10,PRE=0>" for dt in ("f32", "bf16") for k in ("3,2,2", "1,2,2", "1,1,2")}


def test_the_exact_backward_cases_cover_every_wgrad_family(ops):
    """The k_wgrad / k_wgrad1 names this module's weight-gradient launches dispatch (from rho_conv_wgrad_variant) hold one member of
    every family; the data-gradient launches (k_conv names) are covered by the forward module's table and only collected here."""
    want = set(EXPECT_W.values()) | PHASE_W
    seen_w = {v for v in _SEEN if v.startswith("k_wgrad")}
    assert seen_w <= want, sorted(seen_w - want)
    missing = [f for f, pred in W_FAMILIES.items() if not any(pred(v) for v in want)]
    assert not missing, missing
