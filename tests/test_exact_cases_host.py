"""CPU: the proof, runnable without a GPU, that the references of the integer-operand GPU tests (exact_cases.py) stay inside the
representability caps - every tensor a kernel stores or accumulates is an integer of at most 256 where it passes through bf16 and
below 2^24 where it stays in fp32 - and that torch's fp32 CPU evaluation of the same op equals the fp64 one exactly.  A case that
violated a cap would get sparser inputs, never a tolerance."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_cases as X
from exact_util import (assert_bit_equal, assert_within_abs, assert_within_ulps, check_bf16_exact, check_f32_exact, check_f32_grid, f32_ulp, int_tensor,
                        mismatch_report)


def _ids(cases):
    return [c["name"] for c in cases]


def test_int_tensor_is_integer_valued_and_deterministic():
    a, b = int_tensor((3, 5, 7), "t", 0.75, 2), int_tensor((3, 5, 7), "t", 0.75, 2)
    assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, a.round()) and float(a.abs().max()) <= 2
    x = int_tensor((100000,), "frac", 0.75, 2)
    w = int_tensor((100000,), "frac", 0.45, 1)
    assert 0.45 < float((x != 0).float().mean()) < 0.60 and 0.22 < float((w != 0).float().mean()) < 0.34


def test_assert_bit_equal_names_the_index_and_the_axes():
    want = torch.zeros(2, 4, 6)
    got = want.clone()
    assert_bit_equal(-got, want, "signed zero")                       # -0 == +0
    got[1, 2, 5] = 1.0
    got[1, 3, 5] = float("nan")
    with pytest.raises(AssertionError) as e:
        assert_bit_equal(got, want, "probe")
    msg = str(e.value)
    assert "2 of 48" in msg and "(1, 2, 5)" in msg and "axis 2 (extent 6): 1 indices with a mismatch: [5]" in msg
    assert "axis 1 (extent 4): 2 indices with a mismatch: [2, 3]" in msg
    assert mismatch_report(got.double(), want.double(), "x").count("\n") == 3


@pytest.mark.parametrize("c", X.FWD_CASES, ids=_ids(X.FWD_CASES))
def test_forward_case_reference_is_exactly_representable(c):
    o = X.fwd_operands(c, N=max(c["N"], 3) if c["ksplit"] else None)        # (k-split cases: the GPU test raises N; a few samples here)
    act, y = X.fwd_reference(c, o, torch.float64)
    act32, y32 = X.fwd_reference(c, o, torch.float32)
    assert_bit_equal(y32, y, c["name"] + ": fp32 vs fp64 on the CPU")
    assert_bit_equal(act32, act, c["name"] + ": activated input fp32 vs fp64")
    for k in ("x", "w", "sx", "sw", "res", "res2"):
        if k in o:
            check_bf16_exact(o[k], k)
    check_bf16_exact(act, "activated input")                            # the loader rounds a * x + b to the MFMA input type
    check_bf16_exact(y, "output")
    if c["res"] or c["res2"] or c["skip"]:                              # the addends join an exact fp32 accumulator: nothing else to cap
        check_f32_exact(y)
    if c["stats"]:
        assert float(y.abs().max()) <= X.STATS_Y_CAP, float(y.abs().max())
        kind = "conv32" if c["name"].startswith("c32") else "gemm" if c["name"].startswith("gemm") else "k_conv"
        st = X.stats_reference(y, X.tile_ids(c, kind))
        check_f32_exact(st, "fused statistics")
        assert_bit_equal(st.sum(1)[:, 0], y.double().sum((2, 3, 4)), "tile rows partition the sample")


@pytest.mark.parametrize("kernel,shape,up,cin,cout", X.PHASE_CASES, ids=["3x2x2", "1x2x2", "1x1x2"])
def test_phase_case_reference_is_exactly_representable(kernel, shape, up, cin, cout):
    o = X.phase_operands(kernel, shape, cin, cout)
    y = X.conv5(o["x"].double(), o["w"].double(), o["b"].double(), up=up)
    assert_bit_equal(X.conv5(o["x"], o["w"], o["b"], up=up), y, "fp32 vs fp64")
    check_bf16_exact(y, "output")
    # the phase weights are sums of up to four taps: integers of at most 4
    check_bf16_exact(o["w"].abs().sum((3, 4)) if up[0] else o["w"].abs().sum(4), "phase weights")
    dy = int_tensor(tuple(y.shape), "ph_dy", 0.45, 1).double()
    xr = o["x"].double().requires_grad_(True)
    wr = o["w"].double().requires_grad_(True)
    X.conv5(xr, wr, None, up=up).backward(dy)
    check_bf16_exact(xr.grad, "dX")
    check_f32_exact(wr.grad, "dW")
    # the phase data gradients accumulate in place through the stored dX: every running sum over the parities of dY is capped too
    acc = torch.zeros_like(xr.grad)
    for a in ((0, 1) if up[0] else (None,)):
        for c in ((0, 1) if up[1] else (None,)):
            part = torch.zeros_like(dy)
            sl = (Ellipsis, slice(None) if a is None else slice(a, None, 2), slice(None) if c is None else slice(c, None, 2))
            part[sl] = dy[sl]
            xp = o["x"].double().requires_grad_(True)
            X.conv5(xp, o["w"].double(), None, up=up).backward(part)
            acc = acc + xp.grad
            check_bf16_exact(acc, "running sum of the phase data gradients")
    assert_bit_equal(acc, xr.grad, "the parities of dY add up to dX")


@pytest.mark.parametrize("shape,cin,cout", X.S2_CASES, ids=["32to64"])
def test_parity_split_partial_sums_are_exactly_representable(shape, cin, cout):
    o = X.phase_operands((3, 3, 3), shape, cin, cout, tag="s2")
    y = X.conv5(o["x"].double(), o["w"].double(), o["b"].double(), stride=(2, 2))
    assert_bit_equal(X.conv5(o["x"], o["w"], o["b"], stride=(2, 2)), y, "fp32 vs fp64")
    acc = o["b"].double().reshape(1, -1, 1, 1, 1)
    for wpart in X.s2_partial_weights(o["w"].double()):                  # each launch stores the running sum in the engine dtype
        acc = acc + X.conv5(o["x"].double(), wpart, None, stride=(2, 2))
        check_bf16_exact(acc, "partial sum of the parity launches")
    assert_bit_equal(acc, y, "the four tap selections add up to the conv")
    dy = int_tensor(tuple(y.shape), "s2_dy", 0.45, 1).double()
    xr = o["x"].double().requires_grad_(True)
    X.conv5(xr, o["w"].double(), None, stride=(2, 2)).backward(dy)
    check_bf16_exact(xr.grad, "dX")


@pytest.mark.parametrize("c", X.BWD_CASES, ids=_ids(X.BWD_CASES))
def test_backward_case_reference_is_exactly_representable(c):
    o = X.bwd_operands(c)
    r = X.bwd_reference(c, o, torch.float64)
    r32 = X.bwd_reference(c, o, torch.float32)
    for k in ("dx", "dw", "db"):
        assert_bit_equal(r32[k], r[k], f"{c['name']} {k}: fp32 vs fp64 on the CPU")
    check_bf16_exact(r["act"], "activated input")
    check_bf16_exact(r["dx"], "dX")                                      # stored in the engine dtype
    check_f32_exact(r["dw"], "dW")                                       # fp32 buffer
    check_f32_exact(r["db"], "dbias")
    check_f32_exact(2 * r["dw"], "dW accumulated onto itself")
    if "base" in o:
        check_bf16_exact(r["dx"][:, c["c1"]:] + o["base"].double(), "second gradient accumulated onto its base")
    if any(c["up"]):
        # the upsample form: gradient w.r.t. the upsampled input (stored), then its 2x2 / 1x2 sum
        up = r["act"].clone()
        for ax, f in ((3, c["up"][0]), (4, c["up"][1])):
            up = up.repeat_interleave(2, dim=ax) if f else up
        up.requires_grad_(True)
        X.conv5(up, o["w"].double(), None).backward(o["dy"].double())
        check_bf16_exact(up.grad, "gradient w.r.t. the upsampled input")
        pooled = F.avg_pool3d(up.grad, (1, 2 if c["up"][0] else 1, 2 if c["up"][1] else 1)) * (2 ** sum(c["up"]))
        assert_bit_equal(pooled, r["dx"], "pool2x sum of it")


@pytest.mark.parametrize("B,T,heads,ch", X.ATTN_CASES)
def test_attention_case_is_one_hot(B, T, heads, ch):
    o = X.attn_operands(B, T, heads, ch)
    r = X.attn_reference(o, ch)
    assert float(r["gap"].min()) >= X.ATTN_MIN_GAP, float(r["gap"].min())
    assert 2.0 ** -X.ATTN_MIN_GAP < 2.0 ** -149                          # below the smallest fp32 subnormal
    for k in ("q", "k", "v", "do"):
        assert torch.equal(o[k], o[k].to(torch.bfloat16).float()), k     # exact in bf16
    assert float(o["v"].abs().max()) <= 127 and float(o["do"].abs().max()) <= 2
    for b in range(B):
        for h in range(heads):
            assert sorted(o["pi"][b, h].tolist()) == list(range(T))
    if B * heads > 1:
        assert len({tuple(o["pi"][b, h].tolist()) for b in range(B) for h in range(heads)}) == B * heads
    codes = X.attn_codes(T, ch)
    assert len({tuple(r_) for r_ in codes.tolist()}) == T
    # exact softmax of these logits in fp64 is one-hot to far below fp32 resolution
    p = torch.softmax(r["logits"] * math.log(2.0), -1)
    assert float((p.max(-1).values - 1).abs().max()) < 1e-40
    # raw logits and dP = dO . V are exact integers in fp32
    check_f32_exact(torch.einsum("bhct,bhcs->bhts", o["q"].double(), o["k"].double()), "raw logits")
    check_f32_exact(torch.einsum("bhct,bhcs->bhts", o["do"].double(), o["v"].double()), "dP")


# ----------------------------------------------------------------------------- GroupNorm passes
def test_assert_within_ulps_is_per_element_and_names_the_index():
    want = torch.tensor([[1.0, 3.0, 0.0], [2.0 ** -130, -1024.0, 0.75]], dtype=torch.float64)
    assert f32_ulp(want).tolist() == [[2.0 ** -23, 2.0 ** -22, 2.0 ** -149], [2.0 ** -149, 2.0 ** -13, 2.0 ** -24]]
    got = want.float()
    assert assert_within_ulps(got, want, 0, "equal") == 0.0
    got[1, 1] = torch.nextafter(got[1, 1], torch.tensor(-2048.0))
    assert assert_within_ulps(got, want, 1, "one ulp") == 1.0
    with pytest.raises(AssertionError) as e:
        assert_within_ulps(got, want, 0.5, "probe")
    msg = str(e.value)
    assert "1 of 6" in msg and "(1, 1)" in msg and "axis 1 (extent 3): 1 indices with a mismatch: [1]" in msg and msg.count("\n") == 2
    got[0, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"1 of 6 .*first at \(0, 2\): got nan"):
        assert_within_ulps(got, want, 1, "NaN never passes")
    # a magnitude other than want's: 1e-3 off is far inside one ulp of 2^20, far outside one ulp of 1
    assert_within_ulps(torch.tensor([1.001]), torch.tensor([1.0], dtype=torch.float64), 1, "mag", mag=torch.tensor([2.0 ** 20]))


def test_assert_within_abs_is_per_element_and_names_the_index():
    want = torch.zeros(2, 3, 4, dtype=torch.float64)
    got = want.float()
    got[1, 2, 3] = 0.25
    assert assert_within_abs(got, want, 0.25, "scalar bound") == 0.25
    bound = torch.full_like(want, 0.1)
    bound[1, 2, 3] = 0.5
    assert assert_within_abs(got, want, bound, "a bound per element") == 0.25
    got[0, 1, 3] = 0.2
    got[0, 0, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        assert_within_abs(got, want, bound, "probe")
    msg = str(e.value)
    assert "probe: 2 of 24 elements are outside their bound; first at (0, 0, 0): got nan" in msg and msg.count("\n") == 3
    assert "axis 1 (extent 3): 2 indices with a mismatch: [0, 1]" in msg and "axis 2 (extent 4): 2 indices with a mismatch: [0, 3]" in msg
    with pytest.raises(AssertionError, match="shape"):
        assert_within_abs(got[0], want, 1.0, "shape")


def _gn_dropped(g, tag):
    """g under a stand-in keep mask at p = 0.5 (inv_keep = 2): the GPU tests use the mask the kernels draw and repeat these checks."""
    return g * 2.0 * X.gn_int(tuple(g.shape), tag, 0, 1)


@pytest.mark.parametrize("c", X.GN_CASES, ids=_ids(X.GN_CASES))
def test_groupnorm_case_references_are_exactly_representable(c):
    N, S, C, cpg = c["N"], c["S"], c["C"], c["cpg"]
    assert C % 32 == 0 and c["c1"] % 8 == 0 and c["c2"] % 8 == 0 and C <= 2048
    # statistics: integer x of at most 7, channel sums and sums of squares (and every partial sum of them) below 2^24
    o = X.gn_stats_operands(c)
    check_bf16_exact(o["x"], "x")
    assert float(o["x"].abs().max()) <= 7
    r, r32 = X.gn_stats_reference(o["x"]), X.gn_stats_reference(o["x"], torch.float32)
    for k in ("sum", "sumsq"):
        check_f32_exact(r[k], k)
        assert_bit_equal(r32[k], r[k], f"{c['name']} {k}: fp32 vs fp64 on the CPU")
    check_f32_exact(o["x"].abs().double().sum(1), "sum of |x| (bounds every partial sum)")
    # apply: a x + b
    o = X.gn_apply_operands(c)
    y = X.gn_apply_reference(o["x"], o["a"], o["b"])
    assert_bit_equal(X.gn_apply_reference(o["x"], o["a"], o["b"], torch.float32), y, "apply: fp32 vs fp64")
    check_bf16_exact(y, "a x + b")
    check_bf16_exact(2 * y, "dropout(a x + b) at p = 0.5")
    # backward: reduce -> finalize -> apply, plain and under a p = 0.5 mask
    o = X.gn_bwd_operands(c)
    for k in ("g", "x", "mean", "gamma", "beta", "film", "a", "b", "cA", "cP", "cQ", "dx0", "add1", "dgamma0", "dbeta0"):
        check_bf16_exact(o[k], k)
    assert set(o["rstd"].unique().tolist()) <= {0.5, 1.0, 2.0}
    scale = o["film"][:, :C]
    for drop in (False, True):
        gq = _gn_dropped(o["g"], "hostmask" + c["name"]) if drop else o["g"]
        r = X.gn_bwd_reference(gq, o["x"], o["mean"], o["rstd"], o["gamma"], o["beta"], scale)
        r32 = X.gn_bwd_reference(gq, o["x"], o["mean"], o["rstd"], o["gamma"], o["beta"], scale, torch.float32)
        check_f32_exact(r["R1"], "R1")
        check_f32_grid(r["absR2"], 0.5, "sum of |gq xhat| (bounds every partial sum of R2)")
        for k in ("R2", "dgamma_n", "dbeta_n", "dgamma", "dbeta", "dscale", "dshift", "cA"):
            check_f32_grid(r[k], 0.5, k)
            assert_bit_equal(r32[k], r[k], f"{c['name']} {k}: fp32 vs fp64 on the CPU")
        check_f32_grid(r["dgamma_n"].abs().sum(0) + o["dgamma0"].abs().double(), 0.5, "running sums of dgamma over the samples")
        check_f32_grid(r["dbeta_n"].abs().sum(0) + o["dbeta0"].abs().double(), 0.5, "running sums of dbeta over the samples")
        if X.is_pow2(cpg * S):                                      # the division by M = cpg S is exact: cP, cQ fit fp32
            for k in ("cP", "cQ"):
                assert_bit_equal(r[k].float(), r[k], f"{c['name']} {k}: representable in fp32")
                assert_bit_equal(r32[k], r[k], f"{c['name']} {k}: fp32 vs fp64 on the CPU")
        # apply: cA gq + cP + cQ x on top of a running gradient and a residual addend
        t = X.gn_bwd_apply_reference(gq, o["x"], o["cA"], o["cP"], o["cQ"])
        assert_bit_equal(X.gn_bwd_apply_reference(gq, o["x"], o["cA"], o["cP"], o["cQ"], torch.float32), t, "bwd apply: fp32 vs fp64")
        full = t + o["dx0"].double()
        full[..., :c["c1"]] += o["add1"].double()
        check_bf16_exact(t, "apply term")
        check_bf16_exact(o["dx0"][..., :c["c1"]] + o["add1"], "running gradient + residual addend (rounded to the storage type first)")
        check_bf16_exact(full, "apply term + running gradient + residual addend")


@pytest.mark.parametrize("N,c1,c2,nb1,nb2", X.GN_FIN2_CASES)
def test_finalize2_synthetic_partials_are_exact(N, c1, c2, nb1, nb2):
    o = X.gn_fin2_operands(N, c1, c2, nb1, nb2)
    assert c1 % 8 == 0 and c2 % 8 == 0 and (c1 + c2) % 32 == 0 and c1 + c2 <= 2048
    for key in ("0", "1", "2"):
        check_f32_exact(o["s" + key].abs().double().sum(1), "channel sums")
        check_f32_exact(o["q" + key].double().sum(1), "channel sums of squares")
        assert torch.equal(X.partials_fmt0(o["s" + key], o["q" + key])[..., :8].reshape(o["s" + key].shape), o["s" + key])
        assert torch.equal(X.partials_fmt1(o["s" + key], o["q" + key])[:, :, 1], o["q" + key])
    s = torch.cat([o["s1"].sum(1), o["s2"].sum(1)], 1)
    q = torch.cat([o["q1"].sum(1), o["q2"].sum(1)], 1)
    mean, rstd = X.gn_moments_reference(s, q, o["S"])
    assert bool((rstd < 100.0).all()) and bool((rstd > 0.1).all())     # a positive variance: nothing rests on the clamp at 0


@pytest.mark.parametrize("N,C,nb", X.GN_FIN1_CASES)
def test_bwd_finalize_synthetic_tile_sums_are_exact(N, C, nb):
    o = X.gn_fin1_operands(N, C, nb)
    mu, rs = X.per_channel(o["mean"], C // 32).double(), X.per_channel(o["rstd"], C // 32).double()
    r2 = rs * (o["dzx"].double() - mu * o["dz"].double())                # per tile: what fmt 0 holds in its second row
    check_f32_grid(r2.abs().sum(1), 0.5, "R2 per channel")
    check_f32_exact(o["dz"].abs().double().sum(1), "R1 per channel")
    assert_bit_equal(r2.float(), r2, "per-tile R2 in fp32")
    sc = 1.0 + o["film"][:, :C].double()
    for v, k in ((r2.sum(1) * sc, "dgamma_n"), (o["dz"].double().sum(1) * sc, "dbeta_n")):
        check_f32_grid(v.abs().sum(0), 0.5, k + " summed over the samples")
    check_f32_grid(o["gamma"].double() * r2.sum(1) + o["beta"].double() * o["dz"].double().sum(1), 0.5, "dscale")


@pytest.mark.parametrize("c", X.GNB_CASES, ids=_ids(X.GNB_CASES))
def test_gnb_case_references_are_exactly_representable(c):
    o = X.gnb_operands(c)
    r, r32 = X.bwd_reference(c, o), X.bwd_reference(c, o, torch.float32)
    assert_bit_equal(r32["dx"], r["dx"], "dX: fp32 vs fp64")
    check_bf16_exact(r["dx"], "dX")
    check_bf16_exact(o["x0"], "x0")
    C = c["c1"] + c["c2"]
    assert c["c1"] % 32 == 0 and c["c2"] % 32 == 0
    st = X.stats_reference(r["dx"], X.tile_ids(c, "k_conv"), o["x0"])
    check_f32_exact(st, "per-tile sum dz, sum dz x0")
    check_f32_exact(X.stats_reference(r["dx"].abs(), X.tile_ids(c, "k_conv"), o["x0"].abs()), "per-tile sums of magnitudes")
    assert_bit_equal(st.sum(1)[:, 1], (r["dx"] * o["x0"].double()).sum((2, 3, 4)), "tile rows partition the sample")
    dz, x0 = X.to_nsc(r["dx"]), X.to_nsc(o["x0"])
    scale = o["film"][:, :C]
    q = X.gn_bwd_reference(dz, x0, o["mean"], o["rstd"], o["gamma"], o["beta"], scale)
    q32 = X.gn_bwd_reference(dz, x0, o["mean"], o["rstd"], o["gamma"], o["beta"], scale, torch.float32)
    check_f32_grid(q["absR2"], 0.5, "sum of |dz xhat|")
    for k in ("R1", "R2", "dgamma", "dbeta", "dscale", "dshift", "cA"):
        check_f32_grid(q[k], 0.5, k)
        assert_bit_equal(q32[k], q[k], f"{k}: fp32 vs fp64")
    if X.is_pow2((C // 32) * o["S"]):
        for k in ("cP", "cQ"):
            assert_bit_equal(q[k].float(), q[k], f"{k}: representable in fp32")


@pytest.mark.parametrize("case", X.GNA_CASES, ids=[c[0] for c in X.GNA_CASES])
def test_gna_case_reference_is_exactly_representable(case):
    o = X.gna_operands(case)
    for k in ("dy", "w", "g", "x0", "cA", "cP", "cQ"):
        check_bf16_exact(o[k], k)
    y = X.gna_reference(o)
    assert_bit_equal(X.gna_reference(o, torch.float32), y, "fp32 vs fp64")
    check_bf16_exact(y, "conv + cA g + cQ x0 + cP")
    assert case[3] % 32 == 0 and case[4] % 32 == 0


# ----------------------------------------------------------------------------- the streams of k_gn_bwd_reduce
def test_reduce_stream_twin_reaches_every_accumulation():
    """The position -> accumulation map the sparse test relies on (exact_cases.gn_reduce_stream), by hand for the three shapes:
    nblk2_tails: ppi = 32, blocks of 129 and 128 positions: lane 0 of block 0 has 5 positions, the fifth (128) is unpaired;
    cpg3_straddle: S = 7 < ppi = 21, every lane has one position; c2048: ppi = 1, nine positions: four pairs and the ninth alone."""
    assert X.gn_reduce_stream_positions(257, 64) == {"gq": 0, "gr": 32, "tail": 128}
    assert X.gn_reduce_stream_positions(7, 96) == {"tail": 0}
    assert X.gn_reduce_stream_positions(9, 2048) == {"gq": 0, "gr": 1, "tail": 8}
    assert X.gn_reduce_stream(257, 64, 129 + 96) == "gr" and X.gn_reduce_stream(257, 64, 129 + 64) == "gq"      # second block: four per lane


# ----------------------------------------------------------------------------- SiLU in the conv loaders
import embed_cases as EC  # noqa: E402
from exact_util import TIE_MARGIN_FACTOR, bf16_round, tie_share  # noqa: E402
from exact_cases import BF16, F32  # noqa: E402

_silu_ids = lambda c: c["name"]  # noqa: E731


def test_silu_operand_is_uniquely_determined_on_the_integer_set():
    """For every u the SiLU cases use, silu64(u) is farther from the nearest bf16 rounding tie than TIE_MARGIN_FACTOR times the
    derived silu_f bound (embed_cases.silu_f_ulps: at most 7.6 ulps on [-2, 6]): every fp32 value inside the bound rounds to
    bf16(silu64(u)), so the share of loader operands with a choice is 0: the nearest tie is at least 742 fp32 ulps away."""
    u = torch.tensor(X.SILU_U, dtype=torch.float64)
    s = u / (1.0 + torch.exp(-u))
    want, bound, mag = EC.hw_act_bound(u, 1, False)
    assert float((want - s).abs().max()) < 1e-15
    assert tie_share(s[u != 0], TIE_MARGIN_FACTOR * bound[u != 0]) == 0.0            # (u = 0: x * rcp(2) is an exact zero)
    nz = u != 0
    ulp16 = f32_ulp(s[nz]) * 65536
    lo = torch.floor(s[nz].abs() / ulp16) * ulp16
    dist = ((s[nz].abs() - lo - 0.5 * ulp16).abs() / f32_ulp(s[nz]))
    assert float(dist.min()) >= 742, dist.tolist()
    assert float((TIE_MARGIN_FACTOR * EC.silu_f_ulps(u, False)).max()) < 40 < float(dist.min())
    check_f32_grid(bf16_round(s), X.SILU_GRID, "bf16(silu64(u))")


@pytest.mark.parametrize("c", X.SILU_FWD_CASES, ids=_silu_ids)
def test_silu_forward_cases_are_exact_after_one_rounding(c):
    o = X.silu_fwd_operands(c)
    u = X.affine(o["x"].double(), o["pa"].double(), o["pb"].double())
    assert set(u.unique().tolist()) <= set(float(v) for v in X.SILU_U), "u = a x + b must stay on the proven integer set"
    assert set(o["pa"].unique().tolist()) == {-1.0, 1.0, 2.0}, "a differs per (sample, channel), so the coefficient rows matter"
    assert torch.equal(X.affine(o["x"], o["pa"], o["pb"]).double(), u)
    if BF16 in c["dtypes"]:
        _, y = X.silu_fwd_reference(c, o, BF16)
        check_f32_grid(X.silu_fwd_magnitude(c, o, BF16), X.SILU_GRID, "sum |w s| + |bias| + |res| + |add|")
        check_f32_grid(y, X.SILU_GRID, "y")
        # the mutated loaders hand the MFMA another operand for some u of this case, and the output moves
        for form in X.SILU_FORMS[1:]:
            uu = u.unique()
            assert not torch.equal(X.silu_operand(uu, BF16, form), X.silu_operand(uu, BF16)), f"{c['name']}: {form} gives the same operands"
            _, ym = X.silu_fwd_reference(c, o, BF16, form)
            assert not torch.equal(bf16_round(ym), bf16_round(y)), f"{c['name']}: a loader computing SiLU as {form} would pass"
    if F32 in c["dtypes"]:
        b = X.silu_fwd_bound(c, o)
        _, y = X.silu_fwd_reference(c, o, F32)
        assert float((b / (X.silu_fwd_magnitude(c, o, F32) + 1e-30)).max()) < 1e-3, "the float32 bound must stay a per-element one"


def test_silu_float32_bound_notices_a_wrong_silu():
    """The float32 bound carries n 2^-24 sum |w s| for the accumulation, which at K = 96 * 27 terms is wider than the damage of a
    bf16-rounded exponential; the short-K cases (1x1x1, 1-D) are the ones that must notice, and are named."""
    for form in X.SILU_FORMS[1:]:
        bad = []
        for c in X.SILU_FWD_CASES:
            if F32 in c["dtypes"]:
                o = X.silu_fwd_operands(c)
                _, y = X.silu_fwd_reference(c, o, F32)
                _, ym = X.silu_fwd_reference(c, o, F32, form)
                if bool(((ym - y).abs() > X.silu_fwd_bound(c, o)).any()):
                    bad.append(c["name"])
        assert {"3d_1x1", "1d_1x1", "1d_basic"} <= set(bad), f"float32 SiLU as {form}: noticed by {bad}"


@pytest.mark.parametrize("c", X.SILU_BWD_CASES, ids=_silu_ids)
def test_silu_wgrad_cases_are_exact_on_the_grid(c):
    o = X.silu_bwd_operands(c)
    u = X.affine(o["x"].double(), o["pa"].double(), o["pb"].double())
    assert set(u.unique().tolist()) <= set(float(v) for v in X.SILU_U)
    assert float(o["dy"].abs().max()) == 1.0
    for dt in c["dtypes"]:
        dw, mag, bound = X.silu_wgrad_reference(c, o, dt)
        for form in X.SILU_FORMS[1:]:
            dwm, _, _ = X.silu_wgrad_reference(c, o, dt, form)
            if dt == BF16:
                assert not torch.equal(dwm, dw), f"{c['name']}: a wgrad loader computing SiLU as {form} would pass"
            else:
                assert bool(((dwm - dw).abs() > bound).any()), f"{c['name']}: a float32 wgrad loader computing SiLU as {form} would pass"
        if dt == BF16:
            check_f32_grid(mag, X.SILU_GRID, "sum |dY s|")
            check_f32_grid(dw, X.SILU_GRID, "dW")


@pytest.mark.parametrize("c", X.GNB_CASES, ids=_silu_ids)
def test_gnb_silu_rows_keep_a_per_element_bound(c):
    """The per-tile rows of a data-gradient launch with gnb_silu = 1 on integer u in [-10, 10]: the bound stays far below one term
    (so one wrong, missing or doubled position fails), and a launch that left dsilu out of the rows is outside it."""
    o = X.gnb_silu_operands(c)
    u = X.affine(o["x0"].double(), o["a"].double(), o["b"].double())
    assert float(u.abs().max()) <= 12 and torch.equal(u, u.round())
    ids = X.tile_ids(c, "k_conv")
    z, rows, rb = X.gnb_silu_reference(c, o, ids)
    check_bf16_exact(z, "the integer data gradient")
    mags = X.stats_reference(z.abs(), ids, o["x0"].abs())
    assert float((rb / mags.clamp_min(1.0)).max()) < 1e-3, "a missing position worth a thousandth of its row's magnitude sum must fail"
    plain = X.stats_reference(z, ids, o["x0"])
    assert bool(((plain - rows).abs() > rb).any()), c["name"] + ": rows without dsilu would pass"


@pytest.mark.parametrize("case", X.GNA_CASES, ids=[c[0] for c in X.GNA_CASES])
def test_gna_silu_cases_leave_at_most_one_percent_near_a_tie(case):
    """The skip data gradient with gna_* and gnb_silu = 1: u on the integers of [-10, 10], the conv part an exact integer, the
    coefficients the identity, and (bf16) at most 1 % of the stored outputs within the tie margin of four times the float32 bound."""
    from exact_util import TIE_SHARE_MAX
    o = X.gna_silu_operands(case)
    u, conv, want, fb = X.gna_silu_reference(o)
    assert float(u.abs().max()) <= 12 and torch.equal(u, u.round())
    check_bf16_exact(conv, "the integer conv part")
    assert set(o["g"].unique().tolist()) == {-0.5, -0.25, 0.0, 0.25, 0.5} and bool((o["cA"] == 1).all())
    d = (want - conv).abs()                                      # |g dsilu(u)| <= |g| Mag(u)
    assert float((fb / (conv.abs() + d).clamp_min(2.0 ** -20)).max()) < 2e-5, "the bound is a few dozen fp32 ulps of the terms"
    # leaving dsilu out (gq = g) is far outside the bound
    nz = o["g"] != 0
    assert float((((conv + o["g"].double()) - want).abs()[nz] / fb[nz]).max()) > 1000
    if case[1] == BF16:
        share = tie_share(want, TIE_MARGIN_FACTOR * fb)
        assert share <= TIE_SHARE_MAX, f"{case[0]}: {share:.3%} of the outputs within the tie margin"
