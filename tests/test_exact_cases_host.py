"""CPU: the proof, runnable without a GPU, that the references of the integer-operand GPU tests (exact_cases.py) stay inside the
representability caps - every tensor a kernel stores or accumulates is an integer of at most 256 where it passes through bf16 and
below 2^24 where it stays in fp32 - and that torch's fp32 CPU evaluation of the same op equals the fp64 one exactly.  A case that
violated a cap would get sparser inputs, never a tolerance."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_cases as X
from exact_util import assert_bit_equal, check_bf16_exact, check_f32_exact, int_tensor, mismatch_report


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
