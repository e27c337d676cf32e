"""-m gpu: every attention kernel the dispatcher can launch, element by element against an fp64 reference.

The operands of tests/attn_cases.py give a softmax that is peaked but not one-hot (3 to 16 effective keys), whose running maximum
climbs from key tile to key tile in even heads (a rescale with 0 < alpha < 1 on tile after tile) and is found in the first tile in
odd heads (the rescale-skip branch afterwards), so l accumulated over tiles, P and dS rounded to bf16 at general values, delta,
dQ and dK all carry signal.  Every element of out, lse, dQ, dK and dV must lie within a bound derived from the kernels' rounding
points (attn_cases.bounds; tests/test_attn_cases_host.py shows on the CPU that a model of those rounding points stays inside the
bounds and that dropping a key, a key tile, a rescale, delta, or taking a neighbour's head or lse leaves them).

Cases (B, T, heads, ch), the smallest shapes that reach the edges, each in bf16 and fp32:
    (2, 161, 2, 16)   odd T: element-wise V^T fills; two query blocks (128 + 33), three key tiles
    (1, 333, 2, 32)   odd T, three query blocks
    (1, 328, 2, 64)   T % 8 == 0 but not % 64: vector and fast-tile paths with a ragged last tile; k_attn_dkv_fused
    (1, 130, 1, 64)   T % 4 == 2: the second query block holds two queries, three of its waves are clamped entirely
    (2, 49, 2, 128)   the ViT's token count: one ragged tile, batch and head offsets at odd T
    (1, 177, 2, 128)  odd T
    (1, 161, 1, 256), (1, 200, 2, 256)   ch = 256 over six / seven key tiles and two query blocks, scalar and vector fill
The backward is fed the REFERENCE's O (rounded to the dtype) and lse (fp32), so a failure there names a backward kernel; one
further case runs forward into backward end to end with the bounds widened by the forward's own.  Outputs are NaN-prefilled
between guard bands.  Each launch asserts the kernel names rho_attention_variant reports for it; the kernels behind
RHO_ATTN_F32_VALU / RHO_ATTN_DKV_SPLIT (latched by the library on first use) run in one child process; the last test asserts that
this process and the child together launched every kernel the dispatcher can name.  Every test prints its largest
error / bound ratio per output (the figures of an MI355X run are in DESIGN.md)."""
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):      # (run as a script by the switched-kernels test)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_cases as A  # noqa: E402
from attn_cases import BF16, F32  # noqa: E402
from exact_util import GUARD_VALUE, assert_within_abs, guarded, guards_intact  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DNAME = {BF16: "bf16", F32: "f32"}
# both switches on in this process?  (the parent runs without them, the child with both)
SW = all(os.environ.get(k, "0") not in ("", "0") for k in A.SWITCHES)
CASE_DT = [pytest.param(c, dt, id=f"{A.case_id(c)}-{DNAME[dt]}") for c in A.CASES for dt in (BF16, F32)]
STRIDE_CASES = [pytest.param((2, 49, 2, 128), BF16, id="bf16"), pytest.param((2, 161, 2, 16), F32, id="f32")]

SEEN = set()          # variant strings launched and checked in this process
RATIOS = {}           # "case-dtype-what" -> {output: largest error / bound}
_DONE = {}
_CHILD = {}


def _ops():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops as o
    hip.load()
    return o


def _expect(dtype, ch, backward):
    return A.EXPECT_ATTN[(SW, DNAME[dtype], ch, backward)]


def _inputs(case, dtype):
    pk = A.pack(A.operands(case, dtype), dtype)
    return {n: t.to(DEV) for n, t in pk.items()}


def _check(got, case, dtype, b, names, what, tag):
    """Every element of every output within its bound; prints and records the largest error / bound ratios."""
    r = A.reference(case, dtype)
    ra = A.ratios(got, case, dtype, b=b, names=names)
    RATIOS[tag] = ra
    print(f"{tag} [{what}]: error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in ra.items()))
    for n in names:
        axes = "[B, heads, T]" if n == "lse" else "[B, heads, T, ch]"
        assert_within_abs(got[n], r[n], b[n], f"{tag}: {n} {axes} of {what}")


def _forward(case, dtype):
    """out and lse of the forward kernel for this case, checked; cached."""
    key = ("fwd", case, dtype)
    if key in _DONE:
        return _DONE[key]
    ops = _ops()
    B, T, H, ch = case
    C = H * ch
    name = ops.attention_variant(dtype, ch)
    assert name == _expect(dtype, ch, False), (name, _expect(dtype, ch, False))
    x = _inputs(case, dtype)
    oflat, out = guarded((B, T, C), dtype)
    lflat, lse = guarded((B, H, T), F32)
    ops.attention(x["qk"], x["vt"], H, out=out, lse=lse)
    torch.cuda.synchronize()
    assert guards_intact(oflat) and guards_intact(lflat), f"{name}: a write outside out or lse"
    got = dict(out=A.from_cl(out.float(), H), lse=lse.cpu().double())
    # out: 2u sum p |v| (P rounded to bf16 before the PV product, one rounding of the output) + the fp32 term; fp32: that term alone.
    # lse: the logit error eps_t + 2 ulp32(lse).  (attn_cases.bounds derives the terms.)
    _check(got, case, dtype, A.bounds(case, dtype), ("out", "lse"), name, f"{A.case_id(case)}-{DNAME[dtype]}-fwd")
    SEEN.add(name)
    _DONE[key] = (out, lse)
    return _DONE[key]


def _split(dqkv, H):
    C = dqkv.shape[-1] // 3
    g = dqkv.float()
    return dict(dq=A.from_cl(g[..., :C], H), dk=A.from_cl(g[..., C:2 * C], H), dv=A.from_cl(g[..., 2 * C:], H))


def _backward(case, dtype):
    """dQ, dK, dV from the reference's O and lse (the engine's layout: one [B, T, 3C] buffer), checked; cached."""
    key = ("bwd", case, dtype)
    if key in _DONE:
        return
    ops = _ops()
    B, T, H, ch = case
    C = H * ch
    name = ops.attention_variant(dtype, ch, backward=True)
    assert name == _expect(dtype, ch, True), (name, _expect(dtype, ch, True))
    x, r = _inputs(case, dtype), A.reference(case, dtype)
    o_in = A.to_cl(r["o_in"]).to(dtype).contiguous().to(DEV)
    lse_in = r["lse_in"].contiguous().to(DEV)
    gflat, dqkv = guarded((B, T, 3 * C), dtype)
    ops.attention_bwd(x["qk"], x["vt"], o_in, x["do"], lse_in, H, dqkv=dqkv)
    torch.cuda.synchronize()
    assert guards_intact(gflat), f"{name}: a write outside dqkv"
    # dV: 2u sum_t p |dO|; dQ: u (2 sum_s |dS| |k| + ch^-0.5 D_t sum_s p |k|): dS rounded to bf16, the output rounded, delta from the
    # bf16 O; dK alike over queries; each + the fp32 term (alone for fp32).
    _check(_split(dqkv, H), case, dtype, A.bounds(case, dtype), ("dq", "dk", "dv"), name, f"{A.case_id(case)}-{DNAME[dtype]}-bwd")
    SEEN.add(name)
    _DONE[key] = True


@pytest.mark.parametrize("case,dtype", CASE_DT)
def test_forward_every_element(case, dtype):
    _forward(case, dtype)


@pytest.mark.parametrize("case,dtype", CASE_DT)
def test_backward_every_element_from_the_reference_forward(case, dtype):
    _backward(case, dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_forward_into_backward_end_to_end(dtype):
    """The backward fed with the forward KERNEL's out and lse.  Against the backward of the reference's forward its inputs differ
    by at most the forward's bounds b_out, b_lse: delta_t moves by at most w_t = sum_c |dO_tc| b_out[t, c], every p_ts by the
    relative g_t = 1.01 ln 2 b_lse[t]; dV gains sum_t g_t p_ts |dO_tc|, dS_ts moves by h_ts = g_t |dS_ts| + (1 + g_t) p_ts ch^-0.5 w_t,
    so dQ gains sum_s h_ts |k_sc| and dK sum_t h_ts |q_tc| (attn_cases.bounds, fwd_out_bound)."""
    case = A.E2E_CASE
    ops = _ops()
    B, T, H, ch = case
    C = H * ch
    out, lse = _forward(case, dtype)
    name = ops.attention_variant(dtype, ch, backward=True)
    assert name == _expect(dtype, ch, True)
    x = _inputs(case, dtype)
    gflat, dqkv = guarded((B, T, 3 * C), dtype)
    ops.attention_bwd(x["qk"], x["vt"], out, x["do"], lse, H, dqkv=dqkv)
    torch.cuda.synchronize()
    assert guards_intact(gflat)
    fb = A.bounds(case, dtype)
    b = A.bounds(case, dtype, fwd_out_bound=fb["out"], fwd_lse_bound=fb["lse"])
    for n in ("dq", "dk", "dv"):
        assert bool((b[n] >= fb[n]).all())
    _check(_split(dqkv, H), case, dtype, b, ("dq", "dk", "dv"), name, f"{A.case_id(case)}-{DNAME[dtype]}-e2e")


@pytest.mark.parametrize("padded", [False, True], ids=["default", "padded"])
@pytest.mark.parametrize("case,dtype", STRIDE_CASES)
def test_backward_row_strides(case, dtype, padded):
    """rho_attention_bwd itself: strides 0 (dense dqk [B, T, 2C] and a separate dv [B, T, C]) and padded rows (2C + 16, C + 8)
    whose gaps hold the guard value and must come back untouched."""
    from rho_diffusion_amd import hip
    ops = _ops()
    B, T, H, ch = case
    C = H * ch
    qs, vs = (2 * C + 16, C + 8) if padded else (2 * C, C)
    name = ops.attention_variant(dtype, ch, backward=True)
    assert name == _expect(dtype, ch, True), (name, _expect(dtype, ch, True))
    x, r = _inputs(case, dtype), A.reference(case, dtype)
    o_in = A.to_cl(r["o_in"]).to(dtype).contiguous().to(DEV)
    lse_in = r["lse_in"].contiguous().to(DEV)
    delta = torch.empty(B, H, T, dtype=F32, device=DEV)
    qflat, dqk = guarded((B, T, qs), dtype)
    vflat, dv = guarded((B, T, vs), dtype)
    dqk[..., 2 * C:] = GUARD_VALUE
    dv[..., C:] = GUARD_VALUE
    rc = hip.lib().rho_attention_bwd(x["qk"].data_ptr(), x["vt"].data_ptr(), o_in.data_ptr(), x["do"].data_ptr(), lse_in.data_ptr(),
                                     delta.data_ptr(), dqk.data_ptr(), qs if padded else 0, dv.data_ptr(), vs if padded else 0,
                                     hip.dtype_code(dtype), B, T, H, ch, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_intact(qflat) and guards_intact(vflat)
    assert bool((dqk[..., 2 * C:] == GUARD_VALUE).all()) and bool((dv[..., C:] == GUARD_VALUE).all()), "a write into the row gaps"
    got = dict(dq=A.from_cl(dqk[..., :C].float(), H), dk=A.from_cl(dqk[..., C:2 * C].float(), H), dv=A.from_cl(dv[..., :C].float(), H))
    _check(got, case, dtype, A.bounds(case, dtype), ("dq", "dk", "dv"), name,
           f"{A.case_id(case)}-{DNAME[dtype]}-strides-{'padded' if padded else 'default'}")


# ----------------------------------------------------------------------------- the kernels behind the switches
def _switched_work():
    """(case, dtype, forward?, backward?) whose kernels the two switches change (fp32 at ch = 256 backward is the VALU pair either
    way and runs again for the name)."""
    work = [(c, F32, True, True) for c in A.CASES]
    return work + [(c, BF16, False, True) for c in A.CASES if c[3] == 64]


def _child_main(path):
    assert SW, "the child runs with both switches set"
    for case, dtype, fwd, bwd in _switched_work():
        if fwd:
            _forward(case, dtype)
        if bwd:
            _backward(case, dtype)
    with open(path, "w") as f:
        json.dump(dict(names=sorted(SEEN), ratios=RATIOS), f)


def _child(tmp_path):
    """One child process with RHO_ATTN_F32_VALU=1 RHO_ATTN_DKV_SPLIT=1, started once per session: a failure is kept and raised
    again, never run again."""
    if "error" in _CHILD:
        raise AssertionError("the child process failed earlier in this session and is not started again:\n" + _CHILD["error"])
    if "result" not in _CHILD:
        path = str(tmp_path / "switched.json")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", path]
        try:
            r = subprocess.run(cmd, env=dict(os.environ, **A.SWITCHES), capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as exc:
            _CHILD["error"] = f"no exit within {exc.timeout} s"
            raise AssertionError(_CHILD["error"])
        print(r.stdout[-6000:])
        if r.returncode != 0:
            _CHILD["error"] = f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
            raise AssertionError(_CHILD["error"])
        with open(path) as f:
            _CHILD["result"] = json.load(f)
    return _CHILD["result"]


def test_switched_kernels_in_a_child_process(tmp_path):
    """k_attn_f32, the VALU backward pair at every head width and k_attn_dkv<64,64,*>: the same cases and assertions."""
    got = _child(tmp_path)
    want = {A.EXPECT_ATTN[(True, DNAME[dt], c[3], b)] for c, dt, fwd, bwd in _switched_work() for b in ([False] if fwd else []) + ([True] if bwd else [])}
    assert set(got["names"]) == want
    assert all(v <= 1.0 for ra in got["ratios"].values() for v in ra.values())
    ks = A.kernel_names(got["names"])
    assert {"k_attn_f32<16,64>", "k_attn_f32<256,16>", "k_attn_dq_f32<64,64>", "k_attn_dkv_f32<128,32>", "k_attn_dkv<64,64,0>",
            "k_attn_dkv<64,64,1>"} <= ks


def test_every_dispatched_kernel_was_launched_and_checked(tmp_path):
    """This process (whatever of it has not run yet runs now) plus the child: exactly the names the dispatcher can produce over
    ch in {16, 32, 64, 128, 256}, both dtypes, both settings of the switches."""
    assert not SW
    for p in CASE_DT:
        case, dtype = p.values
        _forward(case, dtype)
        _backward(case, dtype)
    seen = A.kernel_names(SEEN) | A.kernel_names(_child(tmp_path)["names"])
    every = A.kernel_names(A.EXPECT_ATTN.values())
    assert seen == every, (sorted(every - seen), sorted(seen - every))
    assert {c[3] for c in A.CASES} == {16, 32, 64, 128, 256}


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child"
    _child_main(sys.argv[2])
