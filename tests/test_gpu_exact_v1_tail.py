"""-m gpu: the legacy-UNet tail of csrc/unet_v1.hip - rho_groupnorm_act / _bwd, rho_act_add, rho_act_bwd - element by element.

tests/v1_cases.py holds the group shapes (cpg = 1, 3, 12, 32, 260; S = 1; more than 16384 elements per group, where the fp32 run
carry of k_gn_groups_fwd executes; cpg > 256, where the `j += 256` loops of the backward take a second pass), the operands and the
fp64 references; tests/test_ln_cases_host.py proves their representability on the CPU.
  forward: integer x with integer group means: mean bit-equal, rstd equal to the fp64 reference rounded to fp32 (V1_RSTD_ULPS),
    y at act 0 within V1_Y_ULPS (bf16: the tie rule of exact_util.py);
  backward: stats supplied (integer mean, rstd in {0.5, 1, 2}), act 0: dgamma / dbeta bit-equal on top of a nonzero prefill (the
    kernel accumulates with float atomics: exact in any order on these operands); dx bit-equal where S * cpg is a power of two, else
    within V1_DX_ULPS;
  activation codes 1 - 3 per element on embed_cases.code_inputs() through every kernel, against act64 / dact64 with the ACT_ULPS
    allowances (act_f / dact_f are the libm expressions those were measured for); bf16 stores add half a bf16 ulp;
  the addends of rho_act_add, r and nc present and absent, on integers: bit-equal, which pins nc[(i / (s c)) c + i % c].
Every output lies between guard bands and starts as NaN unless the launch accumulates onto it."""
import pytest
import torch

import embed_cases as EC
import v1_cases as V1
from embed_cases import ACT_ULPS
from exact_util import (assert_bf16_tie_rule, assert_bit_equal, assert_within_abs, assert_within_ulps, bf16_store_bound, f32_ulp, guarded,
                        guarded_copy, guards_intact, tie_margin)
from ln_cases import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
_ids = lambda c: c["name"]  # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


def dev(t, dtype=F32):
    return None if t is None else t.to(DEV).to(dtype).contiguous()


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _gn_fwd(hip, x, gamma, beta, dtype, N, S, C, groups, act):
    (fy, y), (fs, st) = guarded((N, S, C), dtype), guarded((N, groups, 2), F32)
    hip.check(hip.lib().rho_groupnorm_act(x.data_ptr(), y.data_ptr(), st.data_ptr(), gamma.data_ptr(), beta.data_ptr(), hip.dtype_code(dtype),
                                          N, S, C, groups, V1.V1_EPS, act, hip.stream()), "rho_groupnorm_act")
    torch.cuda.synchronize()
    assert guards_intact(fy) and guards_intact(fs), "store outside y / stats"
    return y, st


def _gn_bwd(hip, x, dy, stats, gamma, beta, pre_dg, pre_db, dtype, N, S, C, groups, act):
    (fd, dx), (fg, dg), (fb, db) = guarded((N, S, C), dtype), guarded_copy(pre_dg, F32), guarded_copy(pre_db, F32)
    hip.check(hip.lib().rho_groupnorm_act_bwd(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dx.data_ptr(),
                                              dg.data_ptr(), db.data_ptr(), hip.dtype_code(dtype), N, S, C, groups, act, hip.stream()),
              "rho_groupnorm_act_bwd")
    torch.cuda.synchronize()
    assert guards_intact(fd) and guards_intact(fg) and guards_intact(fb), "store outside dx / dgamma / dbeta"
    return dx, dg, db


# ----------------------------------------------------------------------------- rho_groupnorm_act, act 0
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", V1.V1_CASES, ids=_ids)
def test_groupnorm_forward_statistics_and_output(hip, c, dtype):
    o = V1.v1_fwd_operands(c)
    r = V1.v1_fwd_reference(c, o)
    what = f"{c['name']} {_dn(dtype)}"
    y, st = _gn_fwd(hip, dev(o["x"], dtype), dev(o["gamma"]), dev(o["beta"]), dtype, c["N"], c["S"], c["C"], c["groups"], 0)
    assert_bit_equal(st[..., 0], r["mean"], what + ": stats[..., 0] = mean [N, groups]")
    w_r = assert_within_ulps(st[..., 1], r["rstd"].float().double(), V1.V1_RSTD_ULPS, what + ": stats[..., 1] = rstd [N, groups]")
    if dtype == F32:
        w_y = assert_within_ulps(y, r["y"], V1.V1_Y_ULPS, what + ": y [N, S, C] (ulps of |xhat gamma| + |beta|)", mag=r["y_mag"])
        print(f"measured: v1 gn fwd {what}: rstd worst {w_r:.3f} ulp (derived {V1.V1_RSTD_ULPS}), y worst {w_y:.3f} ulp (derived {V1.V1_Y_ULPS})")
    else:
        share = assert_bf16_tie_rule(y, r["y"], tie_margin(V1.V1_Y_ULPS, r["y_mag"]), what + ": y [N, S, C]")
        print(f"measured: v1 gn fwd {what}: rstd worst {w_r:.3f} ulp (derived {V1.V1_RSTD_ULPS}), y bf16 by the tie rule, {share:.4%} near a tie")


# ----------------------------------------------------------------------------- rho_groupnorm_act_bwd, act 0
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", V1.V1_CASES, ids=_ids)
def test_groupnorm_backward_supplied_statistics(hip, c, dtype):
    o = V1.v1_bwd_operands(c)
    r = V1.v1_bwd_reference(c, o)
    what = f"{c['name']} {_dn(dtype)}"
    stats = dev(torch.stack([o["mean"], o["rstd"]], 2))
    dx, dg, db = _gn_bwd(hip, dev(o["x"], dtype), dev(o["dy"], dtype), stats, dev(o["gamma"]), dev(o["beta"]), o["pre_dgamma"], o["pre_dbeta"],
                         dtype, c["N"], c["S"], c["C"], c["groups"], 0)
    assert_bit_equal(dg, r["dgamma"], what + ": dgamma [C] on top of its prefill")
    assert_bit_equal(db, r["dbeta"], what + ": dbeta [C] on top of its prefill")
    if V1.dx_is_exact(c):
        assert_bit_equal(dx, r["dx"].float().to(dtype), what + ": dx [N, S, C]")        # exact in fp32; bf16 rounds it once
    elif dtype == F32:
        worst = assert_within_ulps(dx, r["dx"], V1.V1_DX_ULPS, what + ": dx [N, S, C] (ulps of rstd (|g| + |m1| + |xhat m2|))", mag=r["dx_mag"])
        print(f"measured: v1 gn bwd {what}: dx worst {worst:.3f} ulp (derived {V1.V1_DX_ULPS})")
    else:
        assert_within_abs(dx, r["dx"], bf16_store_bound(r["dx"], V1.V1_DX_ULPS * f32_ulp(r["dx_mag"])), what + ": dx (fp32 bound + half a bf16 ulp)")


# ----------------------------------------------------------------------------- activation codes 1 - 3, per element
def _act_ulps(code, deriv):
    return 0.0 if code in EC.INT_ACTS else float(ACT_ULPS[code][int(deriv)])


def _judge(got, want, bound, mag, dtype, what):
    meas = float(((got.detach().cpu().double() - want).abs() / f32_ulp(mag)).max())
    if dtype == F32:
        print(f"measured: {what}: worst {meas:.3f} ulp of the term magnitude")
        assert_within_abs(got, want, bound, what)
    else:
        assert_within_abs(got, want, bf16_store_bound(want, bound), what + " (fp32 bound + half a bf16 ulp)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("code", [1, 2, 3])
def test_activation_codes_act_add_and_act_bwd(hip, code, dtype):
    """rho_act_add without addends is act(x); rho_act_bwd with dout = 1 is act'(x)."""
    x = EC.code_inputs().to(dtype)
    u = x.double()
    n = x.numel()
    xd = dev(x, dtype)
    ones = torch.ones(n, device=DEV, dtype=dtype)
    (fo, out), (fd, dx) = guarded((n,), dtype), guarded((n,), dtype)
    hip.check(hip.lib().rho_act_add(xd.data_ptr(), None, None, out.data_ptr(), hip.dtype_code(dtype), 1, 16, 64, code, hip.stream()), "rho_act_add")
    hip.check(hip.lib().rho_act_bwd(xd.data_ptr(), ones.data_ptr(), dx.data_ptr(), hip.dtype_code(dtype), n, code, hip.stream()), "rho_act_bwd")
    torch.cuda.synchronize()
    assert guards_intact(fo) and guards_intact(fd)
    for got, deriv, name in ((out, False, "rho_act_add"), (dx, True, "rho_act_bwd")):
        want = (EC.dact64 if deriv else EC.act64)(u, code).reshape(-1)
        mag = (EC.dact_mag64 if deriv else EC.act_mag64)(u, code).reshape(-1)
        _judge(got, want, _act_ulps(code, deriv) * f32_ulp(mag), mag, dtype, f"{name} {EC.ACT_NAMES[code]} {_dn(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("code", [1, 2, 3])
def test_activation_codes_groupnorm_forward(hip, code, dtype):
    """gamma = 1, beta = 0: u = fma(xhat, 1, 0) = xhat = fl(fl(x - mean) * rstd) with the mean / rstd the launch itself returns, which
    are first held to fp64 statistics of this input within their derived bound: torch's float32 gives that u bit for bit, and
    y = act(u) per element."""
    N, S, C, groups = 1, 16, 64, 2
    x = EC.code_inputs().reshape(N, S, C).to(dtype)
    y, st = _gn_fwd(hip, dev(x, dtype), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), dtype, N, S, C, groups, code)
    # the statistics of this real-valued input against fp64.  m = 512: a thread adds two elements in fp32 (one rounding of the
    # sum, two of the fma chain of squares) before the fp64 carry: |dmean| <= u (mean |x| + |mean|) with the rounding to fp32;
    # E[x^2] is off by at most 2 u relative, so |dvar| <= 2 u E[x^2] + 2 |mean| |dmean| and rstd by dvar / (2 (var + eps)) relative,
    # plus its own rounding
    xg = V1._group_view(x.double(), dict(N=N, S=S, groups=groups, cpg=C // groups))
    m64, ax, e2 = xg.mean(1), xg.abs().mean(1), (xg * xg).mean(1)
    v64 = e2 - m64 * m64
    dm = U * (ax + m64.abs())
    r64 = 1.0 / torch.sqrt(v64 + V1.V1_EPS)
    dr = r64 * ((2 * U * e2 + 2 * m64.abs() * dm) / (2 * (v64 + V1.V1_EPS)) + U)
    assert_within_abs(st[..., 0].reshape(-1), m64, dm, f"rho_groupnorm_act {EC.ACT_NAMES[code]} {_dn(dtype)}: mean [N * groups]")
    assert_within_abs(st[..., 1].reshape(-1), r64, dr, f"rho_groupnorm_act {EC.ACT_NAMES[code]} {_dn(dtype)}: rstd [N * groups]")
    s = st.cpu()
    mu, rstd = s[..., 0].repeat_interleave(C // groups, 1)[:, None, :], s[..., 1].repeat_interleave(C // groups, 1)[:, None, :]
    u = ((x.float() - mu) * rstd).double()
    want, mag = EC.act64(u, code), EC.act_mag64(u, code)
    _judge(y, want, _act_ulps(code, False) * f32_ulp(mag), mag, dtype, f"rho_groupnorm_act {EC.ACT_NAMES[code]} {_dn(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("code", [1, 2, 3])
def test_activation_codes_groupnorm_backward(hip, code, groups, dtype):
    """N = S = 1, C = 1024 (cpg = 1024 and 256), mean 0, rstd 1, gamma 1, beta 0 supplied, dy = 1: u = x exactly and every channel sum has
    ONE term, so dbeta[c] = act'(x_c) (the activation allowance alone) and dgamma[c] = fl(act'(x_c) * x_c) (one rounding more).
    dx = gq - m1 - x m2 with m1 = mean(gq), m2 = mean(gq x) over the group: each gq within a = ACT_ULPS u of its term magnitude Mq,
    the means within a u mean(Mq) and a u mean(Mq |x|), the products gq * x inside m2 round once (u mean(|gq x|)), and m1, m2 and the
    expression round as in V1_DX_ULPS:
        |ddx| <= a u (Mq + mean(Mq) + |x| mean(Mq |x|)) + 3 u (|gq| + |m1| + |x m2|) + u |x| mean(|gq x|)."""
    C = 1024
    cpg = C // groups
    x = EC.code_inputs().reshape(1, 1, C).to(dtype)
    u = x.double()
    stats = torch.tensor([0.0, 1.0]).repeat(groups).reshape(1, groups, 2)
    zeros = torch.zeros(C)
    dx, dg, db = _gn_bwd(hip, dev(x, dtype), torch.ones(1, 1, C, device=DEV, dtype=dtype), dev(stats), torch.ones(C, device=DEV),
                         torch.zeros(C, device=DEV), zeros, zeros, dtype, 1, 1, C, groups, code)
    a = _act_ulps(code, True)
    gq, mq = EC.dact64(u, code), EC.dact_mag64(u, code)
    what = f"rho_groupnorm_act_bwd {EC.ACT_NAMES[code]} groups={groups} {_dn(dtype)}"
    _judge(db, gq.reshape(C), a * f32_ulp(mq.reshape(C)), mq.reshape(C), F32, what + ": dbeta")
    _judge(dg, (gq * u).reshape(C), (a + 1) * f32_ulp((mq * u.abs()).reshape(C)), (mq * u.abs()).reshape(C), F32, what + ": dgamma")

    def gmean(t):
        return t.reshape(groups, cpg).mean(1).repeat_interleave(cpg).reshape(1, 1, C)
    m1, m2 = gmean(gq), gmean(gq * u)
    want = gq - m1 - u * m2
    mag = gq.abs() + m1.abs() + (u * m2).abs()
    bound = a * U * (mq + gmean(mq) + u.abs() * gmean(mq * u.abs())) + 3 * U * mag + U * u.abs() * gmean((gq * u).abs())
    _judge(dx, want, bound, mag, dtype, what + ": dx")


# ----------------------------------------------------------------------------- rho_act_add addends
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("has_r,has_nc", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("code", [0, 2])
def test_act_add_addends_bit_exact(hip, code, has_r, has_nc, dtype):
    N, S, C = V1.ACT_ADD_SHAPE
    o = V1.act_add_operands()
    want = EC.act64(o["x"], code)
    if has_r:
        want = want + o["r"].double()
    if has_nc:
        want = want + o["nc"].double()[:, None, :]
    xd, rd, ncd = dev(o["x"], dtype), dev(o["r"], dtype) if has_r else None, dev(o["nc"]) if has_nc else None
    fo, out = guarded((N, S, C), dtype)
    hip.check(hip.lib().rho_act_add(xd.data_ptr(), hip.ptr(rd), hip.ptr(ncd), out.data_ptr(), hip.dtype_code(dtype), N, S, C, code, hip.stream()),
              "rho_act_add")
    torch.cuda.synchronize()
    assert guards_intact(fo)
    assert float(want.abs().max()) <= 256
    assert_bit_equal(out, want, f"rho_act_add act={code} r={has_r} nc={has_nc} {_dn(dtype)} [N, S, C]")
