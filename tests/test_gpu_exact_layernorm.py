"""-m gpu: the LayerNorm kernels and the element-wise kernels of csrc/vit.hip, element by element.

LayerNorm (rho_layernorm_fwd / rho_layernorm_bwd).  tests/ln_cases.py holds the cases - the smallest shapes that reach every (G, NV)
instantiation up to NV = 8 at LN_MAX_E, idle lanes, a ragged last vector, a row count that is no multiple of the rows per block, one
row, and a backward whose row loop sweeps three times with a partly live block and a block that has no row group left - with their
fp64 references and a Python twin of ln_geom / ln_bps; tests/test_ln_cases_host.py proves on the CPU what is taken for granted here.
Each test first checks the twin against rho_layernorm_bwd_workspace_bytes and asserts that the case reaches its branch.
  backward: mean / rstd are inputs at the C ABI (integer mean, rstd in {0.5, 1, 2}); with integer x, add, gamma and dy every column sum
    is exact in any order, so dgamma, dbeta (written and accumulated), every (b, k) partial row of the workspace and, at the
    power-of-two widths, dx and dadd equal fp64 bit for bit; at the other widths fl(1 / E) is inexact and dx / dadd are held to the
    per-element bounds derived in ln_cases.py.
  forward: integer x with integer row means: mean bit-equal, rstd and y within the derived ulps; bf16 y by the tie rule of
    exact_util.py.  One non-integer case per dtype (rows offset by +100) is judged row by row.
Element-wise (rho_bias_act / _bwd, rho_pos_add / _bwd): per element on embed_cases.code_inputs(); see the bounds below.
Every output lies between guard bands and starts as NaN unless the launch accumulates onto it."""
import pytest
import torch
import torch.nn.functional as F

import embed_cases as EC
import ln_cases as LN
from exact_util import (assert_bf16_tie_rule, assert_bit_equal, assert_within_abs, assert_within_ulps, bf16_store_bound,
                        f32_ulp, guarded, guarded_copy, guards_intact, int_choice, int_tensor, tie_margin)
from detdata import det_normal, det_uniform
from ln_cases import BF16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"

_ids = [LN.case_id(c, dt) for c, dt in LN.LN_PARAMS]
FWD_PARAMS = [(c, dt) for c, dt in LN.LN_PARAMS if c["rows"] * c["E"] <= 2 ** 21]    # the multi-sweep shapes are the backward's


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module")
def cache():
    """Operands and references computed once per key and left unchanged."""
    store = {}

    def get(key, make):
        if key not in store:
            store[key] = make()
        return store[key]
    return get


def dev(t, dtype=F32):
    return None if t is None else t.to(DEV).to(dtype).contiguous()


def _layout(hip, c, dtype):
    """The twin's layout of the case, checked against the library's own workspace size, with the case's branch asserted reached."""
    L = LN.ln_layout(c, dtype)
    need = int(hip.lib().rho_layernorm_bwd_workspace_bytes(c["rows"], L["rps"], c["E"], hip.dtype_code(dtype), int(c["add"])))
    assert need == L["workspace_bytes"], f"{LN.case_id(c, dtype)}: the library wants {need} bytes, the geometry twin {L['workspace_bytes']}: {L}"
    assert LN.BRANCHES[c["branch"]](c, L), f"{LN.case_id(c, dtype)} does not reach {c['branch']}: {L}"
    return L


# ----------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("c,dtype", LN.LN_PARAMS, ids=_ids)
def test_layernorm_backward(hip, cache, c, dtype):
    L = _layout(hip, c, dtype)
    o = cache(("bo", c["name"]), lambda: LN.ln_bwd_operands(c))
    r = cache(("br", c["name"]), lambda: LN.ln_bwd_reference(c, o))
    m = LN.ln_bwd_model32(c, o, dtype)
    R, E, nb, bps = c["rows"], c["E"], L["nb"], L["bps"]
    what = LN.case_id(c, dtype)
    x, dy, add, gamma = dev(o["x"], dtype), dev(o["dy"], dtype), dev(o["add"]), dev(o["gamma"])
    stats = dev(torch.stack([o["mean"], o["rstd"]], 1))
    fdx, dx = guarded_copy(o["pre_dx"], dtype) if c["acc_dx"] else guarded((R, E), dtype)
    fdg, dg = guarded_copy(o["pre_dgamma"], F32) if c["acc_params"] else guarded((E,), F32)
    fdb, db = guarded_copy(o["pre_dbeta"], F32) if c["acc_params"] else guarded((E,), F32)
    fda, dadd = guarded((nb, E), F32) if c["dadd"] else (None, None)
    fws, ws = guarded((nb, bps, 3, E), F32)
    hip.check(hip.lib().rho_layernorm_bwd(dy.data_ptr(), x.data_ptr(), hip.ptr(add), stats.data_ptr(), gamma.data_ptr(), dx.data_ptr(),
                                          int(c["acc_dx"]), hip.ptr(dadd), dg.data_ptr(), db.data_ptr(), int(c["acc_params"]), ws.data_ptr(),
                                          L["workspace_bytes"], hip.dtype_code(dtype), R, L["rps"], E, hip.stream()), "rho_layernorm_bwd")
    torch.cuda.synchronize()
    for f, n in ((fdx, "dx"), (fdg, "dgamma"), (fdb, "dbeta"), (fda, "dadd"), (fws, "workspace")):
        assert f is None or guards_intact(f), f"{what}: store outside {n}"
    # the partial rows [b][k][comp][E] the finalize reads: comp 0 = sum dy xhat, 1 = sum dy over the rows block (k, b) sweeps
    part = ws.cpu()
    assert_bit_equal(part[:, :, 0], m["part"][:, :, 0], what + ": partial rows of dy * xhat [nb, bps, E]")
    assert_bit_equal(part[:, :, 1], m["part"][:, :, 1], what + ": partial rows of dy [nb, bps, E]")
    assert_bit_equal(dg, r["dgamma"], what + ": dgamma [E]")
    assert_bit_equal(db, r["dbeta"], what + ": dbeta [E]")
    if LN.dx_is_exact(c):
        # exact in fp32 (host twin); bf16 rounds that exact value once, to nearest even, as torch does
        assert_bit_equal(dx, r["dx"].float().to(dtype), what + ": dx [rows, E]")
        if c["add"]:
            assert_bit_equal(part[:, :, 2], m["part"][:, :, 2], what + ": partial rows of dx [nb, bps, E]")
        if c["dadd"]:
            assert_bit_equal(dadd, r["dadd"], what + ": dadd [nb, E]")
    else:
        ulps = LN.DX_ULPS + (1 if c["acc_dx"] else 0)          # the addition of what dx held rounds once more
        mag = r["dx_mag"] + (o["pre_dx"].double().abs() if c["acc_dx"] else 0.0)
        if dtype == F32:
            worst = assert_within_ulps(dx, r["dx"], ulps, what + ": dx [rows, E] (ulps of rstd (|g| + |m1| + |xhat m2|))", mag=mag)
            print(f"measured: ln bwd {what}: dx worst {worst:.3f} ulp (derived {ulps})")
        else:
            assert_within_abs(dx, r["dx"], bf16_store_bound(r["dx"], ulps * f32_ulp(mag)), what + ": dx [rows, E] (fp32 bound + half a bf16 ulp)")
        if c["dadd"]:
            # each row's dx within DX_ULPS u of its magnitude, and rps - 1 additions in any order: (DX_ULPS + rps) u sum Mag
            bound = (LN.DX_ULPS + L["rps"]) * LN.U * r["dadd_mag"]
            worst = float(((dadd.cpu().double() - r["dadd"]).abs() / bound).max())
            print(f"measured: ln bwd {what}: dadd worst {worst:.3f} of the derived bound (per element)")
            assert_within_abs(dadd, r["dadd"], bound, what + ": dadd [nb, E]")


# ----------------------------------------------------------------------------- LayerNorm forward
# rstd: RSTD_ULPS = 3 by derivation (ln_cases.py); y: Y_ULPS = 5 of |xhat gamma| + |beta|.
@pytest.mark.parametrize("c,dtype", FWD_PARAMS, ids=[LN.case_id(c, dt) for c, dt in FWD_PARAMS])
def test_layernorm_forward(hip, cache, c, dtype):
    L = _layout(hip, c, dtype)
    o = cache(("fo", c["name"]), lambda: LN.ln_fwd_operands(c))
    r = cache(("fr", c["name"]), lambda: LN.ln_fwd_reference(c, o))
    R, E = c["rows"], c["E"]
    what = LN.case_id(c, dtype)
    fy, y = guarded((R, E), dtype)
    fs, st = guarded((R, 2), F32)
    x, add, gamma, beta = dev(o["x"], dtype), dev(o["add"]), dev(o["gamma"]), dev(o["beta"])
    hip.check(hip.lib().rho_layernorm_fwd(x.data_ptr(), hip.ptr(add), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                          st.data_ptr(), hip.dtype_code(dtype), R, L["rps"], E, hip.stream()), "rho_layernorm_fwd")
    torch.cuda.synchronize()
    assert guards_intact(fy) and guards_intact(fs), what + ": store outside y / stats"
    assert_bit_equal(st[:, 0], r["mean"], what + ": stats[:, 0] = mean [rows]")
    w_r = assert_within_ulps(st[:, 1], r["rstd"], LN.RSTD_ULPS, what + ": stats[:, 1] = rstd [rows]")
    if dtype == F32:
        w_y = assert_within_ulps(y, r["y"], LN.Y_ULPS, what + ": y [rows, E] (ulps of |xhat gamma| + |beta|)", mag=r["y_mag"])
        print(f"measured: ln fwd {what}: rstd worst {w_r:.3f} ulp (derived {LN.RSTD_ULPS}), y worst {w_y:.3f} ulp (derived {LN.Y_ULPS})")
    else:
        share = assert_bf16_tie_rule(y, r["y"], tie_margin(LN.Y_ULPS, r["y_mag"]), what + ": y [rows, E]")
        print(f"measured: ln fwd {what}: rstd worst {w_r:.3f} ulp (derived {LN.RSTD_ULPS}), y bf16 by the tie rule, {share:.4%} near a tie")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,E", [(7, 96), (5, 1056)])
def test_layernorm_forward_offset_rows_per_row(hip, dtype, R, E):
    """Real inputs, rows offset by +100 (where an E[x^2] - mean^2 variance loses four digits): the project's bars of
    test_gpu_vit_kernels.py (3e-5 float32, 1e-2 bf16), held by every row on its own instead of by the tensor."""
    x = (det_normal((R, E), f"lnoff_x{R}_{E}") + 100.0).to(dtype)
    gamma, beta = 1.0 + 0.2 * det_uniform((E,), f"lnoff_g{E}"), 0.1 * det_uniform((E,), f"lnoff_b{E}")
    fy, y = guarded((R, E), dtype)
    fs, st = guarded((R, 2), F32)
    xd, gd, bd = dev(x, dtype), dev(gamma), dev(beta)
    hip.check(hip.lib().rho_layernorm_fwd(xd.data_ptr(), None, gd.data_ptr(), bd.data_ptr(), y.data_ptr(),
                                          st.data_ptr(), hip.dtype_code(dtype), R, R, E, hip.stream()), "rho_layernorm_fwd")
    torch.cuda.synchronize()
    assert guards_intact(fy) and guards_intact(fs)
    xx = x.double()
    want = F.layer_norm(xx, (E,), gamma.double(), beta.double(), 1e-5)
    err = (y.cpu().double() - want).norm(dim=1) / want.norm(dim=1)
    print(f"measured: ln offset rows R={R} E={E} {dtype}: worst row rel_l2 {float(err.max()):.2e}")
    bar = 1e-2 if dtype == BF16 else 3e-5
    assert bool((err < bar).all()), f"rows {(~(err < bar)).nonzero().flatten().tolist()} exceed {bar}: {err.tolist()}"
    rstd = 1.0 / torch.sqrt(xx.var(1, unbiased=False) + 1e-5)
    assert bool(((st[:, 0].cpu().double() - xx.mean(1)).abs() <= 3e-5 * xx.mean(1).abs()).all())
    assert bool(((st[:, 1].cpu().double() - rstd).abs() <= 3e-5 * rstd).all())


# ----------------------------------------------------------------------------- rho_bias_act / rho_bias_act_bwd
# Bounds: embed_cases.hw_act_bound - code 1 is silu_f / dsilu_f (derived there from the expression), codes 2 - 6 carry ACT_ULPS.
act_bound = EC.hw_act_bound


BA_SHAPES = [(70, 32), (23, 96), (53, 40)]       # cols = 40: (i * PE) % cols wraps inside every block (1024 or 2048 elements)


def _ba_operands(R, C, dtype, with_bias):
    src = EC.code_inputs().reshape(-1)
    x = src.repeat(-(-R * C // src.numel()))[:R * C].reshape(R, C).to(dtype)
    bias = int_choice((C,), f"ba_bias{C}", (-1.0, -0.375, 0.0, 0.25, 0.625)) if with_bias else None
    u32 = x.float() + bias if with_bias else x.float()          # the kernel's one IEEE addition, bit for bit
    return x, bias, u32.double()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("code", [1, 2, 3, 4, 5, 6])
def test_bias_act_per_element(hip, code, with_bias, dtype):
    """y = act(x + bias[c]) and dx = dy * act'(x + bias[c]) with dy in {1, -2, 0.5} (exact products) against act64 / dact64 at the
    kernel's own u = fl(x + bias): every element inside its derived bound; bf16 stores add half a bf16 ulp."""
    L = hip.lib()
    for R, C in BA_SHAPES:
        x, bias, u = _ba_operands(R, C, dtype, with_bias)
        dy = int_choice((R, C), f"ba_dy{R}_{C}", (1.0, -2.0, 0.5))
        xd, bd, dyd = dev(x, dtype), dev(bias), dev(dy, dtype)
        fy, y = guarded((R, C), dtype)
        fd, dx = guarded((R, C), dtype)
        hip.check(L.rho_bias_act(xd.data_ptr(), hip.ptr(bd), y.data_ptr(), hip.dtype_code(dtype), R, C, code, hip.stream()), "rho_bias_act")
        hip.check(L.rho_bias_act_bwd(xd.data_ptr(), hip.ptr(bd), dyd.data_ptr(), dx.data_ptr(), hip.dtype_code(dtype), R, C, code, hip.stream()),
                  "rho_bias_act_bwd")
        torch.cuda.synchronize()
        assert guards_intact(fy) and guards_intact(fd)
        for got, deriv, name in ((y, False, "y"), (dx, True, "dx")):
            want, bound, mag = act_bound(u, code, deriv)
            if deriv:
                want, bound, mag = want * dy.double(), bound * dy.double().abs(), mag * dy.double().abs()
            meas = float(((got.cpu().double() - want).abs() / f32_ulp(mag)).max())
            what = f"bias_act{'_bwd' if deriv else ''} {EC.ACT_NAMES[code]} [{R}, {C}] bias={with_bias} {dtype}: {name}"
            if dtype == F32:
                rel = float(((got.cpu().double() - want).abs() / bound.clamp_min(1e-300)).max()) if code not in EC.INT_ACTS else 0.0
                print(f"measured: {what}: worst {meas:.3f} ulp of the magnitude, {rel:.3f} of the derived bound")
                assert_within_abs(got, want, bound, what)
            else:
                assert_within_abs(got, want, bf16_store_bound(want, bound), what + " (fp32 bound + half a bf16 ulp)")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
def test_pos_add_bit_exact(hip, dtype, B):
    """x[b] += pos in place and dpos = sum over b of dx on integers: exact in any order, so bit-equal; m = 7 * 40 is no multiple of a
    block's elements, so i % mvec wraps inside the blocks."""
    N, E = 7, 40
    h = int_tensor((B, N, E), f"pa_h{B}", 8.0, 100.0)
    pos = int_tensor((N, E), "pa_pos", 8.0, 100.0)
    fx, x = guarded_copy(h, dtype)
    pd, hd = dev(pos), dev(h, dtype)
    hip.check(hip.lib().rho_pos_add(x.data_ptr(), pd.data_ptr(), hip.dtype_code(dtype), B, N * E, hip.stream()), "rho_pos_add")
    fp, dpos = guarded((N, E), F32)
    hip.check(hip.lib().rho_pos_add_bwd(hd.data_ptr(), dpos.data_ptr(), hip.dtype_code(dtype), B, N * E, hip.stream()), "rho_pos_add_bwd")
    torch.cuda.synchronize()
    assert guards_intact(fx) and guards_intact(fp)
    want = h.double() + pos.double()
    assert float(want.abs().max()) <= 256                       # exact in bf16
    assert_bit_equal(x, want, f"pos_add B={B} {dtype}")
    assert_bit_equal(dpos, h.double().sum(0), f"pos_add_bwd B={B} {dtype}")
