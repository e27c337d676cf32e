"""-m gpu: the loss side of csrc/gaussian.hip (VLB terms, prior, hybrid loss and its gradient, per-sample MSE, the losses.py metrics)
against the float64 reference of tests/gd_loss_ref.py with per-element bounds fixed on the CPU (its docstring has the constants and how
they were measured; test_gd_loss_ref_host.py holds the float32 restatement to half of each), at the per-sample sizes where the kernels
take another path (gd_loss_ref.CASES), batches of 1, 3 and 5, t mixing 0, a middle step and T - 1, every learned / fixed variance
and mean type, with and without the quantile threshold, inputs built by regime (bounded / saturated) with the branch edges of x_start
placed in every sample.  What has no transcendental (pred_xstart, the mean half of the gradient, the MSE backward) is compared bit
for bit with the float32 restatement.  -s prints the worst error / bound seen per quantity."""
import numpy as np
import pytest
import torch

import gd_loss_ref as R
from gpu_util import DEV, SENT, Guarded, bits, check_bound, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
WORST = {}
MT = {"START_X": 0, "EPSILON": 1}
VT = {R.LEARNED: 0, R.LEARNED_RANGE: 1}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _t64(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def _chk(key, got, ref, bound, mask=None):
    """check_bound over the elements of ``mask``; records the worst error / bound"""
    got, ref, bound = got.double().cpu().reshape(-1), _t64(ref).reshape(-1), _t64(bound).reshape(-1)
    if mask is not None:
        m = torch.from_numpy(np.ascontiguousarray(mask)).reshape(-1)
        got, ref, bound = got[m], ref[m], bound[m]
    if got.numel() == 0:
        return
    frac = ((got - ref).abs() / bound.clamp(min=1e-300)).max()
    WORST[key] = max(WORST.get(key, 0.0), float(frac))
    check_bound(got, ref, bound, key)


def _report():
    print("worst GPU error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def _tab():
    return _dev(R.tables())


def _is_log_clamp(vals):
    """every element is the device's logf(1e-12f): one bit pattern, within 1 ulp (the accuracy of the device's logf) of the correctly
    rounded value"""
    b = bits(vals).flatten()
    return b.numel() == 0 or (bool((b == b[0]).all()) and abs(int(b[0]) - int(R.LOG_CLAMP32.view(np.int32))) <= 1)


# ---------------------------------------------------------------------------------------------------------------- VLB terms, prior
@pytest.mark.parametrize("mean", R.MEANS)
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=R.CASE_IDS)
def test_vlb_terms_per_sample_within_the_mean_bounds(ci, mean):
    from rho_diffusion_amd.engine import ops
    n, B, _ = R.CASES[ci]
    em, tab32, tab = mean == "EPSILON", R.tables(), _tab()
    for vi, var in enumerate((None,) + R.VARS):
        for quant in (False, True):
            t, xs, xt, noise, mo = R.case_inputs(ci, mean, var, quant)
            xsd, xtd, td = _dev(xs), _dev(xt), _dev(t)
            if var is None:
                m_view, v_view = _dev(mo), None
            else:                                                       # the two halves of one [B, 2C, ...] tensor, read in place
                mod = _dev(mo).view(B, 2, n)
                m_view, v_view = mod[:, 0], mod[:, 1]
            q = s = None
            if quant:                                                   # as the pipeline: the device quantile of the unthresholded x0
                pre = m_view if not em else _dev(R._x0(R.N32, R.rows_at(R.N32, tab32, t), xt, mo[:, :n], True))
                q = ops.abs_quantile(pre, 0.9)
                s = np.maximum(q.cpu().numpy(), f32(1.0))
            with_noise = (ci + vi + int(quant)) % 2 == 0
            outs = torch.full((3, B, 3), SENT, device=DEV)               # out_stride = 3: column 1 of a [B, 3] tensor each
            raw_kl, raw_nll, px = Guarded(B), Guarded(B), Guarded(B * n)
            ops.gd_vlb_terms(xsd, xtd, m_view, td, tab, MT[mean], q, _dev(noise) if with_noise else None, outs[0, :, 1], outs[1, :, 1],
                             outs[2, :, 1] if with_noise else None, raw_kl.v, raw_nll.v, px.v.view(B, n), var_values=v_view,
                             var_type=None if var is None else VT[var])
            torch.cuda.synchronize()
            o = R.vlb_terms(tab32, t, xs, xt, mo[:, :n], mo[:, n:] if var else None, em, var, s, noise if with_noise else None)
            what = f"{mean}/{var}/q{int(quant)}"
            assert raw_kl.intact() and raw_nll.intact() and px.intact(), what
            assert bool((outs[:, :, 0] == SENT).all()) and bool((outs[:, :, 2] == SENT).all()), what
            assert same_bits(px.cpu().view(B, n), torch.from_numpy(o["n32"]["x0"] + np.zeros_like(xs))), what
            assert (o["regime"] == R.BETWEEN).mean() <= 0.05, what
            _chk("vlb kl", raw_kl.cpu(), o["kl"], o["kl_bound"])
            _chk("vlb nll", raw_nll.cpu(), o["nll"], o["nll_bound"])
            t0 = torch.from_numpy(t == 0)
            assert same_bits(outs[0, :, 1], torch.where(t0, raw_nll.cpu(), raw_kl.cpu())), what
            _chk("vlb xstart_mse", outs[1, :, 1], o["xstart_mse"], o["xstart_mse_bound"])
            if with_noise:
                _chk("vlb mse", outs[2, :, 1], o["mse"], o["mse_bound"])
            else:
                assert bool((outs[2] == SENT).all()), what
    _report()


@pytest.mark.parametrize("ci", R.PRIOR_CASES, ids=lambda ci: R.CASE_IDS[ci])
def test_prior_bpd_within_the_mean_bound(ci):
    from rho_diffusion_amd.engine import ops
    n, B, _ = R.CASES[ci]
    xs = R.prior_inputs(ci)
    out = torch.full((B, 3), SENT, device=DEV)
    ops.gd_vlb_terms(_dev(xs), None, None, None, _tab(), 0, None, None, out[:, 2], prior=True)
    ref, bound = R.prior_terms(R.tables(), xs)
    _chk("prior", out[:, 2], ref, bound)
    assert bool((out[:, :2] == SENT).all())
    _report()


# ---------------------------------------------------------------------------------------------------------------- hybrid loss
def _hybrid(t, xs, xt, tg, mo, em, var, scale, g, shifts=(0, 0, 0, 0, 0)):
    """rho_gd_hybrid_loss and rho_gd_hybrid_loss_bwd on buffers with sentinels either side, each ``shifts`` floats past a 256-byte
    boundary (x_start, x_t, target, model_out, grad) -> loss, mse, vb [B], grad [B, 2n] on the CPU"""
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    L = hip.lib()
    B, n = xs.shape
    bufs = [Guarded(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1), shift=sh) for a, sh in zip((xs, xt, tg, mo), shifts)]
    td, tab = _dev(t), _tab()
    loss, mse, vb, grad = Guarded(B), Guarded(B), Guarded(B), Guarded(2 * B * n, shift=shifts[4])
    ws = ops.gd_workspace(B, n, DEV)
    head = [b.ptr for b in bufs] + [td.data_ptr(), tab.data_ptr(), R.T, int(em), VT[var], 0 if scale is None else 1, float(scale or 0.0)]
    rc = L.rho_gd_hybrid_loss(*head, loss.ptr, mse.ptr, vb.ptr, ws.data_ptr(), B, n, None, hip.stream())
    assert rc == 0
    gd = [None if a is None else _dev(a) for a in g]
    rc = L.rho_gd_hybrid_loss_bwd(*head, *[None if a is None else a.data_ptr() for a in gd], grad.ptr, B, n, None, hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [loss, mse, vb, grad])
    return loss.cpu(), mse.cpu(), vb.cpu(), grad.cpu().view(B, 2 * n)


@pytest.mark.parametrize("var", R.VARS)
@pytest.mark.parametrize("mean", R.MEANS)
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=R.CASE_IDS)
def test_hybrid_loss_and_gradient_within_the_bounds(ci, mean, var):
    n, B, _ = R.CASES[ci]
    em, tab32 = mean == "EPSILON", R.tables()
    scale = 0.02 if ci % 2 else None
    t, xs, xt, noise, mo = R.case_inputs(ci, mean, var)
    tg = noise if em else xs
    for which in (1, 3):                                                 # g_loss alone, then g_loss, g_mse and g_vb
        g = R.upstream(B, which)
        loss, mse, vb, grad = _hybrid(t, xs, xt, tg, mo, em, var, scale, g)
        h = R.hybrid_loss(tab32, t, xs, xt, tg, mo, em, var, scale, *g)
        h32 = R.hybrid32(tab32, t, xs, xt, tg, mo, em, var, scale, *g)
        _chk("hybrid mse", mse, h["mse"], h["mse_bound"])
        _chk("hybrid vb", vb, h["vb"], h["vb_bound"])
        _chk("hybrid loss", loss, h["loss"], h["loss_bound"])
        assert same_bits(loss, mse + vb)
        # the mean half carries the MSE gradient only: -((g_loss + g_mse) / n) * (2 * (target - m)), bit for bit
        assert same_bits(grad[:, :n], torch.from_numpy(h32["grad"][:, :n])), (mean, var, which)
        gv, reg = grad[:, n:], h["regime"]
        t0 = np.ascontiguousarray(np.broadcast_to(h["t0"], reg.shape))
        assert (reg == R.BETWEEN).mean() <= 0.05
        assert bool(torch.isfinite(gv).all())
        _chk("hybrid grad nll", gv, h["grad"][:, n:], h["grad_v_bound"], t0 & (reg == R.BOUNDED))
        _chk("hybrid grad kl", gv, h["grad"][:, n:], h["grad_v_bound"], ~t0)
        sat = torch.from_numpy(t0 & (reg == R.SATURATED))
        assert bool((h["grad"][:, n:][sat] == 0).all()) and bool((gv[sat] == 0).all()), (mean, var, which)
        if n >= 16 and t0.any():
            assert bool(sat.any()) and float(gv[torch.from_numpy(t0)].abs().max()) > 0
    if n == 263172:                                                      # fixed-order reduction over 258 chunks: the same bits again
        again = _hybrid(t, xs, xt, tg, mo, em, var, scale, g)
        assert all(same_bits(a, b) for a, b in zip(again, (loss, mse, vb, grad)))
    _report()


def test_hybrid_loss_with_misaligned_bases_gives_the_bits_of_the_aligned_call():
    """n = 1028 (the 16-byte path when aligned): each operand alone one float off 16 bytes, then all of them: the scalar kernels.  The
    gradient is elementwise, so its bits are the same by construction.  loss, mse and vb are per-sample sums taken in another fixed
    order (float64 partials of float32 terms, one rounding to float32 at the end): that they come out with the same bits holds for
    these deterministic inputs, not for every input - a sum that lands within 2^-53 relative of a float32 rounding boundary could
    differ by one ulp."""
    ci = 7
    n, B, _ = R.CASES[ci]
    for mean, var in (("EPSILON", R.LEARNED_RANGE), ("START_X", R.LEARNED)):
        em = mean == "EPSILON"
        t, xs, xt, noise, mo = R.case_inputs(ci, mean, var)
        tg = noise if em else xs
        g = R.upstream(B, 3)
        want = _hybrid(t, xs, xt, tg, mo, em, var, 0.02, g)
        for shifts in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (1, 2, 3, 1, 3)):
            got = _hybrid(t, xs, xt, tg, mo, em, var, 0.02, g, shifts)
            assert all(same_bits(a, b) for a, b in zip(got, want)), (mean, var, shifts)


# ---------------------------------------------------------------------------------------------------------------- per-sample MSE
@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=R.CASE_IDS)
def test_mse_per_sample_forward_and_backward(ci):
    from rho_diffusion_amd.engine import ops
    n, B, _ = R.CASES[ci]
    t, xs, xt, noise, mo = R.case_inputs(ci, "START_X", None)
    g = R.upstream(B, 1)[0]
    got = ops.gd_mse_per_sample(_dev(xs), _dev(mo))
    ref = ((xs.astype(np.float64) - mo.astype(np.float64)) ** 2).mean(1)
    _chk("mse_per_sample", got, ref, 4 * R.U * np.abs(ref))
    assert same_bits(ops.gd_mse_per_sample_bwd(_dev(xs), _dev(mo), _dev(g)), torch.from_numpy(R.mse32(xs, mo, g)))
    _report()


# ---------------------------------------------------------------------------------------------------------------- metrics
def _operands(ops_np, modes):
    """(tensor or None, mode, scalar) per operand: a full [B, n] array (mode 0), a per-sample [B, 1] array (1) or a numpy scalar (2)"""
    return [(None, 2, float(a)) if md == 2 else (_dev(a), md, 0.0) for a, md in zip(ops_np, modes)]


@pytest.mark.parametrize("B,n", R.METRIC_SHAPES)
def test_metrics_elementwise_within_the_bounds(B, n):
    from rho_diffusion_amd.engine import ops
    x, means, ls = R.metric_inputs(B, n, f"gdm_{B}_{n}")
    o = R.dgll(x, means, ls)
    out = Guarded(B * n)
    ops.discretized_gaussian_ll(_operands((x, means, ls), (0, 0, 0)), out.v, B, n)
    torch.cuda.synchronize()
    got, reg = out.cpu().view(B, n), o["regime"]
    assert out.intact() and bool(torch.isfinite(got).all()) and (reg == R.BETWEEN).mean() <= 0.05
    _chk("dgll", got, o["value"], o["bound"], reg == R.BOUNDED)
    sat = got[torch.from_numpy(reg == R.SATURATED)]
    assert sat.numel() >= B * n // 10 and _is_log_clamp(sat)
    rest = got[torch.from_numpy(reg == R.BETWEEN)]
    assert all(_is_log_clamp(torch.stack([v, sat[0]])) or float(v) >= float(R.LOG_QUANT32) for v in rest)
    edge = np.isin(x, R.EDGE_X)                                           # +-1, +-0.999 and their neighbours: the branch the reference takes
    assert edge.sum() >= 8 * B
    _chk("dgll edges", got, o["value"], o["bound"], edge & (reg == R.BOUNDED))
    for modes, ops_np in R.metric_mode_operands(B, n, "dgll"):
        o = R.dgll(*ops_np)
        out = Guarded(B * n)
        ops.discretized_gaussian_ll(_operands(ops_np, modes), out.v, B, n)
        torch.cuda.synchronize()
        assert out.intact(), modes
        _chk("dgll", out.cpu(), o["value"].expand(B, n), o["bound"].expand(B, n))
    for modes, ops_np in R.metric_mode_operands(B, n, "kl"):
        ref, bound = R.normal_kl(*ops_np)
        out = Guarded(B * n)
        ops.normal_kl(_operands(ops_np, modes), out.v, B, n)
        torch.cuda.synchronize()
        assert out.intact(), modes
        _chk("normal_kl", out.cpu(), ref.expand(B, n), bound.expand(B, n))
    _report()


def test_approx_normal_cdf_bound_saturation_and_monotonicity():
    from rho_diffusion_amd.engine import ops
    u = R.cdf_inputs()
    out = Guarded(u.size)
    ops.approx_normal_cdf(_dev(u), out.v)
    torch.cuda.synchronize()
    got = out.cpu()
    assert out.intact()
    _chk("cdf", got, R.cdf(u), R.cdf_bound(u), np.abs(u) <= 12)
    ut = torch.from_numpy(u)
    assert bool((got[ut > 12] == 1).all()) and bool((got[ut < -12] == 0).all()) and bool((got[1:] >= got[:-1]).all())
    _report()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_return_their_codes_and_write_nothing():
    from rho_diffusion_amd import hip
    L = hip.lib()
    E_ARG, E_SHAPE = -1, -3
    B, n = 2, 8
    a = [Guarded(torch.zeros(2 * B * n)) for _ in range(5)]
    outs = [Guarded(2 * B * n) for _ in range(6)]
    t, tab, ws = torch.zeros(B, dtype=torch.int64, device=DEV), _tab(), torch.zeros(64, dtype=torch.float64, device=DEV)
    p = [b.ptr for b in a]
    o = [b.ptr for b in outs]
    tp, tabp, wsp, st = t.data_ptr(), tab.data_ptr(), ws.data_ptr(), hip.stream()

    def vlb(**kw):
        k = dict(xs=p[0], xt=p[1], mo=p[2], t=tp, tab=tabp, mt=0, prior=0, vb=o[0], stride=1, ws=wsp, B=B, n=n)
        k.update(kw)
        return L.rho_gd_vlb_terms(k["xs"], k["xt"], k["mo"], k["t"], k["tab"], R.T, k["mt"], None, None, k["prior"], k["vb"], o[1], None,
                                  k["stride"], o[2], o[3], o[4], k["ws"], k["B"], k["n"], None, st)

    def vlb_lv(ms=n, vs=n, stride=1, B_=B, vv=p[3]):
        return L.rho_gd_vlb_terms_lv(p[0], p[1], p[2], ms, vv, vs, tp, tabp, R.T, 0, 1, None, None, o[0], o[1], None, stride, o[2], o[3],
                                     o[4], wsp, B_, n, None, st)

    def hyb(B_=B, xs=p[0], loss=o[0]):
        return L.rho_gd_hybrid_loss(xs, p[1], p[2], p[3], tp, tabp, R.T, 0, 1, 0, 0.0, loss, o[1], o[2], wsp, B_, n, None, st)

    def hyb_bwd(B_=B, grad=o[5], mo=p[3]):
        return L.rho_gd_hybrid_loss_bwd(p[0], p[1], p[2], mo, tp, tabp, R.T, 0, 1, 0, 0.0, p[4], None, None, grad, B_, n, None, st)

    assert vlb(B=65536) == E_SHAPE and vlb_lv(B_=65536) == E_SHAPE and hyb(B_=65536) == E_SHAPE and hyb_bwd(B_=65536) == E_SHAPE
    assert L.rho_gd_mse_per_sample(p[0], p[1], o[0], wsp, 65536, n, st) == E_SHAPE
    assert L.rho_gd_mse_per_sample_bwd(p[0], p[1], p[4], o[5], 65536, n, st) == E_SHAPE
    assert vlb(stride=0) == E_ARG and vlb_lv(stride=0) == E_ARG
    assert vlb_lv(ms=n - 1) == E_ARG and vlb_lv(vs=n - 1) == E_ARG
    assert vlb(xs=None) == E_ARG and vlb(vb=None) == E_ARG and vlb(ws=None) == E_ARG and vlb(mo=None) == E_ARG and vlb(t=None) == E_ARG
    assert vlb(mt=2) == E_ARG and vlb_lv(vv=None) == E_ARG
    assert hyb(xs=None) == E_ARG and hyb(loss=None) == E_ARG and hyb_bwd(grad=None) == E_ARG and hyb_bwd(mo=None) == E_ARG
    assert L.rho_gd_mse_per_sample(p[0], None, o[0], wsp, B, n, st) == E_ARG
    assert L.rho_gd_mse_per_sample_bwd(p[0], p[1], None, o[5], B, n, st) == E_ARG
    z = (0.0,) * 4
    assert L.rho_normal_kl(p[0], p[1], p[2], p[3], *z, 3, o[0], B, n, st) == E_ARG                 # operand 0 in mode 3
    assert L.rho_normal_kl(p[0], p[1], p[2], p[3], *z, 3 << 6, o[0], B, n, st) == E_ARG
    assert L.rho_normal_kl(p[0], p[1], p[2], p[3], *z, 1 << 8, o[0], B, n, st) == E_ARG            # a fifth field
    assert L.rho_normal_kl(None, p[1], p[2], p[3], *z, 0, o[0], B, n, st) == E_ARG and L.rho_normal_kl(p[0], p[1], p[2], p[3], *z, 0, None, B, n, st) == E_ARG
    assert L.rho_discretized_gaussian_ll(p[0], p[1], p[2], *z[:3], 3 << 2, o[0], B, n, st) == E_ARG
    assert L.rho_discretized_gaussian_ll(p[0], None, p[2], *z[:3], 1 << 2, o[0], B, n, st) == E_ARG
    assert L.rho_approx_normal_cdf(None, o[0], n, st) == E_ARG and L.rho_approx_normal_cdf(p[0], None, n, st) == E_ARG
    assert L.rho_approx_normal_cdf(p[0], o[0], 0, st) == E_ARG
    torch.cuda.synchronize()
    for b in outs:
        assert b.intact() and bool(torch.isnan(b.v).all())
    # the same calls are accepted once the argument is right
    assert vlb() == 0 and L.rho_normal_kl(None, p[1], p[2], p[3], 0.5, 0.0, 0.0, 0.0, 2, o[0], B, n, st) == 0
    torch.cuda.synchronize()
