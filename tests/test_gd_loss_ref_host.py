"""CPU only: the float64 reference of tests/gd_loss_ref.py against the recorded reference outputs (tests/golden/g18, g19) and the
oracle, and the float32 restatement against the bounds with K / 2 on every input set test_gpu_gaussian_loss_bounds.py uses (the
constants K are fixed here, on the CPU, never from a GPU result: see the table in gd_loss_ref's docstring; -s prints the ratios)."""
import numpy as np
import pytest
import torch

import gd_loss_ref as R
from helpers import det_normal, load_golden

f32 = np.float32
WORST = {}


def _ratio(key, err, bound, k):
    """worst error / (bound / K): must stay <= K / 2"""
    v = R.ratio(err, np.asarray(bound, dtype=np.float64) / (k * R.U))
    WORST[key] = max(WORST.get(key, 0.0), v)
    assert v <= k / 2, (key, v, k)
    return v


def _np(v):
    return v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)


def _tab(T):
    from rho_diffusion_amd.diffusion.gaussian_diffusion import diffusion_tables, gd_table_rows_learned, get_named_beta_schedule
    return gd_table_rows_learned(diffusion_tables(get_named_beta_schedule("cosine", T)))


def _within(ref, golden, bound, what):
    err = np.abs(_np(ref) - np.asarray(golden, dtype=np.float64).reshape(_np(ref).shape))
    assert np.all(err <= _np(bound)), (what, float((err - _np(bound)).max()))


def test_reference_reproduces_recorded_metrics():
    g = load_golden("g18_gaussian_api.npz")
    d = {k: g[f"metrics/{k}"] for k in ("m1", "m2", "lv1", "lv2", "ps_lv", "dx", "dmeans", "dls", "dps_ls")}
    z = np.zeros((), f32)
    for key, ops in (("kl_full", (d["m1"], d["lv1"], d["m2"], d["lv2"])), ("kl_ps", (d["m1"], d["ps_lv"], d["m2"], d["lv2"])),
                     ("kl_scalar", (d["m1"], d["lv1"], z, z))):
        ref, bound = R.normal_kl(*ops)
        _within(ref, g[f"metrics/{key}"], bound, key)
    for key, ls in (("dgll_full", d["dls"]), ("dgll_ps", d["dps_ls"])):
        o = R.dgll(d["dx"], d["dmeans"], ls)
        rec, ok = g[f"metrics/{key}"], o["regime"] == R.BOUNDED
        _within(o["value"][torch.from_numpy(ok)], rec[ok], o["bound"][torch.from_numpy(ok)], key)
        sat = o["regime"] == R.SATURATED
        assert np.all(rec[sat] == R.LOG_CLAMP32), key
        rest = rec[o["regime"] == R.BETWEEN]
        assert np.all(np.isfinite(rest) & ((rest == R.LOG_CLAMP32) | (rest >= R.LOG_QUANT32))), key
    u = d["m1"] * f32(3.0)
    _within(R.cdf(u), g["metrics/cdf"], R.cdf_bound(u), "cdf")


@pytest.mark.parametrize("case,T", [("tiny2d", 50), ("tiny3d", 20)])
def test_reference_reproduces_recorded_vb_terms_and_hybrid_loss(case, T):
    from oracle import ref_torch as O
    from golden_cfg import UNET_CASES
    g, tag = load_golden("g19_learned_variance.npz"), f"{case}_T{T}"
    xshape = UNET_CASES[case][1]
    B = xshape[0]
    tab, otab = _tab(T), O.gd_tables(O.gd_betas("cosine", T))
    x0 = torch.from_numpy(g[f"{tag}/x0"])
    xs = x0.reshape(B, -1).numpy()
    n = xs.shape[1]
    for vt in R.VARS:
        mo = g[f"{tag}/mo_{vt}"].reshape(B, -1)
        for mt in R.MEANS:
            em = mt == "EPSILON"
            for tn, tv in (("t0", 0), ("tk", T // 3)):
                t = torch.full((B,), tv, dtype=torch.long)
                xt = O.gd_q_sample(otab, x0, t, det_normal(xshape, "g19_vb_noise")).reshape(B, -1).numpy()
                o = R.vlb_terms(tab, t.numpy(), xs, xt, mo[:, :n], mo[:, n:], em, vt)
                _within(o["vb"], g[f"{tag}/vb_{vt}_{mt}_{tn}"], o["vb_bound"], (vt, mt, tn))
            t = torch.from_numpy(g[f"{tag}/train_t"])
            noise = det_normal(xshape, "g19_train_noise")
            xt = O.gd_q_sample(otab, x0, t, noise).reshape(B, -1).numpy()
            tg = noise.reshape(B, -1).numpy() if em else xs
            for lt, scale in (("MSE", None), ("RESCALED_MSE", T / 1000.0)):
                k = f"{tag}/train_{vt}_{mt}_{lt}"
                h = R.hybrid_loss(tab, t.numpy(), xs, xt, tg, mo, em, vt, scale, np.full(B, 1.0 / B, f32))
                for name in ("mse", "vb", "loss"):
                    _within(h[name], g[f"{k}/{name}"], h[name + "_bound"], (k, name))
                rec = g[f"{k}/dout"].reshape(B, -1).astype(np.float64)
                gm = h["grad"][:, :n].numpy()
                assert np.all(np.abs(rec[:, :n] - gm) <= 4 * R.U * np.abs(gm)), k
                t0 = np.broadcast_to(h["t0"], h["regime"].shape)
                ok = (h["regime"] == R.BOUNDED) | ~t0
                err = np.abs(rec[:, n:] - h["grad"][:, n:].numpy())
                assert np.all((err <= h["grad_v_bound"].numpy())[ok]), (k, float((err - h["grad_v_bound"].numpy())[ok].max()))
                # saturated: the float32 CDFs are exactly 0 or 1 and the clamp cuts the path, whatever float64 still resolves
                assert np.all(rec[:, n:][t0 & (h["regime"] == R.SATURATED)] == 0), k
                assert (t0 & (h["regime"] == R.BETWEEN)).mean() <= 0.05


def test_chain_agrees_with_the_oracle_q_sample_and_dynamic_threshold():
    from oracle import ref_torch as O
    from rho_diffusion_amd.engine.ops import GD_ROW
    tab, otab = R.tables(), O.gd_tables(O.gd_betas("cosine", R.T))
    for row, key in (("sqrt_recip", "sqrt_recip_alphas_cumprod"), ("sqrt_recipm1", "sqrt_recipm1_alphas_cumprod"),
                     ("coef1", "posterior_mean_coef1"), ("coef2", "posterior_mean_coef2"), ("post_logvar", "posterior_log_variance_clipped"),
                     ("sqrt_abar", "sqrt_alphas_cumprod"), ("log_1m_abar", "log_one_minus_alphas_cumprod")):
        assert np.array_equal(tab[GD_ROW[row]], otab[key].astype(f32)), row
    assert np.array_equal(tab[GD_ROW["log_beta"]], np.log(otab["betas"]).astype(f32))
    t, xs, xt, noise, mo = R.case_inputs(6, "START_X", R.LEARNED, quant=True)
    m = torch.from_numpy(mo[:, :1024].copy())
    s = torch.quantile(m.abs(), 0.9, dim=-1).clamp(min=1.0)
    got = R._x0(R.N32, R.rows_at(R.N32, tab, t), xt, m.numpy(), False, s.numpy().reshape(-1, 1))
    assert np.array_equal(got, O.gd_dynamic_threshold(m).numpy())
    assert float(s.max()) > 1.0 and float(s.min()) == 1.0


def test_metric_restatement_within_half_the_bounds_and_saturated_elements_exact():
    for B, n in R.METRIC_SHAPES:
        x, means, ls = R.metric_inputs(B, n, f"gdm_{B}_{n}")
        o = R.dgll(x, means, ls)
        v32, reg = R.dgll32(x, means, ls), o["regime"]
        assert (reg == R.BETWEEN).mean() <= 0.05 and (reg == R.SATURATED).mean() >= 0.1
        ok = reg == R.BOUNDED
        _ratio("dgll", (v32 - o["value"].numpy())[ok], o["bound"].numpy()[ok], R.K["dgll"])
        assert np.all(v32[reg == R.SATURATED] == R.LOG_CLAMP32)
        edge = np.isin(x, R.EDGE_X)
        assert edge.sum() >= 8 and set(np.unique(o["branch"][edge])) == {0, 1, 2}
        for modes, ops in R.metric_mode_operands(B, n, "dgll"):
            o = R.dgll(*ops)
            assert (o["regime"] == R.BOUNDED).all(), modes
            _ratio("dgll", R.dgll32(*ops) - o["value"].numpy(), o["bound"].numpy(), R.K["dgll"])
        for modes, ops in R.metric_mode_operands(B, n, "kl"):
            ref, bound = R.normal_kl(*ops)
            _ratio("kl", R.normal_kl32(*ops) - ref.numpy(), bound.numpy(), R.K["kl"])
    u = R.cdf_inputs()
    c32, c64 = R.cdf32(u), R.cdf(u).numpy()
    inside = np.abs(u) <= 12
    _ratio("cdf", (c32 - c64)[inside], R.cdf_bound(u).numpy()[inside], R.K["cdf"])
    assert np.all(c32[u > 12] == 1) and np.all(c32[u < -12] == 0) and np.all(np.diff(c32) >= 0)
    for ci in R.PRIOR_CASES:
        xs = R.prior_inputs(ci)
        ref, bound = R.prior_terms(R.tables(), xs)
        got = R.prior32(R.tables(), xs).astype(np.float64).mean(1) / R.LN2_32
        assert np.all(np.abs(got - ref.numpy()) <= bound.numpy() / 2), ci


@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=R.CASE_IDS)
def test_chain_restatement_within_half_the_bounds(ci):
    tab = R.tables()
    n, B, _ = R.CASES[ci]
    for mean in R.MEANS:
        em = mean == "EPSILON"
        for var in (None,) + R.VARS:
            for quant in (False, True):
                t, xs, xt, noise, mo = R.case_inputs(ci, mean, var, quant)
                m, v = mo[:, :n], (mo[:, n:] if var else None)
                s = None
                if quant:
                    x0 = R._x0(R.N32, R.rows_at(R.N32, tab, t), xt, m, em)
                    s = torch.quantile(torch.from_numpy(np.abs(x0)), 0.9, dim=1).clamp(min=1.0).numpy()
                    assert np.all(s[t == 0] < 1.0 + 1e-6) and (n < 255 or np.all(s[t != 0] > 1.0))
                o = R.vlb_terms(tab, t, xs, xt, m, v, em, var, s, noise)
                e, n32, eb, reg = o["elements"], o["n32"], o["elem_bound"], o["regime"]
                assert (reg == R.BETWEEN).mean() <= 0.05, (mean, var, quant)
                ok = reg == R.BOUNDED
                _ratio("vlb_kl", n32["kl"] - _np(e["kl"]), eb["kl"], R.K["vlb_kl"])
                _ratio("vlb_nll", (n32["nll"] - _np(e["nll"]))[ok], _np(eb["nll"])[ok], R.K["vlb_nll"])
                _ratio("sq", n32["dx2"] - _np(e["dx2"]), eb["dx2"], R.K["sq"])
                _ratio("sq", n32["de2"] - _np(e["de2"]), eb["de2"], R.K["sq"])
                assert np.all(n32["nll"][reg == R.SATURATED] == -R.LOG_CLAMP32)
                if n >= 16 and not quant:
                    assert (reg == R.SATURATED).any()
                if var is None and not quant and not em:                # the operands of the per-sample MSE tests: within 4 u
                    ref = ((xs.astype(np.float64) - mo.astype(np.float64)) ** 2).mean(1)
                    assert np.all(np.abs(R.mse32(xs, mo) - ref) <= 4 * R.U * ref)
                if var is None or quant:
                    continue
                tg = noise if em else xs
                scale = 0.02 if ci % 2 else None
                for which in (1, 3):
                    g = R.upstream(B, which)
                    h = R.hybrid_loss(tab, t, xs, xt, tg, mo, em, var, scale, *g)
                    h32 = R.hybrid32(tab, t, xs, xt, tg, mo, em, var, scale, *g)
                    for name in ("mse", "vb", "loss"):
                        assert np.all(np.abs(h32[name] - h[name].numpy()) <= h[name + "_bound"].numpy() / 2), (name, mean, var)
                    gv, gv32, gb = h["grad"][:, n:].numpy(), h32["grad"][:, n:], h["grad_v_bound"].numpy()
                    t0 = np.broadcast_to(h["t0"], gv.shape)
                    if (t0 & ok).any():
                        _ratio("g_nll", (gv32 - gv)[t0 & ok], gb[t0 & ok], R.K["g_nll"])
                    if (~t0).any():
                        _ratio("g_kl", (gv32 - gv)[~t0], gb[~t0], R.K["g_kl"])
                    sat = t0 & (reg == R.SATURATED)
                    assert np.all(gv[sat] == 0) and np.all(gv32[sat] == 0)
                    assert np.all(np.abs(h32["grad"][:, :n] - h["grad"][:, :n].numpy()) <= 4 * R.U * np.abs(h["grad"][:, :n].numpy()))
    print("worst ratios so far", {k: round(v, 2) for k, v in WORST.items()})
