"""CPU only: what tests/gd_step_ref.py claims, checked before test_gpu_gaussian_step_edges.py relies on it (-s prints the ratios).

  * N32 against T64 on every input set of the GPU module.  The bit-exact quantities lie within E64's running-error bound (the
    operation-by-operation form of k u sum |terms|).  The quantities behind expf lie within the bound taken with expf at 2 u instead of
    the device's 4 u: the arithmetic part in full and half of the expf allowance (N32's exp is correctly rounded, 1 u).  Half of the
    WHOLE bound holds only where the expf allowance is all of it (variance of LEARNED: 0.25, asserted); where the float32 rounding of
    the argument dominates (a LEARNED_RANGE log-variance of magnitude ~10, the products of the mean) N32 itself uses 0.62 (variance of
    LEARNED_RANGE) and 0.71 / 0.55 (out with the noise and grad terms, LEARNED / LEARNED_RANGE) of the whole bound, as any float32
    evaluation of those expressions may: these ratios are printed and held to 1.
  * The bit comparisons have power: a contracted restatement (a*x +- b*y in float64, rounded once) differs from N32 in bits at every
    case with n >= 255, and each wrong kernel of gd_step_ref.MUTATIONS is told from the right one at every second-trip and stride case.
  * The second-trip shapes make a second trip, and every mode occurs at every size."""
import numpy as np
import pytest
import torch

import gd_step_ref as S
from gd_step_ref import E64, N32, T64

f32 = np.float32
WORST = {}
LV = (S.LEARNED, S.LEARNED_RANGE)
SMALL = 10000                        # elements: what concerns the arithmetic, not the size, runs at the cases up to here


def _held(key, n32, e, shape, limit=1.0):
    v, b = S.value(E64, e, shape)
    r = S.err_ratio(S.value(N32, n32, shape), v, b)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= limit, (key, r)
    return v, b


def _bits_differ(a, b, shape):
    a, b = S.value(N32, a, shape), S.value(N32, b, shape)
    return not np.array_equal(a.view(np.int32), b.view(np.int32))


def _xm(B, n):
    d = S.step_inputs(B, n)
    return d, d["xt"], d["m"]


# ---------------------------------------------------------------------------------------------------------------- N32 against T64
@pytest.mark.parametrize("B,n", S.GRID_CASES, ids=S.ids(S.GRID_CASES))
def test_n32_within_the_bounds_of_t64_grid_kernels(B, n):
    d, xt, m = _xm(B, n)
    t = S.t_of(B, n)
    for op, (ra, rb) in enumerate(S.AFFINE_ROWS):
        a = S.affine(N32, S.table(), t, xt, m, ra, rb, op)
        v, _ = _held(f"affine {S.AFFINE_OPS[op]}", a, S.affine(E64, S.table(), t, xt, m, ra, rb, op), (B, n))
        if B * n <= SMALL:                                               # E64 carries T64's value
            assert torch.equal(v, S.value(T64, S.affine(T64, S.table(), t, xt, m, ra, rb, op), (B, n)))
    with S.expf_allowance(2.0):
        for mode in S.posterior_modes(B, n):
            tab, t, em, kw = S.posterior_args(B, n, mode)
            a, e = S.posterior(N32, tab, t, xt, m, em, **kw), S.posterior(E64, tab, t, xt, m, em, **kw)
            for k in a:
                bounded = k == "variance" or (k == "out" and not S.exact_out(mode[4], kw["grad"], kw["noise"]))
                _held(f"posterior {k}" + (f" (expf, {mode[4]})" if bounded else ""), a[k], e[k], (B, n))
            if mode[4] == S.LEARNED:
                assert not _bits_differ(a["log_variance"], kw["v"], (B, n))
    with S.expf_allowance(4.0):                                          # the whole bound: half of it where expf is all of it
        for var in LV if B * n <= SMALL else ():
            mode = ("START_X", False, True, True, var)
            tab, t, em, kw = S.posterior_args(B, n, mode)
            a, e = S.posterior(N32, tab, t, xt, m, em, **kw), S.posterior(E64, tab, t, xt, m, em, **kw)
            _held(f"whole bound: variance {var}", a["variance"], e["variance"], (B, n), 0.5 if var == S.LEARNED else 1.0)
            _held(f"whole bound: out {var}", a["out"], e["out"], (B, n))
    for mode in S.ddim_modes(B, n):
        tab, t, em, kw = S.ddim_args(B, n, mode)
        a, e = S.ddim(N32, tab, t, xt, m, em, **kw), S.ddim(E64, tab, t, xt, m, em, **kw)
        for k in a:
            _held(f"ddim {k}", a[k], e[k], (B, n))
    print("worst N32 error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("B,n", S.FLAT_CASES, ids=S.ids(S.FLAT_CASES))
def test_n32_within_the_bounds_of_t64_flat_kernels(B, n):
    d, xt, m = _xm(B, n)
    for mode in S.uniform_modes(B, n):
        quant, noise, coef = S.uniform_args(B, n, mode)
        a, e = S.ddim_uniform(N32, xt, m, quant, noise, coef), S.ddim_uniform(E64, xt, m, quant, noise, coef)
        for k in a:
            _held(f"ddim_uniform {k}", a[k], e[k], (B, n))
    assert len(set(S.uniform_args(B, n, S.uniform_modes(B, n)[0])[0].tolist())) == B                        # a quantile per sample
    for mode in S.sched_modes(B, n):
        args = S.sched_args(B, n, mode)
        a, e, r = S.sched_step(N32, xt, m, *args), S.sched_step(E64, xt, m, *args), S.sched_step(T64, xt, m, *args)
        for k in a:
            v, _ = _held(f"sched_step {k}", a[k], e[k], (B, n))
            assert torch.equal(v, S.value(T64, r[k], (B, n))) and np.isfinite(S.value(N32, a[k], (B, n))).all()
        if args[3] == 0.0 and args[1]:                                   # sqrt_alpha_prod == 0: +-inf clamped to +-clip
            assert set(np.unique(S.value(N32, a["pred_xstart"], (B, n))).tolist()) <= {-S.SCHED_CLIP, S.SCHED_CLIP}
    assert S.sched_coefficients(S.SCHED_T - 1)[1] == 0.0
    print("worst N32 error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("bad", [-1, S.T])
def test_n32_within_the_bounds_of_t64_with_a_t_outside_the_table(bad):
    """the input sets of the err_flag test: the clamped row, the mask from the raw t"""
    B, n = S.MODE_SHAPE
    d, xt, m = _xm(B, n)
    t = S.t_of(B, n)
    t[1] = bad
    r = S.step_rows(N32, S.table(), t)
    assert not r["t0"][1] and float(r["nmask"][1]) == 1.0
    assert float(r["coef1"][1]) == float(S.table()[2, 0 if bad < 0 else S.T - 1])
    with S.expf_allowance(2.0):
        for mode in S.posterior_modes(B, n)[::5]:
            tab, _, em, kw = S.posterior_args(B, n, mode, t=t)
            a, e = S.posterior(N32, tab, t, xt, m, em, **kw), S.posterior(E64, tab, t, xt, m, em, **kw)
            for k in a:
                _held(f"posterior {k}, t outside", a[k], e[k], (B, n))
    for mode in S.ddim_modes(B, n)[::5]:
        tab, _, em, kw = S.ddim_args(B, n, mode, t=t)
        a, e = S.ddim(N32, tab, t, xt, m, em, **kw), S.ddim(E64, tab, t, xt, m, em, **kw)
        for k in a:
            _held(f"ddim {k}, t outside", a[k], e[k], (B, n))


# ---------------------------------------------------------------------------------------------------------------- contraction
@pytest.mark.parametrize("B,n", [c for c in S.GRID_CASES if c[1] >= 255], ids=S.ids([c for c in S.GRID_CASES if c[1] >= 255]))
def test_a_contracted_restatement_differs_in_bits_grid_kernels(B, n):
    d, xt, m = _xm(B, n)
    t, tab = S.t_of(B, n), S.table()
    for op in (1, 2, 3):
        ra, rb = S.AFFINE_ROWS[op]
        assert _bits_differ(S.affine(N32, tab, t, xt, m, ra, rb, op), S.affine(N32, tab, t, xt, m, ra, rb, op, fma=True), (B, n)), op
    for var in (S.FIXED_LARGE, S.FIXED_SMALL):
        a, c = (S.posterior(N32, S.table(var), t, xt, m, False, var=var, grad=d["grad"], fma=f) for f in (False, True))
        assert _bits_differ(a["out"], c["out"], (B, n)) and not _bits_differ(a["pred_xstart"], c["pred_xstart"], (B, n))
    a, c = (S.posterior(N32, tab, t, xt, m, True, fma=f) for f in (False, True))
    assert _bits_differ(a["pred_xstart"], c["pred_xstart"], (B, n))
    for kw in (dict(eta=0.0), dict(eta=0.5, noise=d["noise"]), dict(reverse=True)):
        a, c = (S.ddim(N32, tab, t, xt, m, False, fma=f, **kw) for f in (False, True))
        assert _bits_differ(a["sample"], c["sample"], (B, n)), kw
    a, c = (S.ddim(N32, tab, t, xt, m, True, fma=f) for f in (False, True))
    assert _bits_differ(a["pred_xstart"], c["pred_xstart"], (B, n))


@pytest.mark.parametrize("B,n", [c for c in S.FLAT_CASES if c[1] >= 255], ids=S.ids([c for c in S.FLAT_CASES if c[1] >= 255]))
def test_a_contracted_restatement_differs_in_bits_flat_kernels(B, n):
    d, xt, m = _xm(B, n)
    quant, noise, coef = S.uniform_args(B, n, (10, 0.5, True))
    a, c = (S.ddim_uniform(N32, xt, m, quant, noise, coef, fma=f) for f in (False, True))
    assert _bits_differ(a["sample"], c["sample"], (B, n))
    for mode in ((57, True, 0.0, True), (57, False, S.SCHED_CLIP, True)):
        a, c = (S.sched_step(N32, xt, m, *S.sched_args(B, n, mode), fma=f) for f in (False, True))
        assert _bits_differ(a["sample"], c["sample"], (B, n)), mode
        assert _bits_differ(a["pred_xstart"], c["pred_xstart"], (B, n)) == mode[1], mode


# ---------------------------------------------------------------------------------------------------------------- mutations
def _violates(mut, e, shape):
    """the mutated float32 result leaves the whole E64 bound somewhere"""
    v, b = S.value(E64, e, shape)
    err = (torch.from_numpy(S.value(N32, mut, shape).astype(np.float64)) - v).abs()
    return bool((~(err <= b)).any())


@pytest.mark.parametrize("B,n", S.GRID_TRIP2 + (S.STRIDE_SHAPE,), ids=S.ids(S.GRID_TRIP2 + (S.STRIDE_SHAPE,)))
def test_every_mutation_is_detected_grid_kernels(B, n):
    d, xt, m = _xm(B, n)
    t, tab = S.t_of(B, n), S.table()
    t_err = t.copy()
    t_err[1] = -1                                                        # clamped to row 0, the mask stays off
    seen = set()

    def post(mut, what, t_=t, bound=False, **kw):
        em, tb = kw.pop("em", False), S.table(kw.get("var"))
        a, c = (S.posterior(N32, tb, t_, xt, m, em, mut=mu, **kw) for mu in (None, mut))
        if bound:
            e = S.posterior(E64, tb, t_, xt, m, em, **kw)
            assert not _violates(a[what], e[what], (B, n)) and _violates(c[what], e[what], (B, n)), (mut, what)
        else:
            assert _bits_differ(a[what], c[what], (B, n)), (mut, what)
        seen.add(mut)

    def dd(mut, what="sample", t_=t, **kw):
        a, c = (S.ddim(N32, tab, t_, xt, m, False, mut=mu, **kw) for mu in (None, mut))
        assert _bits_differ(a[what], c[what], (B, n)), (mut, kw)
        seen.add(mut)

    quant = S.quantile_of(tab, t, xt, m, False)
    assert float(quant.max()) > 1.0 > float(quant.min())
    dd("swap_abar", eta=0.5, noise=d["noise"])
    dd("swap_abar", reverse=True)
    post("swap_coef", "out")
    post("swap_coef", "out", var=S.FIXED_SMALL, grad=d["grad"])
    for op in (1, 2, 3):
        ra, rb = S.AFFINE_ROWS[op]
        for mut in ("swap_coef", "row_b1"):
            assert _bits_differ(S.affine(N32, tab, t, xt, m, ra, rb, op), S.affine(N32, tab, t, xt, m, ra, rb, op, mut=mut), (B, n)), (op, mut)
    assert _bits_differ(S.affine(N32, tab, t, xt, m, "sqrt_abar", None, 0), S.affine(N32, tab, t, xt, m, "sqrt_abar", None, 0, mut="row_b1"), (B, n))
    post("row_b1", "out")
    post("row_b1", "pred_xstart", em=True)
    post("row_b1", "log_variance", var=S.LEARNED_RANGE, v=d[S.LEARNED_RANGE])
    dd("row_b1")
    dd("row_b1", reverse=True)
    post("mask_clamped", "out", t_=t_err, bound=True, noise=d["noise"])
    post("mask_clamped", "out", t_=t_err, bound=True, noise=d["noise"], var=S.LEARNED, v=d[S.LEARNED])
    a, c = (S.ddim(N32, tab, t_err, xt, m, False, eta=0.5, noise=d["noise"], mut=mu) for mu in (None, "mask_clamped"))
    assert not _bits_differ(a["sample"], c["sample"], (B, n))            # DDIM cannot tell: row 0 has sigma == 0 whatever the mask
    post("div_first", "pred_xstart", quant=quant)
    dd("div_first", "pred_xstart", quant=quant)
    post("grad_half", "out", bound=True, var=S.LEARNED, v=d[S.LEARNED], grad=d["grad"])
    post("grad_half", "out", bound=True, var=S.LEARNED_RANGE, v=d[S.LEARNED_RANGE], grad=d["grad"])
    # the variance half of one [B, 2, n] buffer read at b * n past its base instead of b * 2n
    for var in LV:
        flat = S.merged(m, d[var]).reshape(-1)
        wrong = np.stack([flat[n + b * n: 2 * n + b * n] for b in range(B)])
        a, c = (S.posterior(N32, tab, t, xt, m, False, var=var, v=v) for v in (d[var], wrong))
        assert _bits_differ(a["log_variance"], c["log_variance"], (B, n))
        e = S.posterior(E64, tab, t, xt, m, False, var=var, v=d[var])
        assert not _violates(a["variance"], e["variance"], (B, n)) and _violates(c["variance"], e["variance"], (B, n))
    seen.add("var_stride_n")
    assert seen == set(S.MUTATIONS)


@pytest.mark.parametrize("B,n", S.FLAT_TRIP2, ids=S.ids(S.FLAT_TRIP2))
def test_every_applicable_mutation_is_detected_flat_kernels(B, n):
    """the flat kernels read no table and no variance: a sample's quantile, the threshold and the two coefficients can go wrong"""
    d, xt, m = _xm(B, n)
    quant, noise, coef = S.uniform_args(B, n, (10, 0.5, True))
    a = S.ddim_uniform(N32, xt, m, quant, noise, coef)
    for mut in ("row_b1", "div_first"):
        c = S.ddim_uniform(N32, xt, m, quant, noise, coef, mut=mut)
        assert _bits_differ(a["sample"], c["sample"], (B, n)) and _bits_differ(a["pred_xstart"], c["pred_xstart"], (B, n)), mut
    for mode in S.sched_modes(B, n)[:3]:
        a, c = (S.sched_step(N32, xt, m, *S.sched_args(B, n, mode), mut=mu) for mu in (None, "swap_coef"))
        assert _bits_differ(a["sample"], c["sample"], (B, n)), mode


# ---------------------------------------------------------------------------------------------------------------- trips, coverage
def test_the_second_trip_shapes_make_a_second_trip():
    assert [S.gd_chunks(B, n) for B, n in S.GRID_TRIP2] == [7, 1]
    for B, n in S.GRID_TRIP2:
        assert S.gd_chunks(B, n) * S.GD_THREADS < n
    assert 1801 - 7 * 256 == 9 and -(-700 // 256) == 3
    for B, n in S.GRID_SMALL:
        assert S.gd_chunks(B, n) * S.GD_THREADS >= n
    for B, n in S.FLAT_TRIP2:
        assert B * n > S.FLAT_GRID * S.GD_THREADS and S.flat_grid(B * n) == S.FLAT_GRID
        first = np.arange(B * n - S.FLAT_GRID * S.GD_THREADS)             # the threads that make a second trip: their first element
        assert np.all(first // n != (first + S.FLAT_GRID * S.GD_THREADS) // n)   # i / per_sample is another sample's there
    for B, n in S.FLAT_SMALL:
        assert S.flat_grid(B * n) * S.GD_THREADS >= B * n
    assert S.GRID_LIMIT[0] == 65535 and sorted(set(S.t_of(*S.GRID_TRIP2[0]).tolist())) == list(range(S.T))
    assert S.STRIDE_SHAPE[1] % 4 == 1


def test_every_mode_occurs_at_every_size():
    for B, n in S.GRID_CASES:
        pm = S.posterior_modes(B, n)
        assert {md[0] for md in pm} == set(S.MEANS) and {md[4] for md in pm} == set(S.VARS), (B, n)
        assert all({md[k] for md in pm} == {False, True} for k in (1, 2, 3)), (B, n)
        dm = S.ddim_modes(B, n)
        fw = [md for md in dm if not md[5]]
        assert {md[0] for md in fw} == set(S.MEANS) and {(md[3], md[4]) for md in fw} == set(S.ETAS), (B, n)
        assert all({md[k] for md in fw} == {False, True} for k in (1, 2)) and any(md[5] for md in dm), (B, n)
        assert all(not (md[5] and (md[2] or md[4] or md[3] != 0.0)) for md in dm)
    assert len(set(S.posterior_modes(*S.MODE_SHAPE))) == 64 and len(set(S.ddim_modes(*S.MODE_SHAPE))) == 28
    rev = [md for md in S.ddim_modes(*S.MODE_SHAPE) if md[5]]
    assert {(md[0], md[1]) for md in rev} == {(a, q) for a in S.MEANS for q in (False, True)}
    for B, n in S.FLAT_CASES:
        um, sm = S.uniform_modes(B, n), S.sched_modes(B, n)
        assert {S.uniform_args(B, n, md)[1] is None for md in um} == {False, True} and {md[2] for md in um} == {False, True}
        assert {md[1] for md in sm} == {False, True} and {md[2] > 0 for md in sm} == {False, True}
        assert {S.sched_args(B, n, md)[0] is None for md in sm} == {False, True}
        assert any(md[1] and S.sched_args(B, n, md)[3] == 0.0 for md in sm)
    assert S.MODE_SHAPE in S.GRID_CASES and set(S.GRID_TRIP2) <= set(S.GRID_CASES) and S.GRID_LIMIT in S.GRID_CASES
