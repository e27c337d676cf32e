"""-m gpu: the step side of csrc/gaussian.hip (rho_gd_affine, rho_gd_posterior_step, rho_gd_posterior_step_lv, rho_gd_ddim_step,
rho_gd_ddim_step_strided) and the two older step kernels of csrc/select.hip (rho_ddim_step, rho_ddpm_sched_step) through the C ABI,
against tests/gd_step_ref.py (its docstring has the arithmetics and the bounds; test_gd_step_ref_host.py shows on the CPU that the
chosen inputs notice a contracted product-sum and each wrong kernel).

Every call writes NaN-prefilled outputs between sentinels (gpu_util.Guarded); the sentinels survive and the inputs come back unchanged.
What has no transcendental is compared bit for bit with the float32 restatement N32; what lies behind expf (``out`` with the noise term
or exp(logvar) * grad, ``variance``) per element against float64 with the derived bound.  Sizes: per-sample sizes below, at and past a
workgroup with B = 3 and 1; (300, 1801) and (2049, 700), where the (chunks, batch) grid loops again; batch = 65535, the gridDim.y
limit; for the flat kernels (3, 349551), past 4096 * 256 elements.  Every mode combination runs at (3, 257), a rotating subset
elsewhere.  Then strides, optional outputs, offset bases, err_flag, refusals and the wrappers' checks.  -s prints the worst error /
bound per bounded quantity."""
import functools

import numpy as np
import pytest
import torch

import gd_step_ref as S
from gd_step_ref import E64, N32
from gpu_util import DEV, Guarded, check_bound, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
WORST = {}
E_ARG, E_SHAPE = -1, -3
MT = {"START_X": 0, "EPSILON": 1}
VT = {S.LEARNED: 0, S.LEARNED_RANGE: 1}
LV = (S.LEARNED, S.LEARNED_RANGE)
T = S.T
P_OUTS = ("out", "pred_xstart", "variance", "log_variance")


def _lib():
    from rho_diffusion_amd import hip
    return hip.lib(), hip.stream()


@functools.lru_cache(maxsize=None)
def _tab(var=None):
    return torch.from_numpy(S.table(var)).to(DEV)


class Ins:
    """named inputs on the device, each between sentinels, ``shifts[name]`` elements off 16-byte alignment"""

    def __init__(self, shifts=None, **arrays):
        shifts = shifts or {}
        self.src = {k: torch.from_numpy(np.array(a)).reshape(-1) for k, a in arrays.items() if a is not None}
        self.g = {k: Guarded(v, shift=shifts.get(k, 0)) for k, v in self.src.items()}

    def p(self, k, offset=0):
        return self.g[k].ptr + offset * self.g[k].v.element_size() if k in self.g else None

    def unchanged(self):
        same = lambda a, b: same_bits(a, b) if b.dtype == torch.float32 else torch.equal(a, b)        # noqa: E731  (NaN padding: bits)
        return all(g.intact() and same(g.cpu(), self.src[k]) for k, g in self.g.items())


def _case_ins(B, n, t=None, shifts=None, **extra):
    d = S.step_inputs(B, n)
    return Ins(shifts, xt=d["xt"], m=d["m"], grad=d["grad"], noise=d["noise"], t=S.t_of(B, n) if t is None else t,
               **{S.LEARNED: d[S.LEARNED], S.LEARNED_RANGE: d[S.LEARNED_RANGE]}, **extra)


def _outs(names, size, shift=0):
    return {k: Guarded(size, shift=shift) for k in names}


def _ptr(o, k):
    return o[k].ptr if k in o else None


def _sync_ok(rc, outs, what):
    assert rc == 0, what
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()), what


def _bits(g, want, what):
    assert same_bits(g.cpu(), torch.from_numpy(np.array(want)).reshape(-1)), what


def _bound(key, g, e, shape, what):
    v, b = S.value(E64, e, shape)
    got = g.cpu().double()
    WORST[key] = max(WORST.get(key, 0.0), S.err_ratio(got.numpy(), v, b))
    check_bound(got, v, b, (key, what))


def _untouched(outs):
    torch.cuda.synchronize()
    return all(g.intact() and bool(torch.isnan(g.v).all()) for g in outs.values())


def _report():
    print("worst GPU error / bound:", {k: round(v, 3) for k, v in sorted(WORST.items())})


# ---------------------------------------------------------------------------------------------------------------- the raw calls
def affine_call(ins, B, n, op, row_a, row_b, flag=None, out_shift=0, y="m"):
    from rho_diffusion_amd.engine.ops import GD_ROW
    L, st = _lib()
    o = _outs(("out",), B * n, out_shift)
    rc = L.rho_gd_affine(ins.p("xt"), ins.p(y) if op else None, o["out"].ptr, ins.p("t"), _tab().data_ptr(), T, GD_ROW[row_a],
                         GD_ROW[row_b] if row_b else 0, op, B, n, flag, st)
    _sync_ok(rc, o, ("affine", B, n, op))
    return o["out"]


def posterior_call(ins, B, n, mode, quant=None, names=P_OUTS, flag=None, out_shift=0, m=None, v=None, ms=None, vs=None):
    """rho_gd_posterior_step / _lv of one mode (mean, quant, grad, noise, var); ``m`` / ``v`` (pointer, stride) override the operands"""
    L, st = _lib()
    mean, _, g, z, var = mode
    lv = var in LV
    o = _outs([k for k in names if lv or k in ("out", "pred_xstart")], B * n, out_shift)
    q = None if quant is None else quant.p("q")
    common = (ins.p("t"), _tab(var).data_ptr(), T, MT[mean])
    tail = (q, ins.p("grad") if g else None, ins.p("noise") if z else None)
    if lv:
        rc = L.rho_gd_posterior_step_lv(ins.p("xt"), ins.p("m") if m is None else m, ms or n, ins.p(var) if v is None else v, vs or n, *common,
                                        VT[var], *tail, _ptr(o, "out"), _ptr(o, "pred_xstart"), _ptr(o, "variance"), _ptr(o, "log_variance"),
                                        B, n, flag, st)
    else:
        rc = L.rho_gd_posterior_step(ins.p("xt"), ins.p("m"), *common, *tail, o["out"].ptr, _ptr(o, "pred_xstart"), B, n, flag, st)
    _sync_ok(rc, o, ("posterior", B, n, mode))
    return o


def ddim_call(ins, B, n, mode, quant=None, names=("sample", "pred_xstart"), flag=None, out_shift=0, m=None, stride=None):
    """rho_gd_ddim_step, or _strided where ``stride`` is given, of one mode (mean, quant, grad, eta, noise, reverse)"""
    L, st = _lib()
    mean, _, g, eta, z, rev = mode
    o = _outs(names, B * n, out_shift)
    q = None if quant is None else quant.p("q")
    tail = (ins.p("t"), _tab().data_ptr(), T, MT[mean], q, ins.p("grad") if g else None, ins.p("noise") if z else None, float(eta), int(rev),
            o["sample"].ptr, _ptr(o, "pred_xstart"), B, n, flag, st)
    mp = ins.p("m") if m is None else m
    rc = L.rho_gd_ddim_step(ins.p("xt"), mp, *tail) if stride is None else L.rho_gd_ddim_step_strided(ins.p("xt"), mp, stride, *tail)
    _sync_ok(rc, o, ("ddim", B, n, mode))
    return o


def _quant(q):
    return None if q is None else Ins(q=q)


def check_posterior(B, n, mode, o, kw, tab, t, em, what):
    d = S.step_inputs(B, n)
    var = mode[4]
    a = S.posterior(N32, tab, t, d["xt"], d["m"], em, **kw)
    exact = S.exact_out(var, kw["grad"], kw["noise"])
    e = S.posterior(E64, tab, t, d["xt"], d["m"], em, **kw) if ("variance" in o or ("out" in o and not exact)) else None
    for k, g in o.items():
        if k == "variance" or (k == "out" and not exact):
            _bound(f"posterior {k}" + (f" {var}" if var in LV else " fixed"), g, e[k], (B, n), what)
        else:
            _bits(g, S.value(N32, a[k], (B, n)), (what, k))
    if "log_variance" in o and e is not None:                            # also inside its bound; LEARNED: the input itself
        _bound(f"posterior log_variance {var}", o["log_variance"], e["log_variance"], (B, n), what)
        if var == S.LEARNED:
            _bits(o["log_variance"], d[var], (what, "log_variance is the input"))


# ---------------------------------------------------------------------------------------------------------------- sizes and modes
@pytest.mark.parametrize("B,n", S.GRID_CASES, ids=S.ids(S.GRID_CASES))
def test_affine_every_op_at_every_size(B, n):
    ins, d, t = _case_ins(B, n), S.step_inputs(B, n), S.t_of(B, n)
    for op, (ra, rb) in enumerate(S.AFFINE_ROWS):
        _bits(affine_call(ins, B, n, op, ra, rb), S.value(N32, S.affine(N32, S.table(), t, d["xt"], d["m"], ra, rb, op), (B, n)), (B, n, op))
    assert ins.unchanged()


@pytest.mark.parametrize("B,n", S.GRID_CASES, ids=S.ids(S.GRID_CASES))
def test_posterior_step_sizes_and_modes(B, n):
    ins = _case_ins(B, n)
    for mode in S.posterior_modes(B, n):
        tab, t, em, kw = S.posterior_args(B, n, mode)
        q = _quant(kw["quant"])
        o = posterior_call(ins, B, n, mode, q)
        check_posterior(B, n, mode, o, kw, tab, t, em, (B, n, mode))
        assert q is None or q.unchanged()
    assert ins.unchanged()
    _report()


@pytest.mark.parametrize("B,n", S.GRID_CASES, ids=S.ids(S.GRID_CASES))
def test_ddim_step_sizes_and_modes(B, n):
    ins, d = _case_ins(B, n), S.step_inputs(B, n)
    for mode in S.ddim_modes(B, n):
        tab, t, em, kw = S.ddim_args(B, n, mode)
        q = _quant(kw["quant"])
        o = ddim_call(ins, B, n, mode, q)
        a = S.ddim(N32, tab, t, d["xt"], d["m"], em, **kw)
        for k in o:
            _bits(o[k], S.value(N32, a[k], (B, n)), (B, n, mode, k))
        assert q is None or q.unchanged()
    assert ins.unchanged()


def uniform_call(ins, B, n, quant, noise, coef, pred=True, out_shift=0):
    L, st = _lib()
    o = _outs(("sample", "pred_xstart") if pred else ("sample",), B * n, out_shift)
    rc = L.rho_ddim_step(ins.p("xt"), ins.p("m"), quant.p("q"), ins.p("noise") if noise is not None else None, o["sample"].ptr,
                         _ptr(o, "pred_xstart"), B, n, *[float(c) for c in coef], st)
    _sync_ok(rc, o, ("ddim_uniform", B, n, coef))
    return o


def sched_call(ins, B, n, args, pred=True, out_shift=0):
    L, st = _lib()
    noise, em, sb, sa, clip, c0, c1, sigma = args
    o = _outs(("sample", "pred_xstart") if pred else ("sample",), B * n, out_shift)
    rc = L.rho_ddpm_sched_step(ins.p("xt"), ins.p("m"), ins.p("noise") if noise is not None else None, o["sample"].ptr, _ptr(o, "pred_xstart"),
                               B * n, int(em), float(sb), float(sa), float(clip), float(c0), float(c1), float(sigma), st)
    _sync_ok(rc, o, ("sched_step", B, n, args[1:]))
    return o


@pytest.mark.parametrize("B,n", S.FLAT_CASES, ids=S.ids(S.FLAT_CASES))
def test_flat_kernels_sizes_and_modes(B, n):
    ins, d = _case_ins(B, n), S.step_inputs(B, n)
    for mode in S.uniform_modes(B, n):
        quant, noise, coef = S.uniform_args(B, n, mode)
        q = _quant(quant)
        o = uniform_call(ins, B, n, q, noise, coef, mode[2])
        a = S.ddim_uniform(N32, d["xt"], d["m"], quant, noise, coef)
        for k in o:
            _bits(o[k], S.value(N32, a[k], (B, n)), ("ddim_uniform", B, n, mode, k))
        assert q.unchanged()
    for i, mode in enumerate(S.sched_modes(B, n)):
        args = S.sched_args(B, n, mode)
        o = sched_call(ins, B, n, args, i % 2 == 0)
        a = S.sched_step(N32, d["xt"], d["m"], *args)
        for k in o:
            _bits(o[k], S.value(N32, a[k], (B, n)), ("sched_step", B, n, mode, k))
            assert bool(torch.isfinite(o[k].v).all()), mode
    assert ins.unchanged()


# ---------------------------------------------------------------------------------------------------------------- strides
def test_strided_halves_read_in_place_give_the_bits_of_contiguous_copies():
    """_lv and ddim_step_strided on the two halves of one [B, 2, n] buffer (stride 2n; n = 1029 is odd, so every second row is off
    16 bytes), then on rows 2n + 5 apart with NaN in the padding; for DDIM also with NaN in the whole variance half"""
    B, n = S.STRIDE_SHAPE
    d = S.step_inputs(B, n)
    ins = _case_ins(B, n)
    quant = {em: _quant(S.quantile_of(S.table(), S.t_of(B, n), d["xt"], d["m"], em)) for em in (False, True)}
    for var in LV:
        for pad in (0, 5):
            row = 2 * n + pad
            buf = np.full((B, row), np.nan, dtype=f32)
            buf[:, :n], buf[:, n:2 * n] = d["m"], d[var]
            dbuf = np.full((B, row), np.nan, dtype=f32)
            dbuf[:, :n] = d["m"]
            mo = Ins(both=buf, mean_only=dbuf)
            for mode in (("EPSILON", True, True, True, var), ("START_X", False, False, True, var), ("START_X", True, True, False, var)):
                q = quant[mode[0] == "EPSILON"] if mode[1] else None
                want = posterior_call(ins, B, n, mode, q)
                got = posterior_call(ins, B, n, mode, q, m=mo.p("both"), v=mo.p("both", n), ms=row, vs=row)
                for k in want:
                    assert bool(torch.isfinite(got[k].v).all()) and same_bits(got[k].v, want[k].v), (var, pad, mode, k)
            for mode in (("EPSILON", True, True, 0.5, True, False), ("START_X", False, False, 0.0, False, False),
                         ("START_X", True, False, 0.0, False, True)):
                q = quant[mode[0] == "EPSILON"] if mode[1] else None
                want = ddim_call(ins, B, n, mode, q)
                for src in ("both", "mean_only"):
                    got = ddim_call(ins, B, n, mode, q, m=mo.p(src), stride=row)
                    for k in want:
                        assert bool(torch.isfinite(got[k].v).all()) and same_bits(got[k].v, want[k].v), (var, pad, mode, src, k)
            assert mo.unchanged()
    assert ins.unchanged()


# ---------------------------------------------------------------------------------------------------------------- optional outputs
@pytest.mark.parametrize("var", LV)
def test_lv_each_output_alone_gives_the_bits_of_the_all_outputs_call(var):
    B, n = S.MODE_SHAPE
    ins = _case_ins(B, n)
    mode = ("EPSILON", True, True, True, var)
    tab, t, em, kw = S.posterior_args(B, n, mode)
    q = _quant(kw["quant"])
    full = posterior_call(ins, B, n, mode, q)
    check_posterior(B, n, mode, full, kw, tab, t, em, ("all outputs", var))
    for k in P_OUTS:
        one = posterior_call(ins, B, n, mode, q, names=(k,))
        assert list(one) == [k] and same_bits(one[k].v, full[k].v), (var, k)
    L, st = _lib()
    rc = L.rho_gd_posterior_step_lv(ins.p("xt"), ins.p("m"), n, ins.p(var), n, ins.p("t"), _tab().data_ptr(), T, 1, VT[var], None, None, None,
                                    None, None, None, None, B, n, None, st)
    assert rc == E_ARG
    # the fixed-variance form: out is required, pred_xstart optional
    fmode = ("EPSILON", True, True, True, S.FIXED_SMALL)
    both, alone = posterior_call(ins, B, n, fmode, q), posterior_call(ins, B, n, fmode, q, names=("out",))
    assert same_bits(alone["out"].v, both["out"].v)
    dm = ("EPSILON", True, True, 0.5, True, False)
    assert same_bits(ddim_call(ins, B, n, dm, q, names=("sample",))["sample"].v, ddim_call(ins, B, n, dm, q)["sample"].v)
    assert ins.unchanged()
    _report()


# ---------------------------------------------------------------------------------------------------------------- offset bases
def test_each_operand_one_element_off_alignment_gives_the_bits_of_the_aligned_run():
    """The kernels are scalar today; this pins the behaviour before anyone vectorises them."""
    B, n = S.MODE_SHAPE
    d = S.step_inputs(B, n)
    pm, dm = ("EPSILON", True, True, True, S.LEARNED_RANGE), ("EPSILON", True, True, 0.5, True, False)
    fm = ("EPSILON", True, True, True, S.FIXED_LARGE)
    tab, t, em, kw = S.posterior_args(B, n, pm)
    uq, un, uc = S.uniform_args(B, n, (10, 0.5, True))
    sargs = S.sched_args(B, n, (57, True, S.SCHED_CLIP, True))

    def run(shifts, out_shift):
        ins = _case_ins(B, n, shifts=shifts)
        q, q2 = Ins(shifts, q=kw["quant"]), Ins(shifts, q=uq)
        r = {f"lv {k}": g for k, g in posterior_call(ins, B, n, pm, q, out_shift=out_shift).items()}
        r.update({f"fixed {k}": g for k, g in posterior_call(ins, B, n, fm, q, out_shift=out_shift).items()})
        r.update({f"ddim {k}": g for k, g in ddim_call(ins, B, n, dm, q, out_shift=out_shift).items()})
        r.update({f"uniform {k}": g for k, g in uniform_call(ins, B, n, q2, un, uc, out_shift=out_shift).items()})
        r.update({f"sched {k}": g for k, g in sched_call(ins, B, n, sargs, out_shift=out_shift).items()})
        for op, (ra, rb) in enumerate(S.AFFINE_ROWS):
            r[f"affine {op}"] = affine_call(ins, B, n, op, ra, rb, out_shift=out_shift)
        assert ins.unchanged() and q.unchanged() and q2.unchanged()
        return r

    want = run({}, 0)
    names = ("xt", "m", "grad", "noise", S.LEARNED_RANGE, "q", "t")
    every = [({k: 1}, 0) for k in names] + [({}, 1), ({k: 1 for k in names}, 1), ({k: 1 + i % 3 for i, k in enumerate(names)}, 3)]
    for shifts, out_shift in every:
        got = run(shifts, out_shift)
        for k in want:
            assert same_bits(got[k].v, want[k].v), (shifts, out_shift, k)


# ---------------------------------------------------------------------------------------------------------------- err_flag
@pytest.mark.parametrize("bad", [-1, T])
def test_err_flag_and_the_clamped_row(bad):
    """t[1] outside [0, T): the flag reads 4, sample 1 is the restatement at the clamped row with the mask from the raw t (for -1: row 0
    with the noise on), the other samples keep the bits of a valid run; a NULL flag passes; a valid run leaves the flag 0"""
    B, n = S.MODE_SHAPE
    d = S.step_inputs(B, n)
    t_ok = S.t_of(B, n)
    t_bad = t_ok.copy()
    t_bad[1] = bad
    ok, ins = _case_ins(B, n), _case_ins(B, n, t=t_bad)
    others = torch.tensor([0, 2])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def flagged(call, *a, **kw):
        flag.zero_()
        o = call(ok, *a, flag=flag.data_ptr(), **kw)
        assert int(flag.item()) == 0
        got = call(ins, *a, flag=flag.data_ptr(), **kw)
        assert int(flag.item()) == 4
        null = call(ins, *a, flag=None, **kw)
        o, got, null = ({"out": x} if isinstance(x, Guarded) else x for x in (o, got, null))
        for k in got:
            assert same_bits(null[k].v, got[k].v), k
            assert same_bits(got[k].v.view(B, n)[others], o[k].v.view(B, n)[others]), k
            if k in ("out", "sample"):                                   # (an x0 or a learned variance need not depend on the row)
                assert not same_bits(got[k].v.view(B, n)[1], o[k].v.view(B, n)[1]), k
        return got

    for op, (ra, rb) in enumerate(S.AFFINE_ROWS):
        got = flagged(affine_call, B, n, op, ra, rb)
        _bits(got["out"], S.value(N32, S.affine(N32, S.table(), t_bad, d["xt"], d["m"], ra, rb, op), (B, n)), (bad, op))
    for mode in (("EPSILON", False, False, False, S.FIXED_LARGE), ("EPSILON", False, True, True, S.FIXED_SMALL),
                 ("START_X", False, True, True, S.LEARNED), ("EPSILON", False, False, True, S.LEARNED_RANGE)):
        tab, _, em, kw = S.posterior_args(B, n, mode, t=t_bad)
        got = flagged(posterior_call, B, n, mode)
        check_posterior(B, n, mode, got, kw, tab, t_bad, em, (bad, mode))
        if bad == -1 and mode[3]:                                        # the noise is on: not what the mask of the clamped t would give
            off = S.posterior(N32, tab, t_bad, d["xt"], d["m"], em, **dict(kw, noise=None))
            assert not same_bits(got["out"].v.view(B, n)[1], torch.from_numpy(S.value(N32, off["out"], (B, n))[1].copy()))
    for mode in (("EPSILON", False, True, 0.5, True, False), ("START_X", False, False, 0.0, False, True)):
        tab, _, em, kw = S.ddim_args(B, n, mode, t=t_bad)
        got = flagged(ddim_call, B, n, mode)
        a = S.ddim(N32, tab, t_bad, d["xt"], d["m"], em, **kw)
        for k in got:
            _bits(got[k], S.value(N32, a[k], (B, n)), (bad, mode, k))
    assert ins.unchanged() and ok.unchanged()
    _report()


# ---------------------------------------------------------------------------------------------------------------- grid limit, refusals
def _refusal_fixture():
    B, n = 2, 8
    z = np.zeros(2 * B * n, f32)
    ins = Ins(xt=z, m=z, grad=z, noise=z, v=z, q=np.ones(B, f32), t=np.zeros(B, np.int64))
    outs = _outs(("a", "b", "c", "d"), 2 * B * n)
    return B, n, ins, outs


def test_batch_65535_runs_and_65536_is_refused():
    """batch = 65535 with n = 2: the first and the last sample are right (the whole result is compared in the size tests above);
    batch = 65536 returns RHO_E_SHAPE from all five grid entry points and writes nothing"""
    B, n = S.GRID_LIMIT
    ins, d, t = _case_ins(B, n), S.step_inputs(B, n), S.t_of(B, n)
    mode = ("EPSILON", False, True, False, S.FIXED_LARGE)
    tab, _, em, kw = S.posterior_args(B, n, mode)
    o = posterior_call(ins, B, n, mode)
    a = S.value(N32, S.posterior(N32, tab, t, d["xt"], d["m"], em, **kw)["out"], (B, n))
    got = o["out"].cpu().view(B, n)
    assert same_bits(got[0], torch.from_numpy(a[0])) and same_bits(got[-1], torch.from_numpy(a[-1])) and t[0] != t[-1]
    L, st = _lib()
    _, n, r, outs = _refusal_fixture()
    p, o = r.p, [g.ptr for g in outs.values()]
    tb, B = _tab().data_ptr(), 65536
    assert L.rho_gd_affine(p("xt"), p("m"), o[0], p("t"), tb, T, 0, 1, 1, B, n, None, st) == E_SHAPE
    assert L.rho_gd_posterior_step(p("xt"), p("m"), p("t"), tb, T, 0, None, None, None, o[0], o[1], B, n, None, st) == E_SHAPE
    assert L.rho_gd_posterior_step_lv(p("xt"), p("m"), n, p("v"), n, p("t"), tb, T, 0, 0, None, None, None, *o, B, n, None, st) == E_SHAPE
    assert L.rho_gd_ddim_step(p("xt"), p("m"), p("t"), tb, T, 0, None, None, None, 0.0, 0, o[0], o[1], B, n, None, st) == E_SHAPE
    assert L.rho_gd_ddim_step_strided(p("xt"), p("m"), n, p("t"), tb, T, 0, None, None, None, 0.0, 0, o[0], o[1], B, n, None, st) == E_SHAPE
    assert _untouched(outs)


def test_refusals_return_their_codes_and_write_nothing():
    from rho_diffusion_amd.engine.ops import GD_ROWS
    L, st = _lib()
    B, n, r, outs = _refusal_fixture()
    p, o, tb = r.p, [g.ptr for g in outs.values()], _tab().data_ptr()
    X, M, V, TT, Q, G, Z = p("xt"), p("m"), p("v"), p("t"), p("q"), p("grad"), p("noise")

    def aff(x=X, y=M, out=o[0], t=TT, tab=tb, T_=T, ra=0, rb=1, op=1, B_=B, n_=n):
        return L.rho_gd_affine(x, y, out, t, tab, T_, ra, rb, op, B_, n_, None, st)

    def post(x=X, m=M, t=TT, tab=tb, T_=T, mt=0, out=o[0], B_=B, n_=n):
        return L.rho_gd_posterior_step(x, m, t, tab, T_, mt, Q, G, Z, out, o[1], B_, n_, None, st)

    def lv(x=X, m=M, ms=n, v=V, vs=n, t=TT, tab=tb, T_=T, mt=0, vt=0, outs_=tuple(o), B_=B, n_=n):
        return L.rho_gd_posterior_step_lv(x, m, ms, v, vs, t, tab, T_, mt, vt, Q, G, Z, *outs_, B_, n_, None, st)

    def dd(strided, x=X, m=M, stride=n, t=TT, tab=tb, T_=T, mt=0, g=None, z=None, eta=0.0, rev=0, sample=o[0], B_=B, n_=n):
        tail = (t, tab, T_, mt, Q, g, z, eta, rev, sample, o[1], B_, n_, None, st)
        return L.rho_gd_ddim_step_strided(x, m, stride, *tail) if strided else L.rho_gd_ddim_step(x, m, *tail)

    def uni(x=X, m=M, q=Q, z=Z, out=o[0], B_=B, n_=n, sigma=0.25):
        return L.rho_ddim_step(x, m, q, z, out, o[1], B_, n_, 1.5, 1.0, 0.75, 0.5, sigma, st)

    def sch(x=X, m=M, z=Z, out=o[0], n_=B * n, sigma=0.25):
        return L.rho_ddpm_sched_step(x, m, z, out, o[1], n_, 1, 0.5, 0.75, 1.0, 0.5, 0.5, sigma, st)

    R = len(GD_ROWS)
    arg = [aff(x=None), aff(out=None), aff(t=None), aff(tab=None), aff(y=None), aff(y=None, op=2), aff(y=None, op=3), aff(op=-1), aff(op=4),
           aff(ra=-1), aff(ra=R), aff(rb=-1), aff(rb=R), aff(op=0, ra=R), aff(B_=0), aff(n_=0), aff(T_=0), aff(B_=-1),
           post(x=None), post(m=None), post(t=None), post(tab=None), post(out=None), post(mt=2), post(mt=-1), post(B_=0), post(n_=0), post(T_=0),
           lv(x=None), lv(m=None), lv(v=None), lv(t=None), lv(tab=None), lv(outs_=(None,) * 4), lv(ms=n - 1), lv(vs=n - 1), lv(ms=0), lv(mt=2),
           lv(vt=2), lv(vt=-1), lv(B_=0), lv(n_=0), lv(T_=0),
           uni(x=None), uni(m=None), uni(q=None), uni(out=None), uni(B_=0), uni(n_=0), uni(z=None),
           sch(x=None), sch(m=None), sch(out=None), sch(n_=0), sch(z=None)]
    for s in (False, True):
        arg += [dd(s, x=None), dd(s, m=None), dd(s, t=None), dd(s, tab=None), dd(s, sample=None), dd(s, mt=2), dd(s, mt=-1), dd(s, B_=0),
                dd(s, n_=0), dd(s, T_=0), dd(s, rev=1, eta=0.5), dd(s, rev=1, z=Z), dd(s, rev=1, g=G)]
    arg += [dd(True, stride=n - 1), dd(True, stride=0)]
    assert all(rc == E_ARG for rc in arg), [i for i, rc in enumerate(arg) if rc != E_ARG]
    assert _untouched(outs)
    # the same calls are accepted once the argument is right (op 0 takes no y and ignores row_b; sigma == 0 takes no noise)
    ok = [aff(), aff(y=None, op=0, rb=R), post(), lv(), lv(outs_=(None, None, None, o[3])), lv(ms=2 * n, vs=2 * n), dd(False), dd(True, stride=2 * n),
          dd(False, rev=1), uni(), uni(z=None, sigma=0.0), sch(), sch(z=None, sigma=0.0)]
    assert all(rc == 0 for rc in ok), ok
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()) and r.unchanged()


# ---------------------------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_refuse_what_the_kernels_cannot_check():
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    B, n = 3, 8
    x, m, z = (torch.zeros(B, 2, 4, device=DEV) for _ in range(3))
    t, tab = torch.zeros(B, dtype=torch.int64, device=DEV), _tab()
    t2 = torch.zeros(2 * B, dtype=torch.int64, device=DEV)[::2]
    out = lambda: torch.full((B, 2, 4), float("nan"), device=DEV)       # noqa: E731
    o1, o2 = out(), out()

    def affine(x_=x, y_=m, t_=t, tab_=tab, out_=o1):
        return ops.gd_affine(x_, y_, t_, tab_, "sqrt_recip", "sqrt_recipm1", "ax-by", out=out_)

    def post(x_=x, m_=m, t_=t, tab_=tab, noise=z, out_=o1, **kw):
        return ops.gd_posterior_step(x_, m_, t_, tab_, 0, None, None, noise, out_, o2, **kw)

    def ddim(x_=x, m_=m, t_=t, tab_=tab, noise=z, out_=o1):
        return ops.gd_ddim_step(x_, m_, t_, tab_, 0, None, None, noise, 0.5, False, out_, o2)

    bad_tab = tab[:-1].contiguous()
    refused = [lambda: affine(x_=x.double()), lambda: affine(y_=m.double()), lambda: affine(y_=m[:, :1]), lambda: affine(y_=m.view(B, 4, 2)),
               lambda: affine(t_=t2), lambda: affine(t_=t.int()), lambda: affine(t_=t[:2]), lambda: affine(tab_=bad_tab),
               lambda: affine(out_=o1.view(B, 8)), lambda: affine(x_=x.transpose(1, 2)),
               lambda: post(x_=x.double()), lambda: post(m_=m.half()), lambda: post(m_=m[:, :1]), lambda: post(noise=z.view(B, 8)),
               lambda: post(t_=t2), lambda: post(tab_=bad_tab), lambda: post(tab_=tab.double()), lambda: post(var_values=m),
               lambda: post(var_type=ops.GD_LEARNED), lambda: post(variance=o2), lambda: post(log_variance=o2),
               lambda: post(var_values=m.transpose(1, 2), var_type=ops.GD_LEARNED),
               lambda: ddim(x_=x.double()), lambda: ddim(m_=m.double()), lambda: ddim(m_=m[:, :1]), lambda: ddim(noise=z.view(B, 8)),
               lambda: ddim(t_=t2), lambda: ddim(tab_=bad_tab), lambda: ddim(out_=o1[:, :1])]
    for i, f in enumerate(refused):
        with pytest.raises(RhoHipError):
            f()
            pytest.fail(f"call {i} was accepted")
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    affine(), post(), post(var_values=z, var_type=ops.GD_LEARNED, variance=out(), log_variance=out()), ddim()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o1).all())
