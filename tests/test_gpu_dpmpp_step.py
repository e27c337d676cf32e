"""-m gpu: rho_dpmpp_2m_step, the DPM-Solver++(2M) update of the spaced walk, at the sizes, tails and alignments where a streaming
kernel goes wrong (the manner of test_gpu_pred_step.py, whose grid rule this kernel shares: 256 threads, at most 2048 blocks, so one
trip of the 16-byte form covers 2 097 152 elements and one trip of the scalar form 524 288).

Buffers sit between 64 sentinel elements; the guided form holds x and pred as [2, n] with nothing between the rows and hist as [n], so
only n % 4 == 0 (and 16-byte aligned x / pred / hist) takes the 16-byte form there; the plain form takes it for any n and finishes
with a scalar tail - all must give the same bits.  Rows: dpmpp_2m_coefficients(LinearSchedule(1000, 1e-3, 0.02), logsnr_timesteps
S = 50, kind): k = 24 and k = 1 are second order (c_d1 != 0), k = S - 1 is first order with c_x != 0, k = 0 has c_x == 0.

Inputs follow the model the update inverts: x0* = 0.7 N(0, 1), eps* = N(0, 1), x = sqrt(ab) x0* + sqrt(1 - ab) eps*; the true
predictions are eps*, v* = sqrt(ab) eps* - sqrt(1 - ab) x0* and x0*, the kernel gets them plus 0.1 N(0, 1), and the history is
x0* + 0.1 N(0, 1).  The x0 estimate is x0* + O(0.1 sqrt(1/ab - 1)), so at the rows with signal the clamp bites on some elements only
(asserted at k <= 24 for n >= 1023).

Reference: the same expression in float64 on the float32 inputs and rows.  Per-element bound, first order in U = 2^-24, from the
kernel's written-out contraction and its roundings (ax = a_x, ap = a_p, cx = c_x, d0 = c_d0, d1 = c_d1):
    guided only:  d = p_c - p_u  (1)     p = fma(s, d, p_u)  (2)                     plain: p = pred, exact
    epsilon, v:   m = ap * p  (3)        x0 = fma(ax, x, -m)  (4)                     sample: x0 = p, no rounding
    x0c = clamp(x0, -1, 1) under clip, exact and 1-Lipschitz; else x0c = x0           hist <- x0c
    d1 != 0:             w = d1 * hist  (5)     t = fma(d0, x0c, w)  (6)     r = fma(cx, x, t)  (7)
    d1 == 0:             u = d0 * x0c  (5)      r = fma(cx, x, u)  (6)
    d1 == 0 and cx == 0: r = d0 * x0c  (5)
Each rounding k contributes U |value_k| times the magnitude of d r / d value_k.  With Ep = |s| |d| + |p| (guided, else 0) and
E0 = ap Ep + |m| + |x0| for epsilon and v, E0 = Ep for sample (the error of x0, and so of the new hist, in units of U):
    d1 != 0:              err <= U [ |d0| E0 + |w| + |t| + |r| ]
    d1 == 0:              err <= U [ |d0| E0 + |u| + |r| ]
    d1 == 0 and cx == 0:  err <= U [ |d0| E0 + |r| ]
    hist:                 err <= U E0
The magnitudes are those of the float64 evaluation; the second-order terms are of relative size 7 U and the factor 1.001 covers
them."""
import functools

import pytest
import torch

from helpers import det_normal
from gpu_util import DEV, Guarded, check_bound, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
T = 1000
S = 50
KS = [S - 1, 24, 1, 0]
SMALL = [1, 3, 4, 5, 1023, 1024, 1027]
TRIP_VEC = 2_097_152               # elements per trip of the 16-byte form: 2048 blocks x 256 threads x 4
TRIP_SCALAR = 524_288              # elements per trip of the scalar form
SECOND, THIRD = TRIP_VEC + 5, 2 * TRIP_VEC + 7
POOL = THIRD + 1
SCALES = [0.0, 1.0, 3.0, -0.5]
EPS, V, SAMPLE = 0, 1, 2           # RHO_PRED_EPSILON, RHO_PRED_V, RHO_PRED_SAMPLE
KINDS = {EPS: "epsilon", V: "v", SAMPLE: "sample"}
ALL = [EPS, V, SAMPLE]
IDS = ["epsilon", "v", "sample"]


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=None)
def _pool(salt: str) -> torch.Tensor:
    """POOL deterministic ~N(0, 1) float32 values on the CPU; tests take prefixes and never write to them."""
    return det_normal((POOL,), "dpmppstep_" + salt)


@functools.lru_cache(maxsize=None)
def _table(schedule: str = "linear"):
    """(alpha_bar float64 list, taus) of the rows under test."""
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.multistep import logsnr_timesteps
    if schedule == "linear20":                                   # alpha_bar == 0 at t = 19: every timestep, S = 20
        ab = LinearSchedule(20, 1e-3, 0.02)["alpha_bar_t"].float()
        return ab.double().tolist(), tuple(range(20))
    ab = LinearSchedule(T, 1e-3, 0.02)["alpha_bar_t"].float()
    return ab.double().tolist(), tuple(logsnr_timesteps(ab, S))


@functools.lru_cache(maxsize=None)
def _rows(kind: int, schedule: str = "linear") -> torch.Tensor:
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients
    ab, taus = _table(schedule)
    return dpmpp_2m_coefficients(torch.tensor(ab, dtype=torch.float64).float(), taus, KINDS[kind])


def _inputs(n, k, kind, schedule="linear"):
    """(x, p_c, p_u, hist) float32 [n] for row k, see the module docstring.  The plain form takes p_c as its prediction."""
    ab, taus = _table(schedule)
    a = ab[taus[k]]
    sa, sb = a ** 0.5, (1.0 - a) ** 0.5
    x0, eps = 0.7 * _pool("x0")[:n].double(), _pool("eps")[:n].double()
    x = (sa * x0 + sb * eps).float()
    true = {EPS: eps, V: sa * eps - sb * x0, SAMPLE: x0}[kind]
    pc = (true + 0.1 * _pool("p1")[:n].double()).float()
    pu = (true + 0.1 * _pool("p2")[:n].double()).float()
    hist = (x0 + 0.1 * _pool("h")[:n].double()).float()
    return x, pc, pu, hist


def _run(hip, rows, k, x, pc, pu, hist, scale, clip, kind, shifts=frozenset(), row1=None, expect=0):
    """Launch on guarded copies.  ``scale`` None: the plain form on (x, pc); else the guided form on [2, n] operands.  Returns
    (x after the call as [1, n] or [2, n], hist after the call [n]).  pred, rows and k must come back unchanged, every sentinel
    intact."""
    n = x.numel()
    guided = scale is not None
    xs = torch.cat([x, x if row1 is None else row1]) if guided else x
    ps = torch.cat([pc, pu]) if guided else pc
    gx, gp, gh = Guarded(xs, int("x" in shifts)), Guarded(ps, int("pred" in shifts)), Guarded(hist, int("hist" in shifts))
    rows_d = rows.to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    rc = hip.lib().rho_dpmpp_2m_step(gx.ptr, gp.ptr, gh.ptr, rows_d.data_ptr(), k_dev.data_ptr(), rows.shape[0], n, int(guided),
                                     float(scale or 0.0), int(clip), kind, hip.stream())
    assert rc == expect, (rc, expect)
    res = gx.cpu().view(2 if guided else 1, n)
    what = (n, k, scale, clip, kind, sorted(shifts))
    assert gx.intact() and gp.intact() and gh.intact(), what
    assert torch.equal(gp.cpu(), ps), what
    assert int(k_dev.item()) == k and torch.equal(rows_d.cpu(), rows), what
    return res, gh.cpu()


def _ref(row, x, pc, pu, hist, scale, clip, kind):
    """float64 value of x', its per-element bound, the (clamped) x0 estimate, its bound, and the unclamped estimate."""
    ax, ap, cx, d0, d1 = (float(v) for v in row.double()[:5])
    x, pc, pu, hist = x.double(), pc.double(), pu.double(), hist.double()
    if scale is None:
        p, Ep = pc, torch.zeros_like(x)
    else:
        d = pc - pu
        p = pu + scale * d
        Ep = abs(scale) * d.abs() + p.abs()
    if kind == SAMPLE:
        x0, E0 = p, Ep
    else:
        m = ap * p
        x0 = ax * x - m
        E0 = ap * Ep + m.abs() + x0.abs()
    x0c = x0.clamp(-1.0, 1.0) if clip else x0
    if d1 != 0.0:
        w = d1 * hist
        t = d0 * x0c + w
        r = cx * x + t
        terms = abs(d0) * E0 + w.abs() + t.abs() + r.abs()
    elif cx != 0.0:
        u = d0 * x0c
        r = cx * x + u
        terms = abs(d0) * E0 + u.abs() + r.abs()
    else:
        r = d0 * x0c
        terms = abs(d0) * E0 + r.abs()
    return r, 1.001 * U * terms, x0c, 1.001 * U * E0, x0


def _one(hip, n, k, clip, scale, kind, schedule="linear", shifts=frozenset()):
    rows = _rows(kind, schedule)
    x, pc, pu, hist = _inputs(n, k, kind, schedule)
    got, h = _run(hip, rows, k, x, pc, pu, hist, scale, clip, kind, shifts)
    ref, bound, x0c, b0, x0 = _ref(rows[k], x, pc, pu, hist, scale, clip, kind)
    what = ("dpmpp_2m_step", KINDS[kind], schedule, n, k, clip, scale, sorted(shifts))
    check_bound(got[0], ref, bound, what)
    check_bound(h, x0c, b0, what + ("hist",))
    if clip:
        assert float(h.abs().max()) <= 1.0, what
        sure = x0.abs() > 1.0 + b0                              # the float32 estimate is beyond the clamp whatever it rounded to
        assert torch.equal(h[sure].double(), x0.sign()[sure]), what
    if scale is not None:
        assert same_bits(got[1], got[0]), what                # the second row is the first, bit for bit
    if n >= 1023 and k <= 24 and schedule == "linear":
        bites = int((x0.abs() > 1.0).sum())
        assert 0 < bites < n, (what, bites)                     # the clamp is exercised on some elements, not on all
        assert (got[0] != x).any() and (h != hist).any(), what
    if k == 0:                                                  # row 0 is {.., 0, 1, 0}: the last step returns the x0 estimate itself
        assert rows[0, 2:5].tolist() == [0.0, 1.0, 0.0] and same_bits(got[0], h), what
    return got, h


def test_rows_under_test_have_the_three_orders():
    for kind in ALL:
        rows = _rows(kind)
        assert tuple(rows.shape) == (S, 8)
        assert float(rows[24, 4]) < 0.0 and float(rows[1, 4]) < 0.0 and float(rows[24, 2]) > 0.0
        assert float(rows[S - 1, 4]) == 0.0 and float(rows[S - 1, 2]) > 0.0 and float(rows[S - 1, 3]) > 0.0
        assert rows[0, 2:5].tolist() == [0.0, 1.0, 0.0]


@pytest.mark.parametrize("kind", ALL, ids=IDS)
@pytest.mark.parametrize("n", SMALL)
def test_sizes(hip, n, kind):
    for k in KS:
        for clip in (1, 0):
            for scale in [None] + SCALES:
                _one(hip, n, k, clip, scale, kind)


@pytest.mark.parametrize("n,k,clip,scale,kind", [(SECOND, 24, 1, None, EPS), (THIRD, 1, 0, None, V), (TRIP_VEC + 8, 24, 1, 3.0, SAMPLE),
                                                 (2 * TRIP_VEC + 8, S - 1, 0, -0.5, EPS), (SECOND, 1, 1, 3.0, V), (THIRD, 0, 1, None, SAMPLE)])
def test_further_trips(hip, n, k, clip, scale, kind):
    """Sizes that need a second and a third trip of the grid-stride loop, one combination each: the 16-byte body plain at
    2 097 152 + 5 and 2 * 2 097 152 + 7 (its scalar tail behind the last trip) and guided at n % 4 == 0 (2 and 3 trips), and the guided
    scalar loop at an odd n (2 097 157 elements: five trips).  The plain scalar loop past its trip boundary: test_alignment."""
    _one(hip, n, k, clip, scale, kind)


@pytest.mark.parametrize("kind", ALL, ids=IDS)
@pytest.mark.parametrize("scale", [None, 3.0])
def test_first_order_rows_do_not_read_hist(hip, scale, kind):
    """c_d1 == 0 (k = S - 1: the first step of a walk, whose hist is uninitialised; k = 0): a hist of NaNs leaves the result finite
    and equal to the run with a finite hist, bit for bit, and hist afterwards is the x0 estimate.  On a second-order row the NaNs do
    arrive in x, and hist is still replaced by the finite estimate."""
    rows = _rows(kind)
    for n in (5, 1027, 1024):
        nan_h = torch.full((n,), float("nan"))
        for k in (S - 1, 0):
            x, pc, pu, hist = _inputs(n, k, kind)
            for clip in (1, 0):
                got, h = _run(hip, rows, k, x, pc, pu, nan_h, scale, clip, kind)
                base, hb = _run(hip, rows, k, x, pc, pu, hist, scale, clip, kind)
                assert torch.isfinite(got).all() and torch.isfinite(h).all(), (n, k, clip)
                assert same_bits(got, base) and same_bits(h, hb), (n, k, clip)
                _, _, x0c, b0, _ = _ref(rows[k], x, pc, pu, hist, scale, clip, kind)
                check_bound(h, x0c, b0, ("hist after a NaN history", n, k, clip))
        x, pc, pu, hist = _inputs(n, 24, kind)
        got, h = _run(hip, rows, 24, x, pc, pu, nan_h, scale, 1, kind)
        assert torch.isnan(got).all() and torch.isfinite(h).all()
        assert same_bits(h, _run(hip, rows, 24, x, pc, pu, hist, scale, 1, kind)[1])


@pytest.mark.parametrize("n", [5, 1024])
@pytest.mark.parametrize("k", [-1, S, -7, S + 100])
def test_k_outside_the_table_writes_nothing(hip, n, k):
    for kind in ALL:
        rows = _rows(kind)
        x, pc, pu, hist = _inputs(n, 1, kind)
        other = x + 1.0
        got, h = _run(hip, rows, k, x, pc, pu, hist, None, 1, kind)
        assert same_bits(got[0], x) and same_bits(h, hist), (n, k)
        got, h = _run(hip, rows, k, x, pc, pu, hist, 3.0, 1, kind, row1=other)
        assert same_bits(got[0], x) and same_bits(got[1], other) and same_bits(h, hist), (n, k)


@pytest.mark.parametrize("n", [5, 1024])
def test_bad_arguments_are_refused(hip, n):
    """An unknown prediction type, a NULL operand, S <= 0, n <= 0: RHO_E_ARG (-1), nothing launched, nothing written."""
    rows = _rows(V)
    x, pc, pu, hist = _inputs(n, 24, V)
    for bad in (3, -1, 7):
        for scale in (None, 3.0):
            got, h = _run(hip, rows, 24, x, pc, pu, hist, scale, 1, bad, expect=-1)
            assert same_bits(got[0], x) and same_bits(h, hist), (n, bad, scale)
    lib = hip.lib()
    g, gh = Guarded(x), Guarded(hist)
    k_dev = torch.tensor([24], dtype=torch.int32, device=DEV)
    rd = rows.to(DEV)
    ok = (g.ptr, g.ptr, gh.ptr, rd.data_ptr(), k_dev.data_ptr(), S, n)
    for i, repl in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (5, -3), (6, 0), (6, -1)):
        args = list(ok)
        args[i] = repl
        for guided in (0, 1):
            assert lib.rho_dpmpp_2m_step(*args, guided, 0.0, 1, V, hip.stream()) == -1, (i, repl, guided)
    torch.cuda.synchronize()
    assert same_bits(g.cpu(), x) and g.intact() and same_bits(gh.cpu(), hist) and gh.intact()


@pytest.mark.parametrize("n,scale,kind", [(n, s, kd) for n in (1027, 1024) for s in (None, 3.0) for kd in ALL]
                         + [(TRIP_SCALAR + 3, None, EPS), (TRIP_SCALAR + 3, 3.0, V), (TRIP_SCALAR + 4, 3.0, SAMPLE)])
def test_alignment(hip, n, scale, kind):
    """x, pred and hist offset by 4 bytes, each in turn and together, take the scalar loop: the bits of the aligned run - which is the
    16-byte body with its tail (plain), the 16-byte body alone (guided, n % 4 == 0) or the scalar loop already (guided, n % 4 != 0) -
    in x and in hist.  524 288 + 3 crosses the scalar form's trip boundary."""
    rows = _rows(kind)
    big = n > 2000
    for k, clip in ((24, 1),) if big else ((24, 1), (24, 0), (S - 1, 1), (0, 0)):
        x, pc, pu, hist = _inputs(n, k, kind)
        base, hb = _run(hip, rows, k, x, pc, pu, hist, scale, clip, kind)
        ref, bound, x0c, b0, _ = _ref(rows[k], x, pc, pu, hist, scale, clip, kind)
        check_bound(base[0], ref, bound, ("aligned", n, scale, k, clip))
        check_bound(hb, x0c, b0, ("aligned hist", n, scale, k, clip))
        for shifts in [frozenset([s]) for s in ("x", "pred", "hist")] + [frozenset(("x", "pred", "hist"))]:
            got, h = _run(hip, rows, k, x, pc, pu, hist, scale, clip, kind, shifts)
            assert same_bits(got, base) and same_bits(h, hb), (n, scale, k, clip, sorted(shifts))


@pytest.mark.parametrize("scale", [None, 3.0])
def test_source_without_signal(hip, scale):
    """LinearSchedule(20, 1e-3, 0.02) has alpha_bar == 0 exactly at t = 19: the epsilon rows refuse it, the v row is
    {0, 1, sigma', alpha', 0} (x0 = -p) and the sample row {0, 0, sigma', alpha', 0}; the update is finite and within the bound of
    the float64 reference, as are row 18 (first order: its h_prev is not finite) and row 17 (second order)."""
    from rho_diffusion_amd.diffusion.multistep import dpmpp_2m_coefficients
    ab, taus = _table("linear20")
    assert ab[19] == 0.0
    with pytest.raises(ValueError):
        dpmpp_2m_coefficients(torch.tensor(ab).float(), taus, "epsilon")
    for kind in (V, SAMPLE):
        rows = _rows(kind, "linear20")
        assert torch.isfinite(rows).all() and rows[19, 4] == 0.0 and rows[18, 4] == 0.0 and rows[17, 4] < 0.0
        assert rows[19, :2].tolist() == ([0.0, 1.0] if kind == V else [0.0, 0.0])
        for n in (5, 1027):
            for clip in (1, 0):
                for k in (19, 18, 17):
                    got, h = _one(hip, n, k, clip, scale, kind, schedule="linear20")
                    assert torch.isfinite(got).all() and torch.isfinite(h).all()


def test_wrapper_checks_dtypes_and_shapes(hip):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    n, k = 3 * 16 * 16, 24
    rows_c = _rows(EPS)
    x, pc, pu, hist = _inputs(n, k, EPS)
    rows = rows_c.to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    shape = (3, 1, 16, 16)
    xd, pd, hd = x.view(shape).to(DEV), pc.view(shape).to(DEV), hist.view(shape).to(DEV)
    out = ops.dpmpp_2m_step(xd, pd, hd, rows, k_dev, EPS)
    want, hw = _run(hip, rows_c, k, x, pc, pu, hist, None, 1, EPS)
    assert out is xd and same_bits(xd.flatten(), want[0]) and same_bits(hd.flatten(), hw)
    x2, p2 = torch.cat([x, x]).view(6, 1, 16, 16).to(DEV), torch.cat([pc, pu]).view(6, 1, 16, 16).to(DEV)
    hd = hist.view(shape).to(DEV)
    out = ops.dpmpp_2m_step(x2, p2, hd, rows_c.to(DEV), k_dev, EPS, 3.0, clip=False)
    want, hw = _run(hip, rows_c, k, x, pc, pu, hist, 3.0, 0, EPS)
    assert out is x2 and torch.equal(x2[:3], x2[3:]) and tuple(hd.shape) == shape
    assert same_bits(x2.view(2, n), want) and same_bits(hd.flatten(), hw)
    xd, hd = x.view(shape).to(DEV), hist.view(shape).to(DEV)
    for bad in (lambda: ops.dpmpp_2m_step(xd.double(), pd, hd, rows, k_dev, EPS),
                lambda: ops.dpmpp_2m_step(xd, pd[:2].contiguous(), hd, rows, k_dev, EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd[:2].contiguous(), rows, k_dev, EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd.double(), rows, k_dev, EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd, rows[:, :3].contiguous(), k_dev, EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd, rows, k_dev.long(), EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd, rows, k_dev.cpu(), EPS),
                lambda: ops.dpmpp_2m_step(xd, pd, hd, rows, k_dev, 3),
                lambda: ops.dpmpp_2m_step(x2, pd, hd, rows, k_dev, EPS, 3.0),
                lambda: ops.dpmpp_2m_step(x2, p2, torch.cat([hd, hd]), rows, k_dev, EPS, 3.0)):
        with pytest.raises(RhoHipError):
            bad()
    assert same_bits(xd.flatten(), x) and same_bits(hd.flatten(), hist)         # nothing was launched
