"""-m gpu: rho_p_sample_step_spaced_pred, the update of the spaced walk for a backbone that predicts v or x0, at the sizes, tails and
alignments where a streaming kernel goes wrong (the manner of test_gpu_spaced_step.py, whose grid rule this kernel shares).

Buffers sit between 64 sentinel elements; the guided form holds [2, n] with nothing between its rows, so only n % 4 == 0 (and
16-byte aligned bases) takes the 16-byte form there, the plain form takes it for any n and finishes with a scalar tail - all must
give the same bits.  Rows: spaced_pred_coefficients(LinearSchedule(1000), S = 50, eta in {0, 1}) as float32.

Inputs follow the model the update inverts: x0* = 0.7 N(0, 1), eps* = N(0, 1), x = sqrt(ab) x0* + sqrt(1 - ab) eps*; the true
predictions are v* = sqrt(ab) eps* - sqrt(1 - ab) x0* and x0*, and the kernel gets them plus 0.1 N(0, 1).  The x0 estimate is then
x0* + O(0.1) at EVERY row, and the clamp bites where |x0*| is near or above 1: on some elements only (asserted for n >= 255).

Reference: the same expression in float64 on the float32 inputs and rows.  Per-element bound, first order in U = 2^-24, from the
kernel's written-out contraction and its roundings (sa = sqrt_ab, sb = sqrt_1mab, iv = inv_sqrt_1mab, sp = sqrt_abp, ce = coef_eps,
sg = sigma where noise enters, else 0):
    guided only:  d = p_c - p_u  (1)     p = fma(s, d, p_u)  (2)                     plain: p = pred, exact
    v:       m = sb * p  (3)     x0 = fma(sa, x, -m)  (4)                              sample: x0 = p, no rounding
    x0c = clamp(x0, -1, 1) under clip, exact and 1-Lipschitz; else x0c = x0
    [A] clip, or sample:   q = fma(-sa, x0c, x)  (5)     ep = q * iv  (6)
    [B] v without clip:    u = sa * p  (5)               ep = fma(sb, x, u)  (6)
    w  = sg * z  (7)       t = fma(ce, ep, w)  (8)       r = fma(sp, x0c, t)  (9)
Each rounding k contributes U |value_k| times the magnitude of d r / d value_k.  With Ep = |s| |d| + |p| (guided, else 0) and
E0 = sb Ep + |m| + |x0| for v, E0 = Ep for sample (the error of x0 in units of U):
    [A]  d r / d x0c = sp - ce iv sa, bounded by sp + ce iv sa;  d r / d q = ce iv;  d r / d ep = ce
         err <= U [ (sp + ce iv sa) E0 + ce iv |q| + ce |ep| + |w| + |t| + |r| ]
    [B]  r = sp x0 + ce ep + w with x0 = sa x - sb p, ep = sb x + sa p:  d r / d p = ce sa - sp sb, bounded by ce sa + sp sb
         err <= U [ (ce sa + sp sb) Ep + sp (|m| + |x0|) + ce (|u| + |ep|) + |w| + |t| + |r| ]
    row with ce == 0 and sg == 0 (k = 0):  r = sp * x0c (one rounding):   err <= U [ sp E0 + |r| ]
The magnitudes are those of the float64 evaluation; the second-order terms are of relative size 9 U and the factor 1.001 covers
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
SMALL = [1, 3, 4, 5, 255, 257, 1029, 1032]
WRAP_SCALAR = 525_065              # guided, n % 4 == 1: scalar loop, 524288 threads -> second trip of 777 elements
WRAP_VEC = 2_100_228               # n % 4 == 0: 525057 16-byte pieces -> second trip of 769 pieces, the last block ragged
POOL = WRAP_VEC
SCALES = [0.0, 1.0, 3.0, -0.5]
V, SAMPLE = 1, 2                   # RHO_PRED_V, RHO_PRED_SAMPLE
KINDS = {V: "v", SAMPLE: "sample"}


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=None)
def _pool(salt: str) -> torch.Tensor:
    """POOL deterministic ~N(0, 1) float32 values on the CPU; tests take prefixes and never write to them."""
    return det_normal((POOL,), "predstep_" + salt)


@functools.lru_cache(maxsize=None)
def _rows(eta: float, schedule: str = "linear") -> torch.Tensor:
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.prediction import spaced_pred_coefficients
    from rho_diffusion_amd.diffusion.spaced import spaced_timesteps
    if schedule == "linear20":                                   # alpha_bar == 0 at t = 19: every timestep, S = 20
        ab = LinearSchedule(20, 1e-3, 0.02)["alpha_bar_t"]
        return spaced_pred_coefficients(ab, range(20), eta, "v")
    ab = LinearSchedule(T, 1e-3, 0.02)["alpha_bar_t"]
    return spaced_pred_coefficients(ab, spaced_timesteps(len(ab), S), eta, "v")


def _inputs(n, row, kind):
    """(x, p_c, p_u, z) float32 [n] for a row, see the module docstring.  The plain form takes p_c as its prediction."""
    sa, sb = float(row[0]), float(row[1])
    x0, eps = 0.7 * _pool("x0")[:n].double(), _pool("eps")[:n].double()
    x = (sa * x0 + sb * eps).float()
    true = sa * eps - sb * x0 if kind == V else x0
    pc = (true + 0.1 * _pool("p1")[:n].double()).float()
    pu = (true + 0.1 * _pool("p2")[:n].double()).float()
    return x, pc, pu, _pool("z")[:n]


def _run(hip, rows, k, x, pc, pu, z, scale, clip, kind, shifts=frozenset(), row1=None, expect=0):
    """Launch on guarded copies.  ``scale`` None: the plain form on (x, pc), returns [1, n]; else the guided form on [2, n] operands,
    returns [2, n].  Inputs must come back unchanged (z bit for bit, NaN payloads included), every sentinel intact."""
    n = x.numel()
    guided = scale is not None
    xs = torch.cat([x, x if row1 is None else row1]) if guided else x
    ps = torch.cat([pc, pu]) if guided else pc
    gx, gp = Guarded(xs, int("x" in shifts)), Guarded(ps, int("pred" in shifts))
    gz = Guarded(z, int("z" in shifts)) if z is not None else None
    rows_d = rows.to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    rc = hip.lib().rho_p_sample_step_spaced_pred(gx.ptr, gp.ptr, gz.ptr if gz else None, rows_d.data_ptr(), k_dev.data_ptr(),
                                                 rows.shape[0], n, int(guided), float(scale or 0.0), int(clip), kind, hip.stream())
    assert rc == expect, (rc, expect)
    res = gx.cpu().view(2 if guided else 1, n)
    what = (n, k, scale, clip, kind, sorted(shifts))
    assert gx.intact() and gp.intact() and (gz is None or gz.intact()), what
    assert torch.equal(gp.cpu(), ps) and (gz is None or same_bits(gz.cpu(), z)), what
    assert int(k_dev.item()) == k and torch.equal(rows_d.cpu(), rows), what
    return res


def _ref(row, x, pc, pu, z, scale, clip, kind):
    """float64 value, per-element bound and the unclamped x0 estimate (module docstring)."""
    sa, sb, iv, sp, sg, ce = (float(v) for v in row.double()[:6])
    x, pc, pu = x.double(), pc.double(), pu.double()
    x0_only = ce == 0.0 and sg == 0.0                             # the row's own sigma, whether or not z is given
    if z is None or sg == 0.0:
        sg, zz = 0.0, torch.zeros_like(x)
    else:
        zz = z.double()
    if scale is None:
        p, Ep = pc, torch.zeros_like(x)
    else:
        d = pc - pu
        p = pu + scale * d
        Ep = abs(scale) * d.abs() + p.abs()
    if kind == V:
        m = sb * p
        x0 = sa * x - m
        E0 = sb * Ep + m.abs() + x0.abs()
    else:
        m = torch.zeros_like(x)
        x0 = p
        E0 = Ep
    x0c = x0.clamp(-1.0, 1.0) if clip else x0
    if x0_only:
        r = sp * x0c
        return r, 1.001 * U * (sp * E0 + r.abs()), x0
    w = sg * zz
    if clip or kind == SAMPLE:
        q = x - sa * x0c
        ep = q * iv
        t = ce * ep + w
        r = sp * x0c + t
        terms = (sp + ce * iv * sa) * E0 + ce * iv * q.abs() + ce * ep.abs() + w.abs() + t.abs() + r.abs()
    else:
        u = sa * p
        ep = sb * x + u
        t = ce * ep + w
        r = sp * x0 + t
        terms = (ce * sa + sp * sb) * Ep + sp * (m.abs() + x0.abs()) + ce * (u.abs() + ep.abs()) + w.abs() + t.abs() + r.abs()
    return r, 1.001 * U * terms, x0


def _one(hip, n, k, eta, with_z, clip, scale, kind, rows=None):
    rows = _rows(eta) if rows is None else rows
    x, pc, pu, z = _inputs(n, rows[k], kind)
    zz = z if with_z else None
    got = _run(hip, rows, k, x, pc, pu, zz, scale, clip, kind)
    ref, bound, x0 = _ref(rows[k], x, pc, pu, zz, scale, clip, kind)
    what = ("p_sample_step_spaced_pred", KINDS[kind], n, k, eta, with_z, clip, scale)
    check_bound(got[0], ref, bound, what)
    if scale is not None:
        assert same_bits(got[1], got[0]), what                # the second row is the first, bit for bit
    if n >= 255:
        bites = int((x0.abs() > 1.0).sum())
        assert 0 < bites < n, (what, bites)                     # the clamp is exercised on some elements, not on all
        assert (got[0] != x).any(), what
    if k == 0:                                                  # the last step returns the (clamped) x0 estimate
        check_bound(got[0], x0.clamp(-1.0, 1.0) if clip else x0, bound, what + ("x0",))
    return got


@pytest.mark.parametrize("kind", [V, SAMPLE], ids=["v", "sample"])
@pytest.mark.parametrize("n", SMALL)
def test_sizes(hip, n, kind):
    for k in KS:
        for eta in (0.0, 1.0):
            for with_z in (True, False):
                for clip in (1, 0):
                    for scale in [None] + SCALES:
                        _one(hip, n, k, eta, with_z, clip, scale, kind)


@pytest.mark.parametrize("n,k,eta,with_z,clip,scale,kind", [(WRAP_VEC, 24, 1.0, True, 1, None, V), (WRAP_VEC, 1, 1.0, True, 0, 3.0, SAMPLE),
                                                            (WRAP_SCALAR, 24, 1.0, True, 1, -0.5, SAMPLE),
                                                            (WRAP_SCALAR, S - 1, 0.0, False, 0, None, V)])
def test_second_trip(hip, n, k, eta, with_z, clip, scale, kind):
    """Sizes that need a second trip of the grid-stride loop (2048 blocks x 256 threads), one combination each: the 16-byte body
    plain and guided (525057 pieces), the guided scalar loop at an odd n (525065 elements), and the plain form at that n, whose
    16-byte body ends one element short (the scalar tail).  The plain scalar loop at these sizes: test_alignment."""
    _one(hip, n, k, eta, with_z, clip, scale, kind)


@pytest.mark.parametrize("kind", [V, SAMPLE], ids=["v", "sample"])
@pytest.mark.parametrize("scale", [None, 3.0])
def test_last_step_does_not_read_z(hip, scale, kind):
    """k = 0 (sigma = 0 in every table) and every row of an eta = 0 table: z is not read - a z of NaNs leaves the result finite and
    equal to the run without z, bit for bit.  Where noise enters, the NaNs do arrive."""
    n = 1032
    nan_z = torch.full((n,), float("nan"))
    for eta, k in ((1.0, 0), (0.0, 0), (0.0, 24), (0.0, S - 1)):
        rows = _rows(eta)
        x, pc, pu, _ = _inputs(n, rows[k], kind)
        for clip in (1, 0):
            got = _run(hip, rows, k, x, pc, pu, nan_z, scale, clip, kind)
            assert torch.isfinite(got).all(), (eta, k, clip)
            assert same_bits(got, _run(hip, rows, k, x, pc, pu, None, scale, clip, kind)), (eta, k, clip)
    rows = _rows(1.0)
    x, pc, pu, _ = _inputs(n, rows[24], kind)
    assert torch.isnan(_run(hip, rows, 24, x, pc, pu, nan_z, scale, 1, kind)).all()


@pytest.mark.parametrize("n", [5, 1032])
@pytest.mark.parametrize("k", [-1, S, -7, S + 100])
def test_k_outside_the_table_writes_nothing(hip, n, k):
    rows = _rows(1.0)
    for kind in (V, SAMPLE):
        x, pc, pu, z = _inputs(n, rows[1], kind)
        other = x + 1.0
        for zz in (z, None):
            got = _run(hip, rows, k, x, pc, pu, zz, None, 1, kind)
            assert same_bits(got[0], x), (n, k)
            got = _run(hip, rows, k, x, pc, pu, zz, 3.0, 1, kind, row1=other)
            assert same_bits(got[0], x) and same_bits(got[1], other), (n, k)


@pytest.mark.parametrize("n", [5, 1032])
def test_epsilon_and_unknown_types_are_refused(hip, n):
    """RHO_PRED_EPSILON stays on rho_p_sample_step_spaced: RHO_E_ARG (-1), nothing launched, nothing written."""
    rows = _rows(1.0)
    x, pc, pu, z = _inputs(n, rows[24], V)
    for bad in (0, 3, -1):
        for scale in (None, 3.0):
            got = _run(hip, rows, 24, x, pc, pu, z, scale, 1, bad, expect=-1)
            assert same_bits(got[0], x), (n, bad, scale)
    lib = hip.lib()
    g = Guarded(x)
    k_dev = torch.tensor([24], dtype=torch.int32, device=DEV)
    rd = rows.to(DEV)
    for args in ((None, g.ptr, None, rd.data_ptr(), k_dev.data_ptr(), S, n), (g.ptr, None, None, rd.data_ptr(), k_dev.data_ptr(), S, n),
                 (g.ptr, g.ptr, None, None, k_dev.data_ptr(), S, n), (g.ptr, g.ptr, None, rd.data_ptr(), None, S, n),
                 (g.ptr, g.ptr, None, rd.data_ptr(), k_dev.data_ptr(), 0, n), (g.ptr, g.ptr, None, rd.data_ptr(), k_dev.data_ptr(), S, 0)):
        assert lib.rho_p_sample_step_spaced_pred(*args, 0, 0.0, 1, V, hip.stream()) == -1
    assert same_bits(g.cpu(), x) and g.intact()


@pytest.mark.parametrize("n,scale,kind", [(n, s, kd) for n in (1029, 1032) for s in (None, 3.0) for kd in (V, SAMPLE)]
                         + [(WRAP_VEC, 3.0, V), (WRAP_VEC, None, SAMPLE)])
def test_alignment(hip, n, scale, kind):
    """Operands offset by 4 bytes, singly and together, take the scalar loop: the bits of the aligned run.  The second-trip size
    runs once per form: v guided, sample plain."""
    k, clip = 24, 1
    rows = _rows(1.0)
    x, pc, pu, z = _inputs(n, rows[k], kind)
    base = _run(hip, rows, k, x, pc, pu, z, scale, clip, kind)
    ref, bound, _ = _ref(rows[k], x, pc, pu, z, scale, clip, kind)
    check_bound(base[0], ref, bound, ("aligned", n, scale))
    for shifts in [frozenset([s]) for s in ("x", "pred", "z")] + [frozenset(("x", "pred", "z"))]:
        got = _run(hip, rows, k, x, pc, pu, z, scale, clip, kind, shifts)
        assert same_bits(got, base), (n, scale, sorted(shifts))
        if n < WRAP_VEC:
            for kk, cl in ((0, 0), (24, 0)):
                got0 = _run(hip, rows, kk, x, pc, pu, z, scale, cl, kind, shifts)
                assert same_bits(got0, _run(hip, rows, kk, x, pc, pu, z, scale, cl, kind)), (n, scale, kk, sorted(shifts))


@pytest.mark.parametrize("scale", [None, 3.0])
def test_row_without_signal(hip, scale):
    """LinearSchedule(20, 1e-3, 0.02) has alpha_bar == 0 exactly at t = 19: the epsilon rows refuse it, the v row is
    {0, 1, 1, sqrt_abp, sigma, coef_eps} and the update is finite and within the bound of the float64 reference - x0 = -p,
    ep = x (or fma(1, x, 0 * p) without clip)."""
    from rho_diffusion_amd.diffusion import LinearSchedule
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients
    ab = LinearSchedule(20, 1e-3, 0.02)["alpha_bar_t"]
    assert float(ab[19]) == 0.0
    with pytest.raises(ValueError):
        spaced_coefficients(ab, range(20), 0.5)
    for eta in (0.0, 0.5):
        rows = _rows(eta, "linear20")
        assert rows[19, :3].tolist() == [0.0, 1.0, 1.0] and torch.isfinite(rows).all()
        for n in (5, 1032):
            for clip in (1, 0):
                for kind in (V, SAMPLE):
                    got = _one(hip, n, 19, eta, True, clip, scale, kind, rows=rows)
                    assert torch.isfinite(got).all()


def test_wrapper_checks_dtypes_and_shapes(hip):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    n, k = 3 * 16 * 16, 24
    rows_c = _rows(1.0)
    x, pc, pu, z = _inputs(n, rows_c[k], V)
    rows = rows_c.to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    shape = (3, 1, 16, 16)
    xd, pd, zd = x.view(shape).to(DEV), pc.view(shape).to(DEV), z.view(shape).to(DEV)
    out = ops.p_sample_step_spaced_pred(xd, pd, zd, rows, k_dev, V)
    assert out is xd and same_bits(xd.flatten(), _run(hip, rows_c, k, x, pc, pu, z, None, 1, V)[0])
    x2, p2 = torch.cat([x, x]).view(6, 1, 16, 16).to(DEV), torch.cat([pc, pu]).view(6, 1, 16, 16).to(DEV)
    out = ops.p_sample_step_spaced_pred(x2, p2, zd, rows, k_dev, SAMPLE, 3.0, clip=False)
    assert out is x2 and torch.equal(x2[:3], x2[3:])
    assert same_bits(x2.view(2, n), _run(hip, rows_c, k, x, pc, pu, z, 3.0, 0, SAMPLE))
    xd = x.view(shape).to(DEV)
    for bad in (lambda: ops.p_sample_step_spaced_pred(xd.double(), pd, zd, rows, k_dev, V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd[:2].contiguous(), zd, rows, k_dev, V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd, zd[:2].contiguous(), rows, k_dev, V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd, zd, rows[:, :3].contiguous(), k_dev, V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd, zd, rows, k_dev.long(), V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd, zd, rows, k_dev.cpu(), V),
                lambda: ops.p_sample_step_spaced_pred(xd, pd, zd, rows, k_dev, 0),
                lambda: ops.p_sample_step_spaced_pred(x2, pd, zd, rows, k_dev, V, 3.0)):
        with pytest.raises(RhoHipError):
            bad()
    assert same_bits(xd.flatten(), x)                           # nothing was launched
