"""-m gpu: rho_p_sample_step_spaced and rho_spaced_advance, the update and the loop state of few-step sampling, at the sizes, tails
and alignments where a streaming kernel goes wrong (the manner of test_gpu_cfg_step.py).

Buffers sit between 64 sentinel elements; the guided form holds [2, n] with nothing between its rows, so only n % 4 == 0 (and
16-byte aligned bases) takes the 16-byte form there, the plain form takes it for any n and finishes with a scalar tail - all must
give the same bits.  Rows: spaced_coefficients(LinearSchedule(1000), S = 50, eta in {0, 1}) as float32.

Inputs follow the model the update inverts: x = sqrt(ab) x0* + sqrt(1 - ab) eps*, with x0* = 0.7 N(0, 1) and the predictions eps*
plus a perturbation of size a = 0.1 / max(c_recipm1, 1), so that at EVERY row the x0 estimate is x0* + O(0.3) and the clamp bites
on some elements only (asserted for n >= 255).

Reference: the same expression in float64 on the float32 inputs and rows.  Per-element bound, first order in U = 2^-24, from the
kernel's written-out contraction and its roundings (c0 = c_recip, c1 = c_recipm1, sa = sqrt_ab, iv = inv_sqrt_1mab, sp = sqrt_abp,
ce = coef_eps, sg = sigma where noise enters, else 0):
    guided only:  d = e_c - e_u  (1)     e = fma(s, d, e_u)  (2)                      plain: e = eps_hat, exact
    m  = c1 * e  (3)       x0 = fma(c0, x, -m)  (4)       x0c = clamp(x0, -1, 1)   exact and 1-Lipschitz
    q  = fma(-sa, x0c, x)  (5)      ep = q * iv  (6)                                 without clip: ep = e, no rounding
    w  = sg * z  (7)       v = fma(ce, ep, w)  (8)        r = fma(sp, x0c, v)  (9)
Each rounding k contributes U |value_k| times the magnitude of d r / d value_k:
    with clip     d r / d x0c = sp - ce iv sa, bounded by A = sp + ce iv sa;  d r / d q = ce iv;  d r / d ep = ce
                  err <= U [ A (c1 (|s| |d| + |e|) + |m| + |x0|) + ce iv |q| + ce |ep| + |w| + |v| + |r| ]
    without clip  r = sp x0 + ce e + w:  d r / d e = ce - sp c1 (through m), bounded by ce + sp c1
                  err <= U [ (ce + sp c1) (|s| |d| + |e|) + sp (|m| + |x0|) + |w| + |v| + |r| ]
    row with ce == 0 and sg == 0 (k = 0):  r = sp * x0c (one rounding)
                  err <= U [ sp (c1 (|s| |d| + |e|) + |m| + |x0|) + |r| ]
(the |s| |d| + |e| terms only when guided).  The magnitudes are those of the float64 evaluation; the second-order terms are of
relative size 9 U and the factor 1.001 covers them."""
import functools

import pytest
import torch

from helpers import det_normal, det_uniform
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


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@functools.lru_cache(maxsize=None)
def _pool(salt: str) -> torch.Tensor:
    """POOL deterministic ~N(0, 1) float32 values on the CPU; tests take prefixes and never write to them."""
    return det_normal((POOL,), "spacedstep_" + salt)


@functools.lru_cache(maxsize=None)
def _rows(eta: float, schedule: str = "linear") -> torch.Tensor:
    from rho_diffusion_amd.diffusion import CosineBetaSchedule, LinearSchedule
    from rho_diffusion_amd.diffusion.spaced import spaced_coefficients, spaced_timesteps
    ab = (LinearSchedule(T, 1e-3, 0.02) if schedule == "linear" else CosineBetaSchedule(T))["alpha_bar_t"]
    return spaced_coefficients(ab, spaced_timesteps(len(ab), S), eta)


def _inputs(n, k):
    """(x, e_c, e_u, z) float32 [n] for row k, see the module docstring.  The plain form takes e_c as its prediction."""
    row = _rows(0.0)[k].double()
    sa, c1 = float(row[2]), float(row[1])
    ab = sa * sa
    x0, eps = 0.7 * _pool("x0")[:n].double(), _pool("eps")[:n].double()
    x = (sa * x0 + (1.0 - ab) ** 0.5 * eps).float()
    a = 0.1 / max(c1, 1.0)
    ec = (eps + a * _pool("p1")[:n].double()).float()
    eu = (eps + a * _pool("p2")[:n].double()).float()
    return x, ec, eu, _pool("z")[:n]


def _run(hip, rows, k, x, ec, eu, z, scale, clip, shifts=frozenset(), row1=None):
    """Launch on guarded copies.  ``scale`` None: the plain form on (x, ec), returns [1, n]; else the guided form on [2, n] operands,
    returns [2, n].  Inputs must come back unchanged (z bit for bit, NaN payloads included), every sentinel intact."""
    n = x.numel()
    guided = scale is not None
    xs = torch.cat([x, x if row1 is None else row1]) if guided else x
    es = torch.cat([ec, eu]) if guided else ec
    gx, ge = Guarded(xs, int("x" in shifts)), Guarded(es, int("eps" in shifts))
    gz = Guarded(z, int("z" in shifts)) if z is not None else None
    rows_d = rows.to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    hip.check(hip.lib().rho_p_sample_step_spaced(gx.ptr, ge.ptr, gz.ptr if gz else None, rows_d.data_ptr(), k_dev.data_ptr(),
                                                 rows.shape[0], n, int(guided), float(scale or 0.0), int(clip), hip.stream()),
              "rho_p_sample_step_spaced")
    res = gx.cpu().view(2 if guided else 1, n)
    what = (n, k, scale, clip, sorted(shifts))
    assert gx.intact() and ge.intact() and (gz is None or gz.intact()), what
    assert torch.equal(ge.cpu(), es) and (gz is None or same_bits(gz.cpu(), z)), what
    assert int(k_dev.item()) == k and torch.equal(rows_d.cpu(), rows), what
    return res


def _ref(row, x, ec, eu, z, scale, clip):
    """float64 value, per-element bound and the unclamped x0 estimate (module docstring)."""
    c0, c1, sa, iv, sp, sg, ce = (float(v) for v in row.double()[:7])
    x, ec, eu = x.double(), ec.double(), eu.double()
    x0_only = ce == 0.0 and sg == 0.0                             # the row's own sigma, whether or not z is given
    if z is None or sg == 0.0:
        sg, zz = 0.0, torch.zeros_like(x)
    else:
        zz = z.double()
    if scale is None:
        e, e_err = ec, torch.zeros_like(x)
    else:
        d = ec - eu
        e = eu + scale * d
        e_err = abs(scale) * d.abs() + e.abs()
    m = c1 * e
    x0 = c0 * x - m
    x0c = x0.clamp(-1.0, 1.0) if clip else x0
    if x0_only:
        r = sp * x0c
        terms = sp * (c1 * e_err + m.abs() + x0.abs()) + r.abs()
        return r, 1.001 * U * terms, x0
    w = sg * zz
    if clip:
        q = x - sa * x0c
        ep = q * iv
        v = ce * ep + w
        r = sp * x0c + v
        terms = (sp + ce * iv * sa) * (c1 * e_err + m.abs() + x0.abs()) + ce * iv * q.abs() + ce * ep.abs() + w.abs() + v.abs() + r.abs()
    else:
        v = ce * e + w
        r = sp * x0 + v
        terms = (ce + sp * c1) * e_err + sp * (m.abs() + x0.abs()) + w.abs() + v.abs() + r.abs()
    return r, 1.001 * U * terms, x0


def _one(hip, n, k, eta, with_z, clip, scale):
    rows = _rows(eta)
    x, ec, eu, z = _inputs(n, k)
    zz = z if with_z else None
    got = _run(hip, rows, k, x, ec, eu, zz, scale, clip)
    ref, bound, x0 = _ref(rows[k], x, ec, eu, zz, scale, clip)
    what = ("p_sample_step_spaced", n, k, eta, with_z, clip, scale)
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


@pytest.mark.parametrize("n", SMALL)
def test_p_sample_step_spaced_sizes(hip, n):
    for k in KS:
        for eta in (0.0, 1.0):
            for with_z in (True, False):
                for clip in (1, 0):
                    for scale in [None] + SCALES:
                        _one(hip, n, k, eta, with_z, clip, scale)


@pytest.mark.parametrize("n,k,eta,with_z,clip,scale", [(WRAP_VEC, 24, 1.0, True, 1, None), (WRAP_VEC, 1, 1.0, True, 1, 3.0),
                                                       (WRAP_SCALAR, 24, 1.0, True, 1, -0.5), (WRAP_SCALAR, S - 1, 0.0, False, 0, None)])
def test_p_sample_step_spaced_second_trip(hip, n, k, eta, with_z, clip, scale):
    """Sizes that need a second trip of the grid-stride loop (2048 blocks x 256 threads), one combination each: the 16-byte body
    plain and guided (525057 pieces), the guided scalar loop at an odd n (525065 elements), and the plain form at that n, whose
    16-byte body ends one element short (the scalar tail).  The plain scalar loop at these sizes: test_alignment."""
    _one(hip, n, k, eta, with_z, clip, scale)


@pytest.mark.parametrize("scale", [None, 3.0])
def test_last_step_does_not_read_z(hip, scale):
    """k = 0 (sigma = 0 in every table) and every row of an eta = 0 table: z is not read - a z of NaNs leaves the result finite and
    equal to the run without z, bit for bit, and comes back untouched."""
    n = 1032
    nan_z = torch.full((n,), float("nan"))
    for eta, k in ((1.0, 0), (0.0, 0), (0.0, 24), (0.0, S - 1)):
        x, ec, eu, _ = _inputs(n, k)
        for clip in (1, 0):
            got = _run(hip, _rows(eta), k, x, ec, eu, nan_z, scale, clip)
            assert torch.isfinite(got).all(), (eta, k, clip)
            assert same_bits(got, _run(hip, _rows(eta), k, x, ec, eu, None, scale, clip)), (eta, k, clip)
    x, ec, eu, _ = _inputs(n, 24)                               # and where noise enters, the NaNs do arrive: z is read there
    assert torch.isnan(_run(hip, _rows(1.0), 24, x, ec, eu, nan_z, scale, 1)).all()


@pytest.mark.parametrize("n", [5, 1032])
@pytest.mark.parametrize("k", [-1, S, -7, S + 100])
def test_k_outside_the_table_writes_nothing(hip, n, k):
    x, ec, eu, z = _inputs(n, 1)
    other = x + 1.0
    for zz in (z, None):
        got = _run(hip, _rows(1.0), k, x, ec, eu, zz, None, 1)
        assert same_bits(got[0], x), (n, k)
        got = _run(hip, _rows(1.0), k, x, ec, eu, zz, 3.0, 1, row1=other)
        assert same_bits(got[0], x) and same_bits(got[1], other), (n, k)


@pytest.mark.parametrize("n", [1029, 1032, WRAP_VEC])
@pytest.mark.parametrize("scale", [None, 3.0])
def test_alignment(hip, n, scale):
    """Operands offset by 4 bytes, singly and together, take the scalar loop: the bits of the aligned run."""
    k, clip = 24, 1
    x, ec, eu, z = _inputs(n, k)
    rows = _rows(1.0)
    base = _run(hip, rows, k, x, ec, eu, z, scale, clip)
    ref, bound, _ = _ref(rows[k], x, ec, eu, z, scale, clip)
    check_bound(base[0], ref, bound, ("aligned", n, scale))
    for shifts in [frozenset([s]) for s in ("x", "eps", "z")] + [frozenset(("x", "eps", "z"))]:
        got = _run(hip, rows, k, x, ec, eu, z, scale, clip, shifts)
        assert same_bits(got, base), (n, scale, sorted(shifts))
        if n < WRAP_VEC:
            got0 = _run(hip, rows, 0, x, ec, eu, z, scale, 0, shifts)
            assert same_bits(got0, _run(hip, rows, 0, x, ec, eu, z, scale, 0)), (n, scale, sorted(shifts))


@pytest.mark.parametrize("scale", [None, 3.0])
def test_degenerate_rows_of_the_cosine_schedule(hip, scale):
    """CosineBetaSchedule(1000): the last row (alpha_bar = 3.75e-33, c_recip = 1.6e16) and the t = 0 row (alpha_bar = 1, so
    inv_sqrt_1mab is written as 0 and ep is never formed).  No bound is claimed, only finite and in range.  In range is a property of
    the inputs as much as of the kernel: with clip the result is bounded by sqrt_abp + coef_eps * inv_sqrt_1mab * (|x| + sqrt_ab) +
    sigma * |z|, so x and z are drawn from [-0.9, 0.9] and that expression is asserted not to exceed 1 from the rows themselves."""
    n = 1032
    x, z = det_uniform((n,), "spaced_cos_x", -0.9, 0.9), det_uniform((n,), "spaced_cos_z", -0.9, 0.9)
    ec, eu = _pool("eps")[:n], _pool("p1")[:n]
    for eta in (0.0, 1.0):
        rows = _rows(eta, "cosine")
        assert float(rows[S - 1, 0]) > 1e15 and float(rows[0, 3]) == 0.0 and float(rows[0, 0]) == 1.0
        for k in (S - 1, 0):
            c0, c1, sa, iv, sp, sg, ce = (float(v) for v in rows[k].double()[:7])
            assert sp + ce * iv * (0.9 + sa) + sg * 0.9 <= 1.0, (eta, k)
            for zz in (z, None):
                got = _run(hip, rows, k, x, ec, eu, zz, scale, 1)
                assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0, (eta, k, zz is not None)
                if scale is not None:
                    assert same_bits(got[0], got[1])
        # t = 0: the update is the clamp of x itself (c_recip = 1, c_recipm1 = 0)
        got = _run(hip, rows, 0, x, ec, eu, z, scale, 1)
        assert same_bits(got[0], x)


def test_spaced_advance(hip):
    taus = torch.tensor([3, 11, 17], dtype=torch.int32, device=DEV)
    guard = torch.full((8,), -5, dtype=torch.int32, device=DEV)         # taus sits inside: a read of taus[-1] would see -5
    guard[4:7] = taus
    tv = guard[4:7]
    k_dev = torch.tensor([2], dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([17], dtype=torch.int32, device=DEV)
    off = torch.tensor([(1 << 40) + 5], dtype=torch.int64, device=DEV)
    delta = (1 << 33) + 3
    seen = []
    for i in range(3):
        hip.check(hip.lib().rho_spaced_advance(k_dev.data_ptr(), t_dev.data_ptr(), tv.data_ptr(), off.data_ptr(), delta, hip.stream()),
                  "rho_spaced_advance")
        seen.append((int(k_dev.item()), int(t_dev.item()), int(off.item())))
    base = (1 << 40) + 5
    assert seen == [(1, 11, base + delta), (0, 3, base + 2 * delta), (-1, 3, base + 3 * delta)]      # t keeps its last value
    assert guard.tolist() == [-5, -5, -5, -5, 3, 11, 17, -5]
    # NULL offset_dev
    k_dev.fill_(2)
    hip.check(hip.lib().rho_spaced_advance(k_dev.data_ptr(), t_dev.data_ptr(), tv.data_ptr(), None, delta, hip.stream()), "rho_spaced_advance")
    assert (int(k_dev.item()), int(t_dev.item()), int(off.item())) == (1, 11, base + 3 * delta)
    # NULL state is refused, not dereferenced
    assert hip.lib().rho_spaced_advance(None, t_dev.data_ptr(), tv.data_ptr(), None, 0, hip.stream()) < 0
    assert hip.lib().rho_spaced_advance(k_dev.data_ptr(), None, tv.data_ptr(), None, 0, hip.stream()) < 0
    assert hip.lib().rho_spaced_advance(k_dev.data_ptr(), t_dev.data_ptr(), None, None, 0, hip.stream()) < 0


def test_wrappers_check_dtypes_and_shapes(hip):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    n, k = 3 * 16 * 16, 24
    x, ec, eu, z = _inputs(n, k)
    rows = _rows(1.0).to(DEV)
    k_dev = torch.tensor([k], dtype=torch.int32, device=DEV)
    shape = (3, 1, 16, 16)
    xd, ed, zd = x.view(shape).to(DEV), ec.view(shape).to(DEV), z.view(shape).to(DEV)
    out = ops.p_sample_step_spaced(xd, ed, zd, rows, k_dev)
    assert out is xd and same_bits(xd.flatten(), _run(hip, _rows(1.0), k, x, ec, eu, z, None, 1)[0])
    x2, e2 = torch.cat([x, x]).view(6, 1, 16, 16).to(DEV), torch.cat([ec, eu]).view(6, 1, 16, 16).to(DEV)
    out = ops.p_sample_step_spaced(x2, e2, zd, rows, k_dev, 3.0, clip=False)
    assert out is x2 and torch.equal(x2[:3], x2[3:])
    assert same_bits(x2.view(2, n), _run(hip, _rows(1.0), k, x, ec, eu, z, 3.0, 0))
    xd = x.view(shape).to(DEV)
    for bad in (lambda: ops.p_sample_step_spaced(xd.double(), ed, zd, rows, k_dev),
                lambda: ops.p_sample_step_spaced(xd, ed[:2].contiguous(), zd, rows, k_dev),
                lambda: ops.p_sample_step_spaced(xd, ed, zd[:2].contiguous(), rows, k_dev),
                lambda: ops.p_sample_step_spaced(xd, ed, zd, rows[:, :3].contiguous(), k_dev),
                lambda: ops.p_sample_step_spaced(xd, ed, zd, rows.flatten(), k_dev),
                lambda: ops.p_sample_step_spaced(xd, ed, zd, rows, k_dev.long()),
                lambda: ops.p_sample_step_spaced(xd, ed, zd, rows, k_dev.cpu()),
                lambda: ops.p_sample_step_spaced(x2, ed, zd, rows, k_dev, 3.0),
                lambda: ops.p_sample_step_spaced(x2, e2, zd[:2].contiguous(), rows, k_dev, 3.0),
                lambda: ops.p_sample_step_spaced(xd[:, :, :, :15], ed, zd, rows, k_dev)):
        with pytest.raises(RhoHipError):
            bad()
    assert same_bits(xd.flatten(), x)                           # nothing was launched
    taus = torch.tensor([3, 11, 17], dtype=torch.int32, device=DEV)
    t_dev = torch.tensor([17], dtype=torch.int32, device=DEV)
    off = torch.zeros(1, dtype=torch.int64, device=DEV)
    k_dev.fill_(2)
    ops.spaced_advance(k_dev, t_dev, taus, off, 7)
    assert (int(k_dev.item()), int(t_dev.item()), int(off.item())) == (1, 11, 7)
    ops.spaced_advance(k_dev, t_dev, taus, None, 7)
    assert (int(k_dev.item()), int(t_dev.item()), int(off.item())) == (0, 3, 7)
    for bad in (lambda: ops.spaced_advance(k_dev.long(), t_dev, taus, off, 7),
                lambda: ops.spaced_advance(k_dev, t_dev.long(), taus, off, 7),
                lambda: ops.spaced_advance(k_dev, t_dev, taus.long(), off, 7),
                lambda: ops.spaced_advance(k_dev, t_dev, taus.cpu(), off, 7),
                lambda: ops.spaced_advance(k_dev, t_dev, taus, off.int(), 7)):
        with pytest.raises(RhoHipError):
            bad()
    assert (int(k_dev.item()), int(t_dev.item()), int(off.item())) == (0, 3, 7)
