"""-m gpu: rho_p_sample_step_cfg, the guided reverse update, at the sizes, tails and alignments where a streaming kernel goes wrong
(the manner of test_gpu_streaming_edges.py).

x2 = [2, n] sits between 64 sentinel elements on either side with nothing between its rows: row 1 starts n elements behind row 0, so
only n % 4 == 0 (with 16-byte aligned bases) takes the 16-byte form, every other n or pointer the scalar loop - which must give the
same bits.  Sizes 1 ... 1029, 1032, one scalar and one 16-byte size that need a SECOND trip of the grid-stride loop (2048 blocks x
256 threads) and end inside a block.

Reference: the same expression in float64 on the float32 inputs,
    g = e_u + s * (e_c - e_u);   clamp(c0 * (x - c1 * g) + c2 * z, -1, 1),
z dropped for t <= 1 or z = NULL, nothing written for t = 0.  Two bars: the rel-L2 of the p_sample_step test (2e-6) and a
per-element bound 4 * 2^-24 * sum |terms|, sum |terms| = c0 * (|x| + c1 * (|s| * (|e_c| + |e_u|) + |e_u|)) + |c2 * z|.  The kernel's
expression PSampleOp(x, fma(s, e_c - e_u, e_u), z), of coefficients c0, c1, c2, rounds five times: d = e_c - e_u, g = fma(s, d, e_u),
i = fma(-c1, g, x), c2 * z, fma(c0, i, c2 * z).  To first order their errors reach the result as
    c0 c1 |s| U|d|  +  c0 c1 U|g|  +  c0 U|i|  +  U|c2 z|  +  U|result|
with |d| <= |e_c| + |e_u|, |g| <= |s| (|e_c| + |e_u|) + |e_u|, |i| <= |x| + c1 |g|, |result| <= c0 |i| + |c2 z|: at most
U * (4 T_e + 2 T_x + 2 T_z) <= 4 U * (T_e + T_x + T_z) for the three groups of terms above (the clamp is exact and 1-Lipschitz)."""
import functools

import pytest
import torch

from helpers import det_normal, rel_l2
from gpu_util import DEV, Guarded, check_bound, same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
T = 1000
SMALL = [1, 3, 4, 5, 255, 257, 1029]
WRAP_SCALAR = 525_065              # n % 4 == 1: scalar loop, 524288 threads -> second trip of 777 elements
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
    return det_normal((POOL,), "cfgstep_" + salt)


def _inputs(n):
    """x (the scale of a half-denoised sample: the clamp bites on some elements only), e_c, e_u (correlated, as two predictions of
    one network are), z."""
    ec = _pool("ec")[:n]
    return _pool("x")[:n] * 0.7, ec, 0.8 * ec + 0.3 * _pool("eu")[:n], _pool("z")[:n]


@functools.lru_cache(maxsize=None)
def _coef():
    from rho_diffusion_amd.diffusion.schedule import LinearSchedule
    return LinearSchedule(T, 1e-3, 0.02).device_tables("cpu")["coef"].clone()       # float32 [T, 3]


def _run(hip, x, ec, eu, z, t, scale, shifts=frozenset(), row1=None):
    """Launch on guarded copies; returns the [2, n] result.  Inputs must come back unchanged, every sentinel intact."""
    n = x.numel()
    x2 = torch.cat([x, x if row1 is None else row1])
    e2 = torch.cat([ec, eu])
    gx, ge = Guarded(x2, int("x2" in shifts)), Guarded(e2, int("eps2" in shifts))
    gz = Guarded(z, int("z" in shifts)) if z is not None else None
    coef = _coef().to(DEV)
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    hip.check(hip.lib().rho_p_sample_step_cfg(gx.ptr, ge.ptr, gz.ptr if gz else None, coef.data_ptr(), t_dev.data_ptr(), scale, n,
                                              hip.stream()), "rho_p_sample_step_cfg")
    res = gx.cpu().view(2, n)
    assert gx.intact() and ge.intact() and (gz is None or gz.intact()), (n, t, scale, sorted(shifts))
    assert torch.equal(ge.cpu(), e2) and (gz is None or torch.equal(gz.cpu(), z))
    assert int(t_dev.item()) == t
    return res


def _ref(x, ec, eu, z, t, scale):
    c0, c1, c2 = (float(v) for v in _coef()[t].double())
    x, ec, eu = x.double(), ec.double(), eu.double()
    g = eu + scale * (ec - eu)
    zz = z.double() * c2 if (z is not None and t > 1) else torch.zeros_like(x)
    ref = (c0 * (x - c1 * g) + zz).clamp(-1.0, 1.0)
    terms = abs(c0) * (x.abs() + abs(c1) * (abs(scale) * (ec.abs() + eu.abs()) + eu.abs())) + zz.abs()
    return ref, 4 * U * terms


def _step(hip, x, e, z, t):
    """rho_p_sample_step on a plain copy (its own edges are test_gpu_streaming_edges.py's business)."""
    xd, ed = x.to(DEV).clone(), e.to(DEV)
    zd = z.to(DEV) if z is not None else None
    coef = _coef().to(DEV)
    t_dev = torch.tensor([t], dtype=torch.int32, device=DEV)
    hip.check(hip.lib().rho_p_sample_step(xd.data_ptr(), ed.data_ptr(), zd.data_ptr() if zd is not None else None, coef.data_ptr(),
                                          t_dev.data_ptr(), x.numel(), hip.stream()), "rho_p_sample_step")
    return xd.cpu()


@pytest.mark.parametrize("n", SMALL + [1032, WRAP_SCALAR, WRAP_VEC])
def test_p_sample_step_cfg_sizes(hip, n):
    x, ec, eu, z = _inputs(n)
    for t in (T - 1, 2, 1):
        for zz in (z, None):
            for scale in SCALES:
                if n > 1032 and (t, scale) not in ((T - 1, 3.0), (2, -0.5), (1, 1.0), (T - 1, 0.0)):
                    continue                                   # the wrap sizes: every t, scale and z form once, not the product
                got = _run(hip, x, ec, eu, zz, t, scale)
                ref, bound = _ref(x, ec, eu, zz, t, scale)
                what = ("p_sample_step_cfg", n, t, zz is not None, scale)
                check_bound(got[0], ref, bound, what, 2e-6)
                assert same_bits(got[1], got[0]), what        # the second row is the first, bit for bit
                assert (got[0] != x).any(), what
    # t = 0: no update - both rows (row 1 made different here) and the sentinels stay as they were
    other = x + 1.0
    for zz in (z, None):
        got = _run(hip, x, ec, eu, zz, 0, 3.0, row1=other)
        assert same_bits(got[0], x) and same_bits(got[1], other), (n, zz is not None)


@pytest.mark.parametrize("n", [1029, 1032, WRAP_VEC])
def test_p_sample_step_cfg_alignment(hip, n):
    """Operands offset by 4 bytes take the scalar loop: the bits of the aligned run (16-byte form at 1032 and the wrap size),
    both are loops of step_walk over PSampleOp."""
    x, ec, eu, z = _inputs(n)
    t, scale = 500, 3.0
    base = _run(hip, x, ec, eu, z, t, scale)
    ref, bound = _ref(x, ec, eu, z, t, scale)
    check_bound(base[0], ref, bound, ("aligned", n), 2e-6)
    for shifts in [frozenset([s]) for s in ("x2", "eps2", "z")] + [frozenset(("x2", "eps2", "z"))]:
        got = _run(hip, x, ec, eu, z, t, scale, shifts)
        assert same_bits(got, base), (n, sorted(shifts))
        got0 = _run(hip, x, ec, eu, z, 0, scale, shifts)
        assert same_bits(got0[0], x) and same_bits(got0[1], x), (n, sorted(shifts))


@pytest.mark.parametrize("n", [257, 1032, WRAP_SCALAR])
def test_scale_one_and_zero_against_the_unguided_step(hip, n):
    """scale = 1 is the conditional model and scale = 0 the unconditional one: the guided kernel against rho_p_sample_step on e_c /
    on e_u.  g = fma(1, e_c - e_u, e_u) is e_c only up to two roundings, so no bit equality is claimed: each kernel lies within its
    own bound of the same float64 value (p_sample_step: 4 * 2^-24 * sum |terms|, test_gpu_streaming_edges.py), so the two differ by at
    most the sum of the two bounds."""
    x, ec, eu, z = _inputs(n)
    for t, zz in ((T - 1, z), (2, z), (1, z), (T - 1, None)):
        c0, c1, c2 = (float(v) for v in _coef()[t].double())
        for scale, e in ((1.0, ec), (0.0, eu)):
            got = _run(hip, x, ec, eu, zz, t, scale)[0].double()
            plain = _step(hip, x, e, zz, t).double()
            ref, bound = _ref(x, ec, eu, zz, t, scale)
            zt = (z.double() * c2).abs() if (zz is not None and t > 1) else torch.zeros_like(ref)
            bound_plain = 4 * U * (abs(c0) * (x.double().abs() + (c1 * e.double()).abs()) + zt)
            excess = (got - plain).abs() - (bound + bound_plain)
            assert float(excess.max()) <= 0.0, (n, t, scale, float(excess.max()))
            assert rel_l2(got, plain) < 2e-6, (n, t, scale)


def test_wrapper_checks_shapes_and_updates_both_halves(hip):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    n = 3 * 16 * 16
    x, ec, eu, z = _inputs(n)
    coef = _coef().to(DEV)
    t_dev = torch.tensor([500], dtype=torch.int32, device=DEV)
    x2 = torch.cat([x, x]).view(6, 1, 16, 16).to(DEV)
    e2 = torch.cat([ec, eu]).view(6, 1, 16, 16).to(DEV)
    out = ops.p_sample_step_cfg(x2, e2, z.view(3, 1, 16, 16).to(DEV), coef, t_dev, 3.0)
    assert out is x2
    assert same_bits(x2.view(2, n)[0], _run(hip, x, ec, eu, z, 500, 3.0)[0]) and torch.equal(x2[:3], x2[3:])
    with pytest.raises(RhoHipError):
        ops.p_sample_step_cfg(x2, e2, z.to(DEV)[:-1].contiguous(), coef, t_dev, 3.0)
    with pytest.raises(RhoHipError):
        ops.p_sample_step_cfg(x2, e2[:3].contiguous(), None, coef, t_dev, 3.0)
    # the unguided wrapper checks what the guided one does: z one row of n contiguous elements, t_dev one element on the device
    xd, ed, zd = x.view(3, 1, 16, 16).to(DEV), ec.view(3, 1, 16, 16).to(DEV), z.view(3, 1, 16, 16).to(DEV)
    for bad in (lambda: ops.p_sample_step(xd, ed, zd[:2].contiguous(), coef, t_dev),
                lambda: ops.p_sample_step(xd, ed, zd[:, :, :, :15], coef, t_dev),
                lambda: ops.p_sample_step(xd, ed, zd, coef, t_dev.cpu()),
                lambda: ops.p_sample_step(xd, ed, zd, coef, torch.tensor([500, 500], dtype=torch.int32, device=DEV)),
                lambda: ops.p_sample_step_cfg(x2, e2, zd, coef, t_dev.cpu(), 3.0)):
        with pytest.raises(RhoHipError):
            bad()
    assert same_bits(xd.flatten(), x)                            # nothing was launched
