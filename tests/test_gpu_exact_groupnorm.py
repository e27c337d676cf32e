"""-m gpu: the GroupNorm passes of groupnorm.hip and their conv-fused forms on operands that make every pass exact.

At the C ABI the folded affine (a, b), the statistics (mean, rstd) and the apply coefficients (cA, cP, cQ) are INPUTS of
rho_gn_apply*, rho_gn_bwd_reduce*, rho_gn_bwd_finalize, rho_gn_bwd_apply* and of the conv descriptor's gnb_* / gna_* attachments,
so a test can hand them integers (integer mean, rstd in {0.5, 1, 2}): every product and every fp32 partial sum is then exact in any
order and the kernel must equal the fp64 reference bit for bit.  The forward statistics take integer x: the partial sums are exact,
mean / rstd / a / b are compared per element within a few fp32 ulps counted from the roundings of the code (never a rel-L2 over the
tensor, under which one wrong group or one wrong channel octet passes).  tests/exact_cases.py holds the cases (GN_CASES: the
smallest shapes that reach gpb = 4, KP = 1 / CB = 256, idle threads, a group that spans both concat sources, the block cap of
rho_gn_nblk and the tails of the unrolled loops) and the plain fp64 references; tests/test_exact_cases_host.py proves on the CPU
that the references are exactly representable.  Every output - partials, stats, a, b, cA / cP / cQ, dgamma / dbeta, dfilm, the
scratch rows, dx - lies between guard bands and is prefilled with NaN unless the pass accumulates onto it.

The activation derivatives of the backward passes (dsilu_f / dact_other_f in k_gn_bwd_reduce - both unrolled streams and the tail
loop - and in k_gn_bwd_apply, and dsilu_f in the per-tile rows of a gnb_silu data gradient) are bounded per element in section 6b
and beside the gnb_* test; the forward codes 1 - 6 in section 3.  rho_groupnorm_act (the legacy UNet) and rho_layernorm_* have
their own files (test_gpu_exact_v1_tail.py, test_gpu_exact_layernorm.py), SiLU inside the conv loaders is in test_gpu_exact_conv.py
and test_gpu_exact_backward.py; dsilu_f on the stored output of the gna_* skip data gradient (gnb_silu = 1, the form the training
plan launches behind a SiLU) is judged per element in section 8."""
import math

import pytest
import torch

import exact_cases as X
from exact_cases import BF16, F32
import embed_cases as EC
from exact_util import (assert_bf16_tie_rule, assert_bit_equal, assert_within_abs, assert_within_ulps, bf16_store_bound, check_bf16_exact, check_f32_exact,
                        check_f32_grid, f32_ulp, guarded, guarded_copy, guards_intact)
from detdata import det_normal

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- bounds (fp32 ulps of the fp64 reference value, per element) ------------------------------------------------------------
# mean, rstd: the kernel combines exact integer sums in fp64 (error far below half an fp32 ulp) and rounds once to fp32, so only
# that final rounding can differ from the fp64 reference rounded to fp32: at most 1 ulp by derivation.  Measured on an MI355X: in
# every GN_CASES case (both dtypes, with and without FiLM, rho_gn_finalize and rho_gn_finalize2) and in every synthetic-partial
# case of the format test, mean and rstd EQUAL the rounded reference, so the bound is tightened to what was measured: 0 ulps from
# the fp64 reference rounded to fp32.  (This equality is measured for these inputs, not guaranteed: the kernel's one-pass
# sq / cnt - mean^2 and the reference's two-pass variance are different fp64 values that can fall on opposite sides of an fp32
# rounding boundary.  A failure by exactly 1 ulp after a change of the OPERANDS means the test data moved, not that the kernel is
# wrong; anything larger, or a failure with unchanged operands, is the kernel's.)
STAT_ULPS = 0
# a = rstd gamma (1 + scale), last loop of k_gn_finalize / k_gn_finalize2.  Each fp32 rounding is a relative error of at most
# u = 2^-24, and u |v| < ulp32(v), so k roundings stay within k ulps of the reference (the second-order terms are below 1e-12 ulp):
#   rstd -> fp32 (1), ga = gamma * rstd (2); with FiLM: sc = 1 + scale (3), av = ga * sc (4).
A_ULPS = {False: 2, True: 4}
# b = (beta - mean rstd gamma)(1 + scale) + shift may cancel, so its roundings are counted against the sum of the magnitudes of
# its terms, Mag = (|beta| + |mean rstd gamma|) |1 + scale| + |shift| >= |b|:
#   t = mean * ga carries mean -> fp32 (1), rstd -> fp32 (2), ga (3) and, where the compiler does not fuse it into the
#   subtraction, its own rounding (4); bv = beta - t rounds once (5): |dbv| <= 5 u (|beta| + |t|).
#   With FiLM: sc (6), the product bv * sc where it is not fused (7), the addition of shift (8).
B_ULPS = {False: 5, True: 8}
# cP, cQ of rho_gn_bwd_finalize: exact numerators divided by M = cpg * S in fp64, rounded to fp32: bit-equal where M is a power of
# two (the host proof shows the quotient fits fp32), else only the final rounding can differ
COEF_ULPS = {True: 0, False: 1}

DROP_P, DROP_SEED, DROP_CTR = 0.5, 0x9E3779B97F4A7C15, 2 ** 33 + 5          # inv_keep = 2 exactly; a counter above 2^32


def _dn(dtype):
    return "bf16" if dtype == BF16 else "f32"


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@pytest.fixture(scope="module")
def ops(hip):
    from rho_diffusion_amd.engine import ops as o
    return o


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


def sources(x, c1, dtype):
    """x [N, S, C] on the CPU -> (x1 [N, S, c1], x2 [N, S, C - c1] or None) on the device."""
    return dev(x[..., :c1], dtype), (dev(x[..., c1:], dtype) if x.shape[-1] > c1 else None)


def bits_equal(u, v):
    return torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


def drop_mask(hip, shape):
    """The multipliers (0 or 2, float64 on the CPU) of the *_drop passes over a tensor of `shape`, from rho_dropout_mask (pinned
    against the numpy Philox reference by test_gpu_philox.py), and the device counter the passes read."""
    n = math.prod(shape)
    ctr = torch.tensor([DROP_CTR], dtype=torch.int64, device=DEV)
    out = torch.full((n,), 0xAB, dtype=torch.uint8, device=DEV)
    hip.check(hip.lib().rho_dropout_mask(out.data_ptr(), n, DROP_P, DROP_SEED, ctr.data_ptr(), hip.stream()), "rho_dropout_mask")
    m = out.cpu()
    assert bool((m <= 1).all())
    return 2.0 * m.double().reshape(shape), ctr


GN_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.GN_CASES for dt in c["dtypes"]]


# ----------------------------------------------------------------------------- 1. statistics and the folded affine
def _finalize(hip, which, parts, c, film, S):
    """rho_gn_finalize (which = 1) or rho_gn_finalize2 (which = 2; parts = [(partials, fmt, nblk, channels), ...]) into guarded,
    NaN-prefilled stats / a / b."""
    N, C = c["N"], c["C"]
    L = hip.lib()
    bufs = [guarded((N, 32, 2), F32), guarded((N, C), F32), guarded((N, C), F32)]
    (sf, st), (af, a), (bf, b) = bufs
    scale, shift = (film, film[:, C:]) if film is not None else (None, None)
    fs = 2 * C if film is not None else 0
    ga, be = c["_gamma"], c["_beta"]
    if which == 1:
        (p, _, nblk, _), = parts
        hip.check(L.rho_gn_finalize(p.data_ptr(), N, C, S, nblk, ga.data_ptr(), be.data_ptr(), hip.ptr(scale), hip.ptr(shift), fs,
                                    st.data_ptr(), a.data_ptr(), b.data_ptr(), hip.stream()), "rho_gn_finalize")
    else:
        p1, f1, n1, c1 = parts[0]
        p2, f2, n2, c2 = parts[1] if len(parts) > 1 else (None, 0, 0, 0)
        hip.check(L.rho_gn_finalize2(p1.data_ptr(), f1, n1, c1, hip.ptr(p2), f2, n2, c2, N, S, ga.data_ptr(), be.data_ptr(),
                                     hip.ptr(scale), hip.ptr(shift), fs, st.data_ptr(), a.data_ptr(), b.data_ptr(), hip.stream()),
                  "rho_gn_finalize2")
    torch.cuda.synchronize()
    assert all(guards_intact(f) for f, _ in bufs), "store outside stats / a / b"
    return st, a, b


def _check_fold(st, a, b, mean, rstd, o, film, what, stat_ulps):
    """stats, a, b of one finalize against the fp64 chain (mean / rstd: against its rounding to fp32); returns the largest errors
    met, in their units."""
    C = o["gamma"].numel()
    worst = dict(mean=assert_within_ulps(st[..., 0], mean.float().double(), stat_ulps, what + ": stats[..., 0] = mean [N, 32]"),
                 rstd=assert_within_ulps(st[..., 1], rstd.float().double(), stat_ulps, what + ": stats[..., 1] = rstd [N, 32]"))
    f = o["film"] if film else None
    wa, wb, mag = X.gn_fold_reference(mean, rstd, o["gamma"], o["beta"], None if f is None else f[:, :C], None if f is None else f[:, C:])
    worst["a"] = assert_within_ulps(a, wa, A_ULPS[film], what + ": a [N, C]")
    worst["b"] = assert_within_ulps(b, wb, B_ULPS[film], what + ": b [N, C] (ulps of the summed term magnitudes)", mag=mag)
    return worst


@pytest.mark.parametrize("c,dtype", GN_PARAMS)
def test_statistics_and_folded_affine(hip, cache, c, dtype):
    """rho_gn_partial -> rho_gn_finalize and -> rho_gn_finalize2 on integer x (+-4 plus an integer offset per group): the partials
    summed over the blocks equal the integer channel sums and sums of squares bit for bit; mean and rstd per element against the
    fp64 two-pass reference rounded to fp32; a and b per element against the fp64 fold, without and with FiLM rows (film_stride = 2C); the two
    finalize kernels agree bit for bit on the same partials (one source of C channels, and one partial buffer per source where
    both widths are multiples of 32)."""
    o = cache(("st", c["name"]), lambda: X.gn_stats_operands(c))
    r = cache(("str", c["name"]), lambda: X.gn_stats_reference(o["x"]))
    N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
    check_f32_exact(r["sumsq"], "sums of squares")
    L = hip.lib()
    nblk = int(L.rho_gn_nblk(S))
    assert nblk == X.gn_nblk(S)
    x1, x2 = sources(o["x"], c1, dtype)
    pf, part = guarded((N, nblk, C // 8, 16), F32)
    hip.check(L.rho_gn_partial(x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, part.data_ptr(), hip.stream()), "rho_gn_partial")
    torch.cuda.synchronize()
    what = f"{c['name']} {_dn(dtype)}"
    assert guards_intact(pf), what + ": store outside the partials"
    pc = part.cpu().double()
    assert_bit_equal(pc[..., :8].reshape(N, nblk, C).sum(1), r["sum"], what + ": partial sums over the blocks [N, C]")
    assert_bit_equal(pc[..., 8:].reshape(N, nblk, C).sum(1), r["sumsq"], what + ": partial sums of squares over the blocks [N, C]")
    cc = dict(c, _gamma=dev(o["gamma"]), _beta=dev(o["beta"]))
    film_d = dev(o["film"])
    two = None
    if c2 and c1 % 32 == 0 and c2 % 32 == 0:                     # one partial buffer per source
        two = []
        for xs, cs in ((x1, c1), (x2, c2)):
            f, p = guarded((N, nblk, cs // 8, 16), F32)
            hip.check(L.rho_gn_partial(xs.data_ptr(), cs, None, 0, hip.dtype_code(dtype), N, S, p.data_ptr(), hip.stream()), "rho_gn_partial")
            two.append((f, p, cs))
    for film in (False, True):
        fd = film_d if film else None
        st, a, b = _finalize(hip, 1, [(part, 0, nblk, C)], cc, fd, S)
        worst = _check_fold(st, a, b, r["mean"], r["rstd"], o, film, f"{what} finalize film={film}", STAT_ULPS)
        print(f"gn stats {what} film={int(film)}: max error mean {worst['mean']:.3g} rstd {worst['rstd']:.3g} a {worst['a']:.3g} "
              f"b {worst['b']:.3g} ulps (bounds {STAT_ULPS} {STAT_ULPS} {A_ULPS[film]} {B_ULPS[film]})")
        st2, a2, b2 = _finalize(hip, 2, [(part, 0, nblk, C)], cc, fd, S)
        assert bits_equal(st, st2) and bits_equal(a, a2) and bits_equal(b, b2), what + ": rho_gn_finalize2 differs from rho_gn_finalize"
        if two:
            assert all(guards_intact(f) for f, _, _ in two)
            st3, a3, b3 = _finalize(hip, 2, [(p, 0, nblk, cs) for _, p, cs in two], cc, fd, S)
            assert bits_equal(st, st3) and bits_equal(a, a3) and bits_equal(b, b3), what + ": two-source rho_gn_finalize2 differs"


def test_one_pass_variance_at_a_large_mean(hip):
    """f32 inputs 64 + N(0, 1) at (2, 64, 0, 1600): rstd of the one-pass form var = E[x^2] - mean^2 against a two-pass fp64
    reference.  Bound: C = 64 gives OCT = 8, ppi = 32, nblk = 7, per = 229, so a thread adds at most ceil(229 / 32) = 8 terms in fp32
    and the LDS pass adds ppi = 32 lane totals; all terms of either sum have one sign, so every rounding is at most 2^-24 of the
    final block total and each of sum x, sum x^2 carries a relative error of at most d = (8 + 32) 2^-24 (the fp64 combine adds
    nothing).  Then |dvar| <= d E[x^2] + 2 d mean^2 <= 3 d E[x^2], i.e. a relative error r = 3 d E[x^2] / (var + eps) of var + eps
    (E[x^2] / var ~ 4097 here: r ~ 0.029), and rstd = (var + eps)^-1/2 is off by at most 1 / sqrt(1 - r) - 1 ~ 1.5 % (plus its own
    rounding to fp32).  Measured on an MI355X: 2.4e-4."""
    N, C, S = 2, 64, 1600
    x = 64.0 + det_normal((N, S, C), "gn_onepass")
    r = X.gn_stats_reference(x)
    L = hip.lib()
    nblk = int(L.rho_gn_nblk(S))
    ppi = 256 // (C // 8)
    per = -(-S // nblk)
    d = (-(-per // ppi) + ppi) * 2.0 ** -24
    xg = x.double().reshape(N, S, 32, C // 32)
    e2, var = (xg * xg).mean((1, 3)), xg.var((1, 3), unbiased=False)
    rr = 3 * d * e2 / (var + X.GN_EPS)
    bound = (1.0 / torch.sqrt(1.0 - rr) - 1.0 + 2.0 ** -23) * r["rstd"]
    xd = dev(x)
    pf, part = guarded((N, nblk, C // 8, 16), F32)
    hip.check(L.rho_gn_partial(xd.data_ptr(), C, None, 0, hip.dtype_code(F32), N, S, part.data_ptr(), hip.stream()), "rho_gn_partial")
    cc = dict(N=N, C=C, _gamma=torch.ones(C, device=DEV), _beta=torch.zeros(C, device=DEV))
    st, _, _ = _finalize(hip, 1, [(part, 0, nblk, C)], cc, None, S)
    assert guards_intact(pf)
    worst = assert_within_abs(st[..., 1], r["rstd"], bound, "rstd of 64 + N(0, 1) [N, 32]")
    rel = float(((st[..., 1].cpu().double() - r["rstd"]).abs() / r["rstd"]).max())
    print(f"one-pass variance: max relative error of rstd {rel:.3e} (abs {worst:.3e}); derived bound {float((bound / r['rstd']).max()):.3e}")
    assert_within_abs(st[..., 0], r["mean"], 2 * d * r["mean"].abs(), "mean of 64 + N(0, 1) [N, 32]")


# ----------------------------------------------------------------------------- 2. rho_gn_finalize2 formats
@pytest.mark.parametrize("N,c1,c2,nb1,nb2", X.GN_FIN2_CASES)
def test_finalize2_formats_agree_and_match_fp64(hip, N, c1, c2, nb1, nb2):
    """Synthetic integer partials written in both layouts (fmt 0 [n][nblk][C/8][16], fmt 1 [n][tiles][2][C]): one source of c1 + c2
    channels as (0) and (1), two sources of c1 and c2 channels with different block counts as (0,0), (1,0), (0,1), (1,1).  40 + 56
    channels (cpg = 3: a group spans both sources) at block counts 1 (fewer blocks than the KP lanes of a channel), 3 and 1025
    (many blocks per lane), N = 3 (gpb = 1) and N = 32 (gpb = 4); the wide cases at N = 32 are the ones that reach KP = 1 with
    CB = 256 (C = 2048) and CB = 132 with idle threads (C = 1056) in k_gn_finalize2 - see GN_FIN2_CASES.  mean / rstd / a / b are
    bit-equal between the formats and within the bounds of the fp64 chain (mean / rstd: equal to its rounding to fp32)."""
    o = X.gn_fin2_operands(N, c1, c2, nb1, nb2)
    C, S = o["C"], o["S"]
    cc = dict(N=N, C=C, _gamma=dev(o["gamma"]), _beta=dev(o["beta"]))
    film = dev(o["film"])

    def lay(key, fmt):
        return dev((X.partials_fmt1 if fmt else X.partials_fmt0)(o["s" + key], o["q" + key]))

    for srcs, keys in (((c1, c2), ("1", "2")), ((C,), ("0",))):
        nbs = (nb1, nb2)
        sums = torch.cat([o["s" + k].double().sum(1) for k in keys], 1)
        sq = torch.cat([o["q" + k].double().sum(1) for k in keys], 1)
        mean, rstd = X.gn_moments_reference(sums, sq, S)
        first = None
        for fmts in ([(0, 0), (1, 0), (0, 1), (1, 1)] if len(keys) == 2 else [(0,), (1,)]):
            parts = [(lay(k, f), f, nb, cs) for k, f, nb, cs in zip(keys, fmts, nbs, srcs)]
            st, a, b = _finalize(hip, 2, parts, cc, film, S)
            what = f"finalize2 N={N} channels={srcs} blocks={nbs[:len(keys)]} fmt={fmts}"
            if first is None:
                first = (st, a, b)
                worst = _check_fold(st, a, b, mean, rstd, o, True, what, STAT_ULPS)
                print(f"gn {what}: max error mean {worst['mean']:.3g} rstd {worst['rstd']:.3g} a {worst['a']:.3g} b {worst['b']:.3g} ulps")
            else:
                assert all(bits_equal(u, v) for u, v in zip(first, (st, a, b))), what + ": differs from fmt 0"


# ----------------------------------------------------------------------------- 3. rho_gn_apply / rho_gn_apply_drop
@pytest.mark.parametrize("c,dtype", GN_PARAMS)
def test_apply_is_bit_exact(hip, cache, c, dtype):
    """Integer a in +-2, b in +-3, x in +-4, act code 0: y = a x + b bit for bit; with dropout at p = 0.5 (inv_keep = 2, a device
    counter above 2^32) y = 2 mask (a x + b) with the mask of rho_dropout_mask."""
    o = cache(("ap", c["name"]), lambda: X.gn_apply_operands(c))
    want = cache(("apr", c["name"]), lambda: X.gn_apply_reference(o["x"], o["a"], o["b"]))
    N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
    check_bf16_exact(2 * want, "dropout(a x + b)")
    L = hip.lib()
    x1, x2 = sources(o["x"], c1, dtype)
    a, b = dev(o["a"]), dev(o["b"])
    what = f"{c['name']} {_dn(dtype)}"
    yf, y = guarded((N, S, C), dtype)
    hip.check(L.rho_gn_apply(x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), 0, y.data_ptr(),
                             hip.stream()), "rho_gn_apply")
    torch.cuda.synchronize()
    assert guards_intact(yf), what + ": store outside y"
    assert_bit_equal(y.float(), want, what + ": rho_gn_apply [N, S, C]")
    mask, ctr = drop_mask(hip, (N, S, C))
    yf, y = guarded((N, S, C), dtype)
    hip.check(L.rho_gn_apply_drop(x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), 0, y.data_ptr(),
                                  DROP_P, DROP_SEED, ctr.data_ptr(), hip.stream()), "rho_gn_apply_drop")
    torch.cuda.synchronize()
    assert guards_intact(yf), what + ": store outside y (drop)"
    assert_bit_equal(y.float(), mask * want, what + ": rho_gn_apply_drop [N, S, C]")
    assert int(ctr.item()) == DROP_CTR


def _act32(u, code):
    """The kernels' expressions (common.h silu_f / act_other_f) evaluated by torch in fp32 on the CPU."""
    if code == 1:
        return u * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * u)))
    if code == 2:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if code == 3:
        return 0.5 * u * (1.0 + torch.erf(u * 0.70710678118654752))
    if code == 4:
        return torch.tanh(u)
    if code == 5:
        return 1.0 / (1.0 + torch.exp(-u))
    return torch.where(u > 0, u, torch.expm1(u))


def _act64(u, code):
    if code == 1:
        return u * torch.sigmoid(u)
    if code == 2:
        return u.clamp_min(0.0)
    if code == 3:
        return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    if code == 4:
        return torch.tanh(u)
    if code == 5:
        return torch.sigmoid(u)
    return torch.where(u > 0, u, torch.expm1(u))


def _half_bf16_ulp(v):
    """Half the spacing of bf16 numbers at |v|: 2^(floor(log2 |v|) - 8); 0 at 0."""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 9))


ACT_NAMES = {1: "silu", 2: "relu", 3: "gelu", 4: "tanh", 5: "sigmoid", 6: "elu"}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("code", sorted(ACT_NAMES), ids=[ACT_NAMES[k] for k in sorted(ACT_NAMES)])
def test_apply_activation_codes_per_element(hip, code, dtype):
    """Act code 1 (SiLU) and every other code of the activation registry on non-integer inputs, per element against fp64.
    Bound (not taken from the kernel): the same expression evaluated by torch in fp32 on the CPU has a largest per-element error
    `base` against fp64 on these very inputs; 8 x base is allowed (the hardware exp / rcp are good to about 1 ulp each), plus half a
    bf16 ulp of the result where the output is stored as bf16.  Measured on an MI355X (base -> GPU maximum, f32): SiLU 8.4e-7 ->
    6.8e-7, ReLU and ELU 4.5e-7 -> 2.4e-7, GELU 6.7e-7 -> 6.4e-7, tanh 8.1e-8 -> 8.7e-8, sigmoid 8.8e-8 -> 8.8e-8; bf16: at most
    8.1e-8 beyond the half ulp of the store."""
    for name in ("cpg3_straddle", "nblk2_tails"):
        c = X.GN_BY_NAME[name]
        N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
        x = (1.5 * det_normal((N, S, C), "gnact_x" + name)).to(dtype).float()
        a, b = 1 + 0.3 * det_normal((N, C), "gnact_a" + name), 0.2 * det_normal((N, C), "gnact_b" + name)
        want = _act64(a.double().unsqueeze(1) * x.double() + b.double().unsqueeze(1), code)
        base = float((_act32(a.unsqueeze(1) * x + b.unsqueeze(1), code).double() - want).abs().max())
        bound = torch.full_like(want, 8 * base)
        if dtype == BF16:
            bound = bound + _half_bf16_ulp(want)
        x1, x2 = sources(x, c1, dtype)
        ad, bd = dev(a), dev(b)
        yf, y = guarded((N, S, C), dtype)
        hip.check(hip.lib().rho_gn_apply(x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, ad.data_ptr(), bd.data_ptr(), code,
                                         y.data_ptr(), hip.stream()), "rho_gn_apply")
        torch.cuda.synchronize()
        assert guards_intact(yf)
        err = (y.float().cpu().double() - want).abs()
        if dtype == BF16:                                                      # (the part of the error the bf16 store does not explain)
            err = (err - _half_bf16_ulp(want)).clamp_min(0.0)
        print(f"gn apply act {ACT_NAMES[code]} {_dn(dtype)} {name}: CPU fp32 base error {base:.3e}, bound 8 x = {8 * base:.3e}, "
              f"GPU max error{' beyond half a bf16 ulp' if dtype == BF16 else ''} {float(err.max()):.3e}")
        assert_within_abs(y.float(), want, bound, f"rho_gn_apply act={ACT_NAMES[code]} {_dn(dtype)} {name} [N, S, C]")


# ----------------------------------------------------------------------------- 4. reduce -> finalize (fmt 0)
def _bwd_finalize(hip, part, nblk, fmt, N, C, S, o, film, dgamma0=None, dbeta0=None):
    """rho_gn_bwd_finalize into guarded buffers (NaN-prefilled; dgamma / dbeta prefilled with integers when accumulating)."""
    L = hip.lib()
    acc = dgamma0 is not None
    B = dict(work=guarded((2, N, C), F32), cA=guarded((N, C), F32), cP=guarded((N, 32), F32), cQ=guarded((N, 32), F32),
             dfilm=guarded((N, 2 * C), F32),
             dgamma=guarded_copy(dgamma0, F32) if acc else guarded((C,), F32), dbeta=guarded_copy(dbeta0, F32) if acc else guarded((C,), F32))
    v = {k: t[1] for k, t in B.items()}
    scale = o["_film"] if film else None
    hip.check(L.rho_gn_bwd_finalize(part.data_ptr(), N, C, S, nblk, fmt, o["_gamma"].data_ptr(), o["_beta"].data_ptr(), hip.ptr(scale),
                                    2 * C if film else 0, o["_stats"].data_ptr(), v["work"].data_ptr(), v["dgamma"].data_ptr(),
                                    v["dbeta"].data_ptr(), int(acc), v["dfilm"].data_ptr() if film else None,
                                    v["dfilm"][:, C:].data_ptr() if film else None, 2 * C, v["cA"].data_ptr(), v["cP"].data_ptr(),
                                    v["cQ"].data_ptr(), hip.stream()), "rho_gn_bwd_finalize")
    torch.cuda.synchronize()
    for k, t in B.items():
        assert guards_intact(t[0]), f"store outside {k}"
    if not film:
        assert bool(torch.isnan(v["dfilm"]).all()), "dfilm written without FiLM outputs"
    return v


def _check_coeffs(v, r, C, film, pow2, what, dgamma0=None, dbeta0=None):
    assert_bit_equal(v["work"][0], r["dgamma_n"], what + ": per-sample dgamma rows (scratch) [N, C]")
    assert_bit_equal(v["work"][1], r["dbeta_n"], what + ": per-sample dbeta rows (scratch) [N, C]")
    assert_bit_equal(v["dgamma"], r["dgamma"] + (0 if dgamma0 is None else dgamma0.double()), what + ": dgamma [C]")
    assert_bit_equal(v["dbeta"], r["dbeta"] + (0 if dbeta0 is None else dbeta0.double()), what + ": dbeta [C]")
    if film:
        assert_bit_equal(v["dfilm"][:, :C], r["dscale"], what + ": dscale [N, C]")
        assert_bit_equal(v["dfilm"][:, C:], r["dshift"], what + ": dshift [N, C]")
    assert_bit_equal(v["cA"], r["cA"], what + ": cA [N, C]")
    return (assert_within_ulps(v["cP"], r["cP"], COEF_ULPS[pow2], what + ": cP [N, 32]"),
            assert_within_ulps(v["cQ"], r["cQ"], COEF_ULPS[pow2], what + ": cQ [N, 32]"))


def _bwd_dev(o):
    return dict(o, _gamma=dev(o["gamma"]), _beta=dev(o["beta"]), _film=dev(o["film"]), _stats=dev(o["stats"]))


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
@pytest.mark.parametrize("c,dtype", GN_PARAMS)
def test_backward_reduce_and_finalize_are_bit_exact(hip, cache, c, dtype, drop):
    """rho_gn_bwd_reduce / _drop -> rho_gn_bwd_finalize (fmt 0) on g in +-2, x in +-4, supplied integer mean and rstd in {0.5, 1, 2},
    act code 0, integer gamma / beta and an integer FiLM scale in -2 .. 2: the partials summed over the blocks equal R1 = sum gq and
    R2 = sum gq xhat; dgamma, dbeta (and the per-sample scratch rows), dscale, dshift and cA are bit-equal, cP / cQ bit-equal where
    cpg * S is a power of two and within the final rounding elsewhere.  A second finalize without FiLM accumulates onto integer
    dgamma / dbeta.  drop: g is multiplied by the regenerated p = 0.5 mask (multiplier 2)."""
    o = cache(("bw", c["name"]), lambda: X.gn_bwd_operands(c))
    N, S, C, c1, c2, cpg = c["N"], c["S"], c["C"], c["c1"], c["c2"], c["cpg"]
    L = hip.lib()
    od = _bwd_dev(o)
    g = dev(o["g"], dtype)
    x1, x2 = sources(o["x"], c1, dtype)
    a, b = dev(o["a"]), dev(o["b"])
    nblk = int(L.rho_gn_nblk(S))
    pf, part = guarded((N, nblk, C // 8, 16), F32)
    args = (g.data_ptr(), x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), od["_stats"].data_ptr(), 0,
            part.data_ptr())
    gq = o["g"].double()
    if drop:
        mask, ctr = drop_mask(hip, (N, S, C))
        gq = gq * mask
        hip.check(L.rho_gn_bwd_reduce_drop(*args, DROP_P, DROP_SEED, ctr.data_ptr(), hip.stream()), "rho_gn_bwd_reduce_drop")
    else:
        hip.check(L.rho_gn_bwd_reduce(*args, hip.stream()), "rho_gn_bwd_reduce")
    torch.cuda.synchronize()
    what = f"{c['name']} {_dn(dtype)}{' drop' if drop else ''}"
    assert guards_intact(pf), what + ": store outside the partials"
    scale = o["film"][:, :C]
    r = X.gn_bwd_reference(gq, o["x"], o["mean"], o["rstd"], o["gamma"], o["beta"], scale)
    r0 = X.gn_bwd_coeffs_reference(r["R1"], r["R2"], o["mean"], o["rstd"], o["gamma"], o["beta"], None, S)
    # representability of the references under the mask the kernels drew (the host proof uses a stand-in mask)
    check_f32_exact(r["R1"], "R1")
    check_f32_grid(r["absR2"], 0.5, "sum of |gq xhat|")
    for q in (r, r0):
        for k in ("dscale",):
            check_f32_grid(q[k], 0.5, k)
        check_f32_grid(q["dgamma_n"].abs().sum(0) + o["dgamma0"].abs().double(), 0.5, "running sums of dgamma")
        check_f32_grid(q["dbeta_n"].abs().sum(0) + o["dbeta0"].abs().double(), 0.5, "running sums of dbeta")
    pc = part.cpu().double()
    assert_bit_equal(pc[..., :8].reshape(N, nblk, C).sum(1), r["R1"], what + ": partials over the blocks, R1 = sum gq [N, C]")
    assert_bit_equal(pc[..., 8:].reshape(N, nblk, C).sum(1), r["R2"], what + ": partials over the blocks, R2 = sum gq xhat [N, C]")
    pow2 = X.is_pow2(cpg * S)
    if pow2:
        for k in ("cP", "cQ"):
            assert_bit_equal(r[k].float(), r[k], k + " fits fp32")
    v = _bwd_finalize(hip, part, nblk, 0, N, C, S, od, True)
    wp, wq = _check_coeffs(v, r, C, True, pow2, what + " finalize FiLM")
    v = _bwd_finalize(hip, part, nblk, 0, N, C, S, od, False, o["dgamma0"], o["dbeta0"])
    wp0, wq0 = _check_coeffs(v, r0, C, False, pow2, what + " finalize accumulate", o["dgamma0"], o["dbeta0"])
    print(f"gn bwd finalize {what}: cpg*S = {cpg * S} max error cP {max(wp, wp0):.3g} cQ {max(wq, wq0):.3g} ulps (bound {COEF_ULPS[pow2]})")


# ----------------------------------------------------------------------------- 5. rho_gn_bwd_finalize fmt 1
@pytest.mark.parametrize("N,C,nb", X.GN_FIN1_CASES)
def test_backward_finalize_tile_sums_equal_reduce_partials(hip, N, C, nb):
    """fmt 1: synthetic integer per-tile sum dz and sum dz x ([n][tiles][2][C]) with integer mean and rstd in {0.5, 1, 2} must give
    what fmt 0 gives on R1 = sum dz, R2 = rstd (sum dz x - mean sum dz) per block, bit for bit, and both must equal the fp64
    coefficients.  KP = 256 / (4 cpg) lanes per channel: 1 block (fewer than KP), 1025 blocks, C = 1056 (CB = 132) and 2048 (KP = 1)."""
    o = X.gn_fin1_operands(N, C, nb)
    S, cpg = o["S"], C // 32
    od = _bwd_dev(o)
    mu, rs = X.per_channel(o["mean"], cpg).double(), X.per_channel(o["rstd"], cpg).double()
    r2 = rs * (o["dzx"].double() - mu * o["dz"].double())
    assert_bit_equal(r2.float(), r2, "per-tile R2 fits fp32")
    r = X.gn_bwd_coeffs_reference(o["dz"].double().sum(1), r2.sum(1), o["mean"], o["rstd"], o["gamma"], o["beta"], o["film"][:, :C], S)
    p1 = dev(X.partials_fmt1(o["dz"], o["dzx"]))
    p0 = dev(X.partials_fmt0(o["dz"], r2.float()))
    pow2 = X.is_pow2(cpg * S)
    v1 = _bwd_finalize(hip, p1, nb, 1, N, C, S, od, True)
    v0 = _bwd_finalize(hip, p0, nb, 0, N, C, S, od, True)
    what = f"bwd finalize N={N} C={C} tiles={nb}"
    _check_coeffs(v1, r, C, True, pow2, what + " fmt 1")
    _check_coeffs(v0, r, C, True, pow2, what + " fmt 0")
    for k in ("work", "cA", "cP", "cQ", "dfilm", "dgamma", "dbeta"):
        assert bits_equal(v0[k], v1[k]), f"{what}: {k} differs between fmt 0 and fmt 1"


# ----------------------------------------------------------------------------- 6. rho_gn_bwd_apply / _drop
def _apply_once(hip, c, dtype, o, od, acc1, acc2, add, mask_ctr, what):
    N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
    L = hip.lib()
    g, x1, x2, a, b, cA, cP, cQ = od
    dx0 = o["dx0"]
    f1, dx1 = guarded_copy(dx0[..., :c1], dtype) if acc1 else guarded((N, S, c1), dtype)
    f2 = dx2 = None
    if c2:
        f2, dx2 = guarded_copy(dx0[..., c1:], dtype) if acc2 else guarded((N, S, c2), dtype)
    add1 = dev(o["add1"], dtype) if add else None
    args = (g.data_ptr(), x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), 0, cA.data_ptr(),
            cP.data_ptr(), cQ.data_ptr(), dx1.data_ptr(), hip.ptr(dx2), acc1, acc2, hip.ptr(add1))
    gq = o["g"].double()
    if mask_ctr is not None:
        gq = gq * mask_ctr[0]
        hip.check(L.rho_gn_bwd_apply_drop(*args, DROP_P, DROP_SEED, mask_ctr[1].data_ptr(), hip.stream()), "rho_gn_bwd_apply_drop")
    else:
        hip.check(L.rho_gn_bwd_apply(*args, hip.stream()), "rho_gn_bwd_apply")
    torch.cuda.synchronize()
    want = X.gn_bwd_apply_reference(gq, o["x"], o["cA"], o["cP"], o["cQ"])
    check_bf16_exact(want, "apply term")
    prev = torch.zeros_like(want)
    if acc1:
        prev[..., :c1] += dx0[..., :c1].double()
    if add:
        prev[..., :c1] += o["add1"].double()
    if acc2:
        prev[..., c1:] += dx0[..., c1:].double()
    want = want + prev
    check_bf16_exact(want, "accumulated gradient")
    what = f"{what} acc1={acc1} acc2={acc2} add1={int(add)}{' drop' if mask_ctr is not None else ''}"
    assert guards_intact(f1), what + ": store outside dx1"
    assert_bit_equal(dx1.float(), want[..., :c1], what + ": dx1 [N, S, c1]")
    if c2:
        assert guards_intact(f2), what + ": store outside dx2"
        assert_bit_equal(dx2.float(), want[..., c1:], what + ": dx2 [N, S, c2]")


@pytest.mark.parametrize("c,dtype", GN_PARAMS)
def test_backward_apply_is_bit_exact(hip, cache, c, dtype):
    """dx = cA gq + cP + cQ x with integer cA in +-2, cP in +-3, cQ in +-1 (act code 0) for every combination of acc1, acc2 and a
    present add1 (a case without a second source has no acc2), written into NaN-prefilled or accumulated onto integer gradients; the
    dropout form (gq = 2 mask g) plain and with everything accumulated."""
    o = cache(("bw", c["name"]), lambda: X.gn_bwd_operands(c))
    c1, c2 = c["c1"], c["c2"]
    x1, x2 = sources(o["x"], c1, dtype)
    od = (dev(o["g"], dtype), x1, x2, dev(o["a"]), dev(o["b"]), dev(o["cA"]), dev(o["cP"]), dev(o["cQ"]))
    what = f"bwd apply {c['name']} {_dn(dtype)}"
    for acc1 in (0, 1):
        for acc2 in ((0, 1) if c2 else (0,)):
            for add in (False, True):
                _apply_once(hip, c, dtype, o, od, acc1, acc2, add, None, what)
    mc = drop_mask(hip, (c["N"], c["S"], c["C"]))
    _apply_once(hip, c, dtype, o, od, 0, 0, False, mc, what)
    _apply_once(hip, c, dtype, o, od, 1, int(bool(c2)), True, mc, what)


@pytest.mark.parametrize("dtype,stored", [(BF16, 256.0), (F32, 258.0)], ids=["bf16", "f32"])
def test_backward_apply_adds_the_residual_before_the_term(hip, dtype, stored):
    """The documented order of rho_gn_bwd_apply with acc1 and add1: the residual's gradient joins the running sum first, rounded to
    the storage type, then the term.  dx1 = 256, add1 = 1, term = 1: bf16(256 + 1) = 256, then 256 + 1 rounds to 256 (a single fp32
    sum 256 + 1 + 1 = 258 would be stored as 258); the f32 twin stores 258."""
    N, S, C = 2, 5, 32
    L = hip.lib()
    one = torch.ones(N, S, C)
    g, x, add1 = dev(one, dtype), dev(3 * one, dtype), dev(one, dtype)
    a, b, cA = torch.ones(N, C, device=DEV), torch.zeros(N, C, device=DEV), torch.ones(N, C, device=DEV)
    cP, cQ = torch.zeros(N, 32, device=DEV), torch.zeros(N, 32, device=DEV)
    f1, dx1 = guarded_copy(256 * one, dtype)
    hip.check(L.rho_gn_bwd_apply(g.data_ptr(), x.data_ptr(), C, None, 0, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), 0, cA.data_ptr(),
                                 cP.data_ptr(), cQ.data_ptr(), dx1.data_ptr(), None, 1, 0, add1.data_ptr(), hip.stream()), "rho_gn_bwd_apply")
    torch.cuda.synchronize()
    assert guards_intact(f1)
    want = ((256 * one + one).to(dtype).float() + one).to(dtype).double()
    assert float(want[0, 0, 0]) == stored
    assert_bit_equal(dx1.float(), want, f"rho_gn_bwd_apply {_dn(dtype)}: cvt_round(dx1 + add1) + term")


# ----------------------------------------------------------------------------- 6b. act'(u) in rho_gn_bwd_apply / rho_gn_bwd_reduce
# a = 1, b = 0 make u = fma(1, x, 0) = x exactly; x is embed_cases.code_inputs() tiled over the case (rounded to the storage type
# first).  Bounds per element from embed_cases.hw_act_bound: code 1 is dsilu_f (derived from its expression: w (2 + 0.8 |t|) + 7 ulps
# of s (1 + |x| (1 + s))), codes 2 - 6 are dact_other_f with the ACT_ULPS allowances; a bf16 store adds half a bf16 ulp.
ACT_BWD_CASES = ("nblk2_tails", "cpg3_straddle", "c2048")      # ppi = 32 with odd tails and two blocks; S < ppi and two sources; ppi = 1
ALL_CODES = (1, 2, 3, 4, 5, 6)


def _code_x(shape, dtype):
    src = EC.code_inputs().reshape(-1)
    n = math.prod(shape)
    return src.repeat(-(-n // src.numel()))[:n].reshape(shape).to(dtype).float()


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("code", ALL_CODES, ids=[EC.ACT_NAMES[k] for k in ALL_CODES])
def test_backward_apply_activation_derivative_per_element(hip, code, dtype, drop):
    """cA = 1, cP = cQ = 0, g = 1: dx = fma(1, gq, fma(0, x, 0)) = gq = act'(x) element for element (times the mask's 0 or 2 in the
    dropout form, both exact)."""
    L = hip.lib()
    for name in ACT_BWD_CASES:
        c = X.GN_BY_NAME[name]
        N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
        x = _code_x((N, S, C), dtype)
        x1, x2 = sources(x, c1, dtype)
        g = torch.ones(N, S, C, device=DEV, dtype=dtype)
        a, b, cA = torch.ones(N, C, device=DEV), torch.zeros(N, C, device=DEV), torch.ones(N, C, device=DEV)
        cP, cQ = torch.zeros(N, 32, device=DEV), torch.zeros(N, 32, device=DEV)
        f1, dx1 = guarded((N, S, c1), dtype)
        f2, dx2 = guarded((N, S, c2), dtype) if c2 else (None, None)
        args = (g.data_ptr(), x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), code, cA.data_ptr(),
                cP.data_ptr(), cQ.data_ptr(), dx1.data_ptr(), hip.ptr(dx2), 0, 0, None)
        want, bound, mag = EC.hw_act_bound(x.double(), code, True)
        if drop:
            mask, ctr = drop_mask(hip, (N, S, C))
            want, bound, mag = want * mask, bound * mask, mag * mask
            hip.check(L.rho_gn_bwd_apply_drop(*args, DROP_P, DROP_SEED, ctr.data_ptr(), hip.stream()), "rho_gn_bwd_apply_drop")
        else:
            hip.check(L.rho_gn_bwd_apply(*args, hip.stream()), "rho_gn_bwd_apply")
        torch.cuda.synchronize()
        assert guards_intact(f1) and (f2 is None or guards_intact(f2)), "store outside dx"
        got = torch.cat([dx1, dx2], 2) if c2 else dx1
        what = f"rho_gn_bwd_apply{'_drop' if drop else ''} act'={EC.ACT_NAMES[code]} {_dn(dtype)} {name} [N, S, C]"
        if dtype == F32:
            meas = float(((got.cpu().double() - want).abs() / f32_ulp(mag)).max())
            part = float(((got.cpu().double() - want).abs() / bound.clamp_min(1e-300)).max()) if code != 2 else 0.0
            print(f"measured: {what}: worst {meas:.3f} ulp of the term magnitude, {part:.3f} of the derived bound")
            assert_within_abs(got, want, bound, what)
        else:
            assert_within_abs(got, want, bf16_store_bound(want, bound), what + " (fp32 bound + half a bf16 ulp)")


def _reduce(hip, c, dtype, g, x, stats, code, mask_ctr):
    """rho_gn_bwd_reduce / _drop with a = 1, b = 0 into NaN-prefilled guarded partials; returns (R1, R2) [N, C] summed over the blocks
    in fp64."""
    N, S, C, c1, c2 = c["N"], c["S"], c["C"], c["c1"], c["c2"]
    L = hip.lib()
    nblk = int(L.rho_gn_nblk(S))
    x1, x2 = sources(x, c1, dtype)
    gd, sd = dev(g, dtype), dev(stats)
    a, b = torch.ones(N, C, device=DEV), torch.zeros(N, C, device=DEV)
    pf, part = guarded((N, nblk, C // 8, 16), F32)
    args = (gd.data_ptr(), x1.data_ptr(), c1, hip.ptr(x2), c2, hip.dtype_code(dtype), N, S, a.data_ptr(), b.data_ptr(), sd.data_ptr(), code,
            part.data_ptr())
    if mask_ctr is not None:
        hip.check(L.rho_gn_bwd_reduce_drop(*args, DROP_P, DROP_SEED, mask_ctr[1].data_ptr(), hip.stream()), "rho_gn_bwd_reduce_drop")
    else:
        hip.check(L.rho_gn_bwd_reduce(*args, hip.stream()), "rho_gn_bwd_reduce")
    torch.cuda.synchronize()
    assert guards_intact(pf), "store outside the partials"
    pc = part.cpu().double()
    return pc[..., :8].reshape(N, nblk, C).sum(1), pc[..., 8:].reshape(N, nblk, C).sum(1)


def _reduce_stats(c):
    """Supplied statistics (integer mean, rstd in {0.5, 1, 2}) and the kernel's xhat = fl(fl(x - mean) * rstd), which torch's float32
    gives bit for bit."""
    N = c["N"]
    mean = X.gn_int((N, 32), "gnact_mean" + c["name"], -1, 2)
    rstd = torch.tensor([0.5, 1.0, 2.0])[X.gn_int((N, 32), "gnact_rstd" + c["name"], 0, 2).long()]
    return mean, rstd, torch.stack([mean, rstd], 2)


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("code", ALL_CODES, ids=[EC.ACT_NAMES[k] for k in ALL_CODES])
def test_backward_reduce_activation_derivative_one_term(hip, code, dtype, drop):
    """(a) g = 2 at ONE position per (n, channel) and 0 elsewhere, that position once in each accumulation the shape reaches (the
    unrolled gq and gr streams and the tail loop): every other term is an exact zero, so R1 summed over the blocks is the single
    term 2 act'(x) (the activation allowance alone) and R2 = fl(2 act'(x) * xhat) with the kernel's own xhat (one rounding more)."""
    reached = set()
    for name in ACT_BWD_CASES:
        c = X.GN_BY_NAME[name]
        N, S, C = c["N"], c["S"], c["C"]
        x = _code_x((N, S, C), dtype)
        mean, rstd, stats = _reduce_stats(c)
        xh = ((x - X.per_channel(mean, c["cpg"])) * X.per_channel(rstd, c["cpg"])).double()
        for stream, pos in X.gn_reduce_stream_positions(S, C).items():
            reached.add((name, stream))
            g = torch.zeros(N, S, C)
            g[:, pos, :] = 2.0
            mc = drop_mask(hip, (N, S, C)) if drop else None
            R1, R2 = _reduce(hip, c, dtype, g, x, stats, code, mc)
            d, bound, mag = EC.hw_act_bound(x[:, pos, :].double(), code, True)
            k = 2.0 * (mc[0][:, pos, :] if drop else 1.0)
            what = f"rho_gn_bwd_reduce{'_drop' if drop else ''} act'={EC.ACT_NAMES[code]} {_dn(dtype)} {name} g at {pos} ({stream})"
            assert_within_abs(R1, k * d, k * bound, what + ": R1 [N, C]")
            xa = xh[:, pos, :].abs()
            assert_within_abs(R2, k * d * xh[:, pos, :], k * bound * xa + EC.U * k * mag * xa, what + ": R2 [N, C]")
            if dtype == F32 and not drop:
                print(f"measured: {what}: R1 worst {float(((R1 - k * d).abs() / f32_ulp(k * mag)).max()):.3f} ulp of the term magnitude")
    assert {s for n, s in reached if n == "nblk2_tails"} == {"gq", "gr", "tail"} and ("c2048", "gr") in reached, reached


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dn)
@pytest.mark.parametrize("code", ALL_CODES, ids=[EC.ACT_NAMES[k] for k in ALL_CODES])
def test_backward_reduce_activation_derivative_dense(hip, code, dtype, drop):
    """(b) dense g in +-2: each term g act'(x) within |g| times the activation bound (the product by +-1, +-2 and the mask's 0 / 2 is
    exact), and S terms added in some order: every addition of a nonzero term rounds at most once, so a term passes through fewer
    than S roundings of partial sums bounded by sum |g| Mag: |dR1| <= sum |g| bound + S 2^-24 sum |g| Mag; R2 likewise with every
    term times |xhat| (the fma adds gq * xhat unrounded)."""
    for name in ACT_BWD_CASES:
        c = X.GN_BY_NAME[name]
        N, S, C = c["N"], c["S"], c["C"]
        x = _code_x((N, S, C), dtype)
        mean, rstd, stats = _reduce_stats(c)
        xh = ((x - X.per_channel(mean, c["cpg"])) * X.per_channel(rstd, c["cpg"])).double()
        g = X.gn_int((N, S, C), "gnact_g" + name, 0, 3).double() - 2.0
        g = torch.where(g >= 0, g + 1.0, g)                                        # -2, -1, 1, 2
        mc = drop_mask(hip, (N, S, C)) if drop else None
        R1, R2 = _reduce(hip, c, dtype, g.float(), x, stats, code, mc)
        d, bound, mag = EC.hw_act_bound(x.double(), code, True)
        k = g * (mc[0] if drop else 1.0)
        what = f"rho_gn_bwd_reduce{'_drop' if drop else ''} act'={EC.ACT_NAMES[code]} {_dn(dtype)} {name} dense g"
        b1 = (k.abs() * bound).sum(1) + S * EC.U * (k.abs() * mag).sum(1)
        b2 = (k.abs() * bound * xh.abs()).sum(1) + S * EC.U * (k.abs() * mag * xh.abs()).sum(1)
        w1 = assert_within_abs(R1, (k * d).sum(1), b1, what + ": R1 [N, C]")
        w2 = assert_within_abs(R2, (k * d * xh).sum(1), b2, what + ": R2 [N, C]")
        if dtype == F32 and not drop:
            print(f"measured: {what}: R1 worst {w1:.3e} (bound up to {float(b1.max()):.3e}), R2 worst {w2:.3e} (bound up to {float(b2.max()):.3e})")


# ----------------------------------------------------------------------------- 7. gnb_* on data-gradient launches
def cl(t, dtype):
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV).to(dtype)


def from_cl(y):
    return y.float().cpu().permute(0, 4, 1, 2, 3)


EXPECT_GNB = {
    ("gnb_bm64", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("gnb_bm64", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
    ("gnb_bm128", "bf16"): "k_conv<bf16,3,3,3,BM=128,MAXP=5,NW=8,M16=1>",
    ("gnb_bm128", "f32"): "k_conv<f32,3,3,3,BM=128,MAXP=5,NW=8,M16=0>",
    ("gnb_ragged", "bf16"): "k_conv<bf16,3,3,3,BM=64,MAXP=10,NW=4,M16=1>",
    ("gnb_ragged", "f32"): "k_conv<f32,3,3,3,BM=64,MAXP=10,NW=4,M16=0>",
}
GNB_PARAMS = [pytest.param(c, dt, id=f"{c['name']}-{_dn(dt)}") for c in X.GNB_CASES for dt in c["dtypes"]]


@pytest.mark.parametrize("c,dtype", GNB_PARAMS)
def test_dgrad_with_fused_groupnorm_backward_reduction(hip, ops, c, dtype):
    """rho_conv_desc.gnb_* on 3x3x3 data-gradient launches (BM = 64, BM = 128, a ragged volume; two concat sources, gnb_c1 < split;
    integer a / b, gnb_silu = 0): the output equals fp64 autograd bit for bit, the per-tile rows sum dz and sum dz x0 equal the sums
    over the stored output, and rho_gn_bwd_finalize(fmt = 1) on them gives the fp64 coefficients of the separate reduce pass."""
    o = X.gnb_operands(c)
    r = X.bwd_reference(c, o)
    N, c1, c2 = c["N"], c["c1"], c["c2"]
    C = c1 + c2
    D, H, W = c["spatial"]
    S = o["S"]
    (check_bf16_exact if dtype == BF16 else check_f32_exact)(r["dx"], "dX")
    dy = cl(o["dy"], dtype)
    wd = ops.prep_conv_weight_dgrad(o["w"].to(DEV), dtype)
    zb = torch.zeros(wd.shape[1], device=DEV)
    x1, x2 = cl(o["x0"][:, :c1], dtype), cl(o["x0"][:, c1:], dtype)
    a, b = dev(o["a"]), dev(o["b"])
    xflat, dx = guarded((N, D, H, W, C), dtype)
    d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=C, split=C, y=dx, y2=None)
    tiles = ops.conv_stats_tiles(d)
    ids = X.tile_ids(c, "k_conv")
    assert tiles == int(ids.max()) + 1, (tiles, int(ids.max()) + 1)
    sflat, sbuf = guarded((N, tiles, 2, C), F32)
    d.stats = sbuf.data_ptr()
    d.gnb_x1, d.gnb_x2, d.gnb_c1, d.gnb_silu = x1.data_ptr(), x2.data_ptr(), c1, 0
    d.gnb_a, d.gnb_b = a.data_ptr(), b.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == EXPECT_GNB[(c["name"], _dn(dtype))], variant
    ops.conv_launch(d)
    torch.cuda.synchronize()
    what = f"{c['name']} {variant} gnb"
    assert guards_intact(xflat), what + ": store outside dX"
    assert guards_intact(sflat), what + ": store outside the statistics"
    assert_bit_equal(from_cl(dx), r["dx"], what + ": dX")
    want = X.stats_reference(r["dx"], ids, o["x0"])
    check_f32_exact(want, "statistics reference")
    assert_bit_equal(sbuf, want, what + ": per-tile (sum dz, sum dz x0) [N, tile, 2, C]")
    # the finalize pass on these rows against the fp64 reduction over the whole tensors
    scale = o["film"][:, :C]
    q = X.gn_bwd_reference(X.to_nsc(r["dx"]), X.to_nsc(o["x0"]), o["mean"], o["rstd"], o["gamma"], o["beta"], scale)
    v = _bwd_finalize(hip, sbuf, tiles, 1, N, C, S, _bwd_dev(o), True)
    _check_coeffs(v, q, C, True, X.is_pow2((C // 32) * S), what + " -> rho_gn_bwd_finalize(fmt=1)")


@pytest.mark.parametrize("c,dtype", GNB_PARAMS)
def test_dgrad_with_fused_activation_derivative_in_the_rows(hip, ops, c, dtype):
    """The same launches with gnb_silu = 1 and integer u = gnb_a x0 + gnb_b in [-10, 10]: the stored dX is still the integer conv
    result, bit for bit; the per-tile rows are sum dz and sum dz x0 with dz = dX * dsilu_f(u), each within the per-row bound of
    exact_cases.gnb_silu_reference (the derived dsilu_f bound per term plus n 2^-24 of the magnitude sums for the n additions)."""
    o = X.gnb_silu_operands(c)
    N, c1, c2 = c["N"], c["c1"], c["c2"]
    C = c1 + c2
    D, H, W = c["spatial"]
    dy = cl(o["dy"], dtype)
    wd = ops.prep_conv_weight_dgrad(o["w"].to(DEV), dtype)
    zb = torch.zeros(wd.shape[1], device=DEV)
    x1, x2 = cl(o["x0"][:, :c1], dtype), cl(o["x0"][:, c1:], dtype)
    a, b = dev(o["a"]), dev(o["b"])
    xflat, dx = guarded((N, D, H, W, C), dtype)
    d = ops.make_conv_desc(dy, None, wd, zb, kernel=c["kernel"], cout=C, split=C, y=dx, y2=None)
    tiles = ops.conv_stats_tiles(d)
    ids = X.tile_ids(c, "k_conv")
    assert tiles == int(ids.max()) + 1, (tiles, int(ids.max()) + 1)
    z, rows, rb = X.gnb_silu_reference(c, o, ids)
    sflat, sbuf = guarded((N, tiles, 2, C), F32)
    d.stats = sbuf.data_ptr()
    d.gnb_x1, d.gnb_x2, d.gnb_c1, d.gnb_silu = x1.data_ptr(), x2.data_ptr(), c1, 1
    d.gnb_a, d.gnb_b = a.data_ptr(), b.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == EXPECT_GNB[(c["name"], _dn(dtype))], variant
    ops.conv_launch(d)
    torch.cuda.synchronize()
    what = f"{c['name']} {variant} gnb_silu"
    assert guards_intact(xflat), what + ": store outside dX"
    assert guards_intact(sflat), what + ": store outside the statistics"
    assert_bit_equal(from_cl(dx), z, what + ": dX")
    worst = float(((sbuf.cpu().double() - rows).abs() / rb.clamp_min(1e-300)).max())
    print(f"measured: {what}: per-tile rows worst {worst:.3f} of the derived bound")
    assert_within_abs(sbuf, rows, rb, what + ": per-tile (sum dz, sum dz x0) [N, tile, 2, C]")


# ----------------------------------------------------------------------------- 8. gna_* on the 1x1x1 skip data gradient
def _gna_variant(case):
    bm = case[5]
    return f"k_conv<{_dn(case[1])},1,1,1,BM={bm},MAXP={5 if bm == 128 else 10},NW={8 if bm == 128 else 4},M16=0>+gn_apply"


@pytest.mark.parametrize("case", X.GNA_CASES, ids=[c[0] for c in X.GNA_CASES])
def test_skip_dgrad_with_fused_groupnorm_backward_apply(hip, ops, case):
    """rho_conv_desc.gna_*: the +gn_apply variants at BM = 32 / 64 / 128 in bf16 and f32, both output regions (y2 channels-last),
    integer cA / cP / cQ, gnb_silu = 0: both outputs equal the fp64 conv + cA g + cQ x0 + cP bit for bit."""
    name, dtype, cy, c1, c2, bm, (N, D, H, W) = case
    o = X.gna_operands(case)
    want = X.gna_reference(o)
    check_bf16_exact(want, "reference")
    C = c1 + c2
    dy = dev(o["dy"], dtype)
    wd = ops.prep_conv_weight_dgrad(o["w"].to(DEV), dtype)
    zb = torch.zeros(wd.shape[1], device=DEV)
    x1, x2, g = dev(o["x0"][..., :c1], dtype), dev(o["x0"][..., c1:], dtype), dev(o["g"], dtype)
    a, b, cA, cP, cQ = (dev(o[k]) for k in ("a", "b", "cA", "cP", "cQ"))
    ff1, f1 = guarded((N, D, H, W, c1), dtype)
    ff2, f2 = guarded((N, D, H, W, c2), dtype)
    d = ops.make_conv_desc(dy, None, wd, zb, kernel=(1, 1, 1), cout=C, split=c1, y=f1, y2=f2, y2_cl=True)
    d.gnb_x1, d.gnb_x2, d.gnb_c1, d.gnb_silu = x1.data_ptr(), x2.data_ptr(), c1, 0
    d.gnb_a, d.gnb_b = a.data_ptr(), b.data_ptr()
    d.gna_g, d.gna_cA, d.gna_cP, d.gna_cQ = g.data_ptr(), cA.data_ptr(), cP.data_ptr(), cQ.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == _gna_variant(case), variant
    ops.conv_launch(d)
    torch.cuda.synchronize()
    assert guards_intact(ff1), name + ": store outside the first region"
    assert guards_intact(ff2), name + ": store outside the second region"
    assert_bit_equal(f1.float(), want[..., :c1], f"{name} {variant}: first region [N, D, H, W, c1]")
    assert_bit_equal(f2.float(), want[..., c1:], f"{name} {variant}: second region [N, D, H, W, c2]")


@pytest.mark.parametrize("case", X.GNA_CASES, ids=[c[0] for c in X.GNA_CASES])
def test_skip_dgrad_with_fused_apply_and_activation_derivative(hip, ops, case):
    """The same +gn_apply launches with gnb_silu = 1, the form the training plan runs behind a SiLU: integer u = a x0 + b in
    [-10, 10], cA = 1, cP = cQ = 0, g in {0, +-1/4, +-1/2}, so each stored element of both output regions is the exact integer conv result plus
    g * dsilu_f(u).  float32: within |g| (dsilu_f bound at u) + 2^-24 (|conv| + |g| Mag) per element; bf16: the tie rule with four
    times that as the margin (the host twin holds the share near a tie to 1 %)."""
    name, dtype, cy, c1, c2, bm, (N, D, H, W) = case
    o = X.gna_silu_operands(case)
    _, _, want, fb = X.gna_silu_reference(o)
    C = c1 + c2
    dy = dev(o["dy"], dtype)
    wd = ops.prep_conv_weight_dgrad(o["w"].to(DEV), dtype)
    zb = torch.zeros(wd.shape[1], device=DEV)
    x1, x2, g = dev(o["x0"][..., :c1], dtype), dev(o["x0"][..., c1:], dtype), dev(o["g"], dtype)
    a, b, cA, cP, cQ = (dev(o[k]) for k in ("a", "b", "cA", "cP", "cQ"))
    ff1, f1 = guarded((N, D, H, W, c1), dtype)
    ff2, f2 = guarded((N, D, H, W, c2), dtype)
    d = ops.make_conv_desc(dy, None, wd, zb, kernel=(1, 1, 1), cout=C, split=c1, y=f1, y2=f2, y2_cl=True)
    d.gnb_x1, d.gnb_x2, d.gnb_c1, d.gnb_silu = x1.data_ptr(), x2.data_ptr(), c1, 1
    d.gnb_a, d.gnb_b = a.data_ptr(), b.data_ptr()
    d.gna_g, d.gna_cA, d.gna_cP, d.gna_cQ = g.data_ptr(), cA.data_ptr(), cP.data_ptr(), cQ.data_ptr()
    variant = ops.conv_variant(d)
    assert variant == _gna_variant(case), variant
    ops.conv_launch(d)
    torch.cuda.synchronize()
    assert guards_intact(ff1), name + ": store outside the first region"
    assert guards_intact(ff2), name + ": store outside the second region"
    for got, sl, region in ((f1, slice(0, c1), "first"), (f2, slice(c1, C), "second")):
        what = f"{name} {variant} gnb_silu: {region} region [N, D, H, W, c]"
        w, f = want[..., sl], fb[..., sl]
        if dtype == F32:
            print(f"measured: {what}: worst error {float(((got.cpu().double() - w).abs() / f.clamp_min(1e-300)).max()):.3f} of the derived bound")
            assert_within_abs(got, w, f, what)
        else:
            share = assert_bf16_tie_rule(got, w, 4 * f, what)
            print(f"measured: {what}: bf16 by the tie rule, {share:.4%} near a tie")
