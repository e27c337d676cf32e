"""-m gpu: attention as a permutation.

An exact softmax does not exist, but a one-hot one does.  Per (batch, head) key s carries a distinct +-1 code c_s of length ch
(k_s = c_s) and query t asks for key pi(t): q_t = A c_{pi(t)} with A = 512 (1024 where ch needs it).  The matched logit A ch exceeds
every other by at least 2 A, i.e. by 2 A / sqrt(ch) * log2(e) >= 160 in the kernel's scaled base-2 units (asserted on the fp64
reference), so every other probability is exp2(< -160) = exactly 0 in fp32 and the row of P is one-hot up to the rounding of the
running maximum.  v holds integers |v| <= 127 that depend on (b, h, c, s), dO integers |dO| <= 2: a key tile assigned to the wrong
query tile, a wrong head or batch offset, a lost tail key - each changes a value.

bf16 (P is rounded to bf16 before the PV product: exactly 1.0):  out[b, t, h, :] == v[b, h, :, pi(t)],
dV[b, h, :, pi(t)] == dO[b, t, h, :] - bit-exact, into NaN-prefilled guarded buffers; dQ == dK == 0 exactly where ch^-0.5 is a power
of two, else within the one rounding the kernel's fma exposes (derived at the assertion).
fp32: out and dV per element within |want| * (ln 2 * ulp(m) / 2 + 2^-21) - m the matched logit (base-2, from the reference);
ulp(m) / 2 is the rounding of the running maximum that fmaf(s, sc, -m) exposes, 2^-21 one exp2 and one reciprocal at about an ulp.
lse (both dtypes): |lse - m| <= ulp(m) + 1e-6 |m|.  Softmax away from one-hot stays with the tolerance tests."""
import math

import pytest
import torch

import exact_cases as X
from exact_cases import BF16, F32
from exact_util import assert_bit_equal, guarded, guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _ulp32(m):
    a = m.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,heads,ch", X.ATTN_CASES)
def test_attention_forward_and_backward_as_a_permutation(ops, dtype, B, T, heads, ch):
    o = X.attn_operands(B, T, heads, ch)
    r = X.attn_reference(o, ch)
    assert float(r["gap"].min()) >= X.ATTN_MIN_GAP
    C = heads * ch
    pi = o["pi"]                                                                  # [B, heads, T]
    q, k, v, do = (o[n].reshape(B, C, T) for n in ("q", "k", "v", "do"))
    qk = torch.cat([q, k], 1).permute(0, 2, 1).contiguous().to(DEV).to(dtype)     # [B, T, 2C]
    vt = v.contiguous().to(DEV).to(dtype)                                         # [B, C, T]
    docl = do.permute(0, 2, 1).contiguous().to(DEV).to(dtype)                     # [B, T, C]
    oflat, out = guarded((B, T, C), dtype)
    lflat, lse = guarded((B, heads, T), F32)
    ops.attention(qk, vt, heads, out=out, lse=lse)
    gflat, dqkv = guarded((B, T, 3 * C), dtype)
    ops.attention_bwd(qk, vt, out, docl, lse, heads, dqkv=dqkv)
    torch.cuda.synchronize()
    assert guards_intact(oflat) and guards_intact(lflat) and guards_intact(gflat)

    idx = pi.unsqueeze(2).expand(B, heads, ch, T)
    want_out = torch.gather(o["v"], 3, idx).double()                              # [b, h, c, t] = v[b, h, c, pi(t)]
    want_dv = torch.zeros(B, heads, ch, T, dtype=torch.float64).scatter_(3, idx, o["do"].double())   # [b, h, c, pi(t)] = dO[b, h, c, t]
    got_out = out.float().cpu().permute(0, 2, 1).reshape(B, heads, ch, T).double()
    g = dqkv.float().cpu().permute(0, 2, 1).double()                              # [B, 3C, T]
    got_dq, got_dk = g[:, :C], g[:, C:2 * C]
    got_dv = g[:, 2 * C:].reshape(B, heads, ch, T)

    m = r["m"]                                                                    # [B, heads, T], fp64
    ulp = _ulp32(m)
    lse_err = (lse.cpu().double() - m).abs()
    lse_bound = ulp + 1e-6 * m.abs()
    print(f"lse: max err {float(lse_err.max()):.3e}, bound at that element {float(lse_bound.flatten()[lse_err.argmax()]):.3e}")
    assert bool((lse_err <= lse_bound).all()), (float(lse_err.max()), float(lse_bound.min()))

    if dtype == BF16:
        assert_bit_equal(got_out, want_out, "out [b, h, c, t] == v[b, h, c, pi(t)]")
        assert_bit_equal(got_dv, want_dv, "dV [b, h, c, pi(t)] == dO[b, h, c, t]")
        # dQ and dK: dS = P (dP - D) ch^-0.5 with dP = D the same exact integer (D = sum_c dO O, O = v exactly).  The kernels form
        # it as P * fmaf(dP, scale, -fl(D * scale)) (attention_bwd.hip): where scale = ch^-0.5 is a power of two (ch = 16, 64, 256)
        # the product is exact and dS, dQ, dK are exactly 0.  Otherwise the fma exposes the rounding of fl(D * scale):
        # |dS| <= P * ulp(D * scale) / 2 at the matched key and 0 elsewhere, so with k = +-1 and q = +-A
        #   |dQ[., t]| <= eps_t,  |dK[., pi(t)]| <= A eps_t,  eps_t = ulp(D_t * scale) / 2 * (1 + 2^-7)
        # (P <= exp2(ulp(m)) <= 1.0014, one bf16 rounding of dS and one of the stored value, 2^-9 each).  D_t = 0 keeps exact zeros.
        D = (o["do"].double() * want_out).sum(2)                                  # [B, heads, T], exact integers
        scale32 = torch.tensor(1.0 / math.sqrt(ch), dtype=torch.float32)
        if math.log2(ch) % 2 == 0:
            eps = torch.zeros_like(D)
        else:
            eps = _ulp32(D.float() * scale32) / 2 * (1 + 2.0 ** -7) * (D != 0)
        eps_s = torch.zeros_like(eps).scatter_(2, pi, eps)                        # by key s = pi(t)
        bq = eps.unsqueeze(2).expand(B, heads, ch, T).reshape(B, C, T)
        bk = (o["amp"] * eps_s).unsqueeze(2).expand(B, heads, ch, T).reshape(B, C, T)
        print(f"dQ: max |value| {float(got_dq.abs().max()):.3e} (bound max {float(bq.max()):.3e}); "
              f"dK: max |value| {float(got_dk.abs().max()):.3e} (bound max {float(bk.max()):.3e})")
        if float(eps.max()) == 0.0:
            assert_bit_equal(got_dq, torch.zeros_like(got_dq), "dQ == 0 [B, C, T]")
            assert_bit_equal(got_dk, torch.zeros_like(got_dk), "dK == 0 [B, C, T]")
        else:
            for nm, got, bound in (("dQ", got_dq, bq), ("dK", got_dk, bk)):
                bad = ~(got.abs() <= bound)                                       # (NaN = unwritten fails)
                assert not bool(bad.any()), (f"{nm}: {int(bad.sum())} elements beyond the rounding of fl(D * scale), first at "
                                             f"{tuple(bad.nonzero()[0].tolist())}: {got[tuple(bad.nonzero()[0].tolist())].item()!r}")
    else:
        rel = (math.log(2.0) * ulp / 2 + 2.0 ** -21)                              # per query t
        bound_out = want_out.abs() * rel.unsqueeze(2)
        # dV[.., s] is the contribution of the one query t with pi(t) = s: its bound is that query's
        rel_s = torch.zeros_like(rel).scatter_(2, pi, rel)
        bound_dv = want_dv.abs() * rel_s.unsqueeze(2)
        e_out, e_dv = (got_out - want_out).abs(), (got_dv - want_dv).abs()
        print(f"out: max err / bound {float((e_out / bound_out.clamp_min(1e-300)).max()):.3f}; "
              f"dV: max err / bound {float((e_dv / bound_dv.clamp_min(1e-300)).max()):.3f}; rel bound max {float(rel.max()):.3e}")
        assert torch.isfinite(got_out).all() and torch.isfinite(g).all()
        bad = ~(e_out <= bound_out)
        assert not bool(bad.any()), f"out: {int(bad.sum())} elements beyond the derived bound, first at {tuple(bad.nonzero()[0].tolist())}"
        bad = ~(e_dv <= bound_dv)
        assert not bool(bad.any()), f"dV: {int(bad.sum())} elements beyond the derived bound, first at {tuple(bad.nonzero()[0].tolist())}"
