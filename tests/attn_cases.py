"""Attention away from one-hot: operands, fp64 reference, per-element bounds and a rounding model of the bf16 kernels.

Shared by tests/test_attn_cases_host.py (CPU: the conditions on the inputs, the model inside the bounds, the mutations outside
them) and tests/test_gpu_attention_elementwise.py (GPU: every dispatched kernel inside the same bounds).  Nothing here touches the
GPU at import.  Every tensor is [B, heads, T, ch] unless said otherwise; `pack` / `unpack` go to and from the kernels' layouts.

Inputs ("peaked, not one-hot, with a staircase"), per (b, h), rounded to the case's dtype before anything else sees them:
    q_t = sharp * (n_t - (n_t . u) u) + sqrt(ch) u        n: noise, u: a unit vector
    k_s = n'_s + stair * sign(h) * (s // 32) * u          sign(h) = +1 for even heads, -1 for odd ones
so the natural logit q_t . k_s / sqrt(ch) = sharp * N(0, 1) + stair * sign(h) * (s // 32) + (u . n'_s): noise of a few nats on a
staircase that climbs (even heads) or falls (odd heads) by `stair` every 32 keys.  The noise of q is projected off u: its
component along u would multiply the staircase by 1 + sharp (n . u) / sqrt(ch) per query, which at ch = 16 turns it around for
some queries.  v and dO are noise over (b, h, t, c), so a wrong head, batch or channel offset changes values.

Bounds.  u = 2^-8 (twice bf16's unit roundoff), p the fp64 probabilities, dS = p (dP - delta) ch^-0.5, D_t = sum_c |dO_tc O_tc|:
    out[t, c]  2u sum_s p_ts |v_sc|                    P is rounded to bf16 before the PV product, the output once
    dV[s, c]   2u sum_t p_ts |dO_tc|
    dQ[t, c]   u (2 sum_s |dS_ts| |k_sc| + ch^-0.5 D_t sum_s p_ts |k_sc|)     dS rounded to bf16, the output rounded, delta formed
    dK[s, c]   u (2 sum_t |dS_ts| |q_tc| + ch^-0.5 sum_t p_ts D_t |q_tc|)     from the bf16-rounded O
each plus the fp32 term, which alone is the bound of the fp32 kernels.  The fp32 term is a worst case, derived in `bounds`."""
from __future__ import annotations

import math

import torch

from detdata import det_normal

F32, BF16 = torch.float32, torch.bfloat16
LOG2E = 1.4426950408889634
U = 2.0 ** -8
EPS24 = 2.0 ** -24

# (B, T, heads, ch): the smallest shapes that reach the edges (tests/test_gpu_attention_elementwise.py says which)
CASES = [(2, 161, 2, 16), (1, 333, 2, 32), (1, 328, 2, 64), (1, 130, 1, 64), (2, 49, 2, 128), (1, 177, 2, 128), (1, 161, 1, 256),
         (1, 200, 2, 256)]
# (sharpness, stair, scale of q) per case, tuned on the CPU until the conditions of test_attn_cases_host.py hold (they are conditions
# on the fp64 reference; no kernel output enters).  T = 161 and 177 need the steeper stair for the third key tile (33 and 49 keys)
# to raise every query's maximum; ch = 256 scales q down to keep the fp32 bounds below 2^-10 of their magnitude terms.
PARAMS = {c: (1.5, 2.5, 1.0) for c in CASES}
PARAMS[(2, 161, 2, 16)] = PARAMS[(1, 177, 2, 128)] = (1.25, 3.0, 1.0)
PARAMS[(1, 161, 1, 256)] = PARAMS[(1, 200, 2, 256)] = (1.5, 2.5, 0.8)
E2E_CASE = (1, 328, 2, 64)


def case_id(c):
    return "B{}_T{}_h{}_ch{}".format(*c)


def fwd_kt(ch):
    """Keys per tile of k_attn_bf16 (and of the rounding model)."""
    return 32 if ch >= 256 else 64


def variant_table():
    """EXPECT_ATTN[(switches on, dtype name, ch, backward)] -> the name rho_attention_variant must give."""
    t = {}
    for ch in (16, 32, 64, 128, 256):
        kb = 32 if ch == 256 else 64
        fm = 64 if ch <= 64 else 32
        bm = 64 if ch <= 32 else 32
        kv = 64 if ch <= 64 else (32 if ch == 128 else 16)
        pair = f"k_attn_delta<bf16>+k_attn_dq<{ch},{kb}>+k_attn_dkv<{ch},{kb},0>+k_attn_dkv<{ch},{kb},1>"
        valu = f"k_attn_delta<f32>+k_attn_dq_f32<{ch},{kv}>+k_attn_dkv_f32<{ch},{kv}>"
        for sw in (False, True):
            t[(sw, "bf16", ch, False)] = f"k_attn_bf16<{ch},{kb}>"
            t[(sw, "f32", ch, False)] = f"k_attn_f32<{ch},{kv}>" if sw else f"k_attn_f32m<{ch},{fm}>"
            t[(sw, "bf16", ch, True)] = pair if (sw or ch != 64) else "k_attn_delta<bf16>+k_attn_dq<64,64>+k_attn_dkv_fused<64,64>"
            t[(sw, "f32", ch, True)] = valu if (sw or ch == 256) else f"k_attn_delta<f32>+k_attn_dq_f32m<{ch},{bm}>+k_attn_dkv_f32m<{ch},{bm}>"
    return t


EXPECT_ATTN = variant_table()
SWITCHES = {"RHO_ATTN_F32_VALU": "1", "RHO_ATTN_DKV_SPLIT": "1"}


def kernel_names(names):
    """Single kernel names of '+'-joined variant strings."""
    return {k for n in names for k in n.split("+")}


# ----------------------------------------------------------------------------- operands
_OPS = {}


def operands(case, dtype):
    """q, k, v, do: float64 [B, heads, T, ch] holding values of `dtype` exactly."""
    key = (case, dtype)
    if key in _OPS:
        return _OPS[key]
    B, T, H, ch = case
    sharp, stair, qs = PARAMS[case]
    tag = "attnew_" + case_id(case)
    u = det_normal((B, H, 1, ch), tag + "u").double()
    u = u / u.norm(dim=-1, keepdim=True)
    nq = det_normal((B, H, T, ch), tag + "q").double()
    q = qs * (sharp * (nq - (nq * u).sum(-1, keepdim=True) * u) + math.sqrt(ch) * u)
    sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(H)], dtype=torch.float64).view(1, H, 1, 1)
    level = (torch.arange(T) // 32).double().view(1, 1, T, 1)
    k = det_normal((B, H, T, ch), tag + "k").double() + stair * sign * level * u
    v = det_normal((B, H, T, ch), tag + "v").double()
    do = det_normal((B, H, T, ch), tag + "do").double()
    o = {n: t.float().to(dtype).double() for n, t in (("q", q), ("k", k), ("v", v), ("do", do))}
    _OPS[key] = o
    return o


def pack(o, dtype):
    """Kernel layouts (CPU tensors of `dtype`): qk [B, T, 2C], vt [B, C, T], do [B, T, C]."""
    B, H, T, ch = o["q"].shape
    cl = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, H * ch)
    return dict(qk=torch.cat([cl(o["q"]), cl(o["k"])], -1).to(dtype).contiguous(),
                vt=o["v"].permute(0, 1, 3, 2).reshape(B, H * ch, T).to(dtype).contiguous(), do=cl(o["do"]).to(dtype).contiguous())


def to_cl(t):
    """[B, heads, T, ch] -> channels-last [B, T, C]."""
    B, H, T, ch = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * ch)


def from_cl(t, heads):
    """channels-last [B, T, C] -> float64 [B, heads, T, ch] on the CPU."""
    B, T, C = t.shape
    return t.detach().cpu().double().view(B, T, heads, C // heads).permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------- fp64 reference
_REF = {}


def reference(case, dtype):
    """fp64: s2 (scaled base-2 logits [B, H, T, T]), p, lse (base 2), out, dq, dk, dv, ds and the magnitude sums of the bounds."""
    key = (case, dtype)
    if key in _REF:
        return _REF[key]
    o = operands(case, dtype)
    q, k, v, do = o["q"], o["k"], o["v"], o["do"]
    ch = q.shape[-1]
    scale = 1.0 / math.sqrt(ch)
    s2 = q @ k.transpose(-1, -2) * (LOG2E * scale)
    m = s2.max(-1).values
    lse = m + torch.log2(torch.exp2(s2 - m.unsqueeze(-1)).sum(-1))
    p = torch.exp2(s2 - lse.unsqueeze(-1))
    out = p @ v
    dp = do @ v.transpose(-1, -2)
    delta = (do * out).sum(-1)
    ds = p * (dp - delta.unsqueeze(-1)) * scale
    r = dict(s2=s2, m=m, lse=lse, p=p, out=out, dp=dp, delta=delta, ds=ds, dq=ds @ k, dk=ds.transpose(-1, -2) @ q,
             dv=p.transpose(-1, -2) @ do)
    r["o_in"] = out.float().to(dtype).double()            # what the backward is fed: the reference O in the case's dtype
    r["lse_in"] = lse.float()
    _REF[key] = r
    return r


def f32_ulp(v):
    _, e = torch.frexp(v.double().abs())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - 24).clamp_min(-149))


def bounds(case, dtype, fwd_out_bound=None, fwd_lse_bound=None):
    """Per-element bounds out, lse, dq, dk, dv (+ the magnitude terms 'mag_*' and the fp32 parts 'f32_*').

    fp32 term, a worst case over the kernels' fp32 operations (T keys or queries, ch channels):
      * a logit (scaled, base 2) is a sum of ch products in some order: |error| <= ch 2^-24 sum_c |q_tc k_sc| sc2, sc2 = log2(e) ch^-0.5;
        the running maximum (forward) and lse (backward input, forward output) are fp32 numbers: 2^-24 |m_t| and 2^-24 |lse_t|,
        and the fused multiply-add that forms the exponent rounds once more at that magnitude.  Together
            eps_t = max_s(ch 2^-24 A_ts sc2) + 2^-23 (|m_t| + |lse_t|),        A_ts = sum_c |q_tc k_sc|;
      * it enters a probability as the relative error ln 2 * eps_t; exp2 is within 2 ulps (exp2f and v_exp_f32 are documented at 1),
        the reciprocal of l within 1, the product with it within a half, the rounding of p itself a half: 4 * 2^-23 together:
            d_t = ln 2 * eps_t + 4 * 2^-23;
      * a sum of n fp32 terms in any order is off by at most n 2^-24 times the sum of the magnitudes: acc = (T + 8) 2^-24 for the sums
        over keys or queries (P V, l, dS K, dS^T Q, P^T dO), (ch + 4) 2^-24 for dP and delta (with the fma that forms dP - delta).
      out = sum_s p v / l: numerator and denominator carry d_t + acc each ->  f32_out[t, c] = 2 (d_t + acc) sum_s p_ts |v_sc|
      dV:   f32_dv[s, c] = sum_t (d_t + acc) p_ts |dO_tc|
      dS:   g_ts = (d_t + acc) |dS_ts| + p_ts ch^-0.5 (ch + 4) 2^-24 (E_ts + D_t),  E_ts = sum_c |dO_tc v_sc| >= |dP_ts|, D_t >= |delta_t|
      dQ:   f32_dq[t, c] = sum_s g_ts |k_sc|,   dK: f32_dk[s, c] = sum_t g_ts |q_tc|
      lse:  |lse - ref| <= eps_t + 2 ulp32(ref): the logit error, the rounding of m + log2(l) and of log2 itself.  (The sum l over T
            terms is not given an accumulation term of its own here: a few keys carry it, and eps_t's 2^-23 (|m| + |lse|) is
            several ulps of lse.)
    With fwd_out_bound / fwd_lse_bound (the forward's own bounds) the backward bounds are widened for a backward that is fed the
    forward kernel's out and lse instead of the reference's: with |dO_t| W-weighted, w_t = sum_c |dO_tc| b_out[t, c] bounds the
    change of delta_t and g'_t = 1.01 ln 2 b_lse[t] the relative change of every p_ts (|2^x - 1| <= 1.01 ln 2 |x| for |x| < 0.01):
      dV += sum_t g'_t p_ts |dO_tc|;  dS_ts changes by at most g'_t |dS_ts| + (1 + g'_t) p_ts ch^-0.5 w_t =: h_ts,
      dQ += sum_s h_ts |k_sc|,  dK += sum_t h_ts |q_tc|;  the rounding terms grow by the factor (1 + max g') at most."""
    o, r = operands(case, dtype), reference(case, dtype)
    q, k, v, do = o["q"], o["k"], o["v"], o["do"]
    B, H, T, ch = q.shape
    scale = 1.0 / math.sqrt(ch)
    p, ds = r["p"], r["ds"].abs()
    pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
    D = (do * r["out"]).abs().sum(-1)                                       # [B, H, T]
    mag = dict(out=p @ v.abs(), dv=pt @ do.abs(), dq=ds @ k.abs(), dk=dst @ q.abs())
    A = q.abs() @ k.abs().transpose(-1, -2)
    eps = (ch * EPS24 * A * (LOG2E * scale)).max(-1).values + 2 * EPS24 * (r["m"].abs() + r["lse"].abs())
    acc = (T + 8) * EPS24
    d = (math.log(2.0) * eps + 4 * 2 * EPS24 + acc).unsqueeze(-1)           # [B, H, T, 1]: d_t + acc
    E = do.abs() @ v.abs().transpose(-1, -2)
    g = d * ds + p * scale * (ch + 4) * EPS24 * (E + D.unsqueeze(-1))
    f32 = dict(out=2 * d * mag["out"], dv=(d * p).transpose(-1, -2) @ do.abs(), dq=g @ k.abs(), dk=g.transpose(-1, -2) @ q.abs())
    b = dict(lse=eps + 2 * f32_ulp(r["lse"]), eps=eps)
    if dtype == BF16:
        b["out"] = 2 * U * mag["out"] + f32["out"]
        b["dv"] = 2 * U * mag["dv"] + f32["dv"]
        b["dq"] = U * (2 * mag["dq"] + scale * D.unsqueeze(-1) * (p @ k.abs())) + f32["dq"]
        b["dk"] = U * (2 * mag["dk"] + scale * (p * D.unsqueeze(-1)).transpose(-1, -2) @ q.abs()) + f32["dk"]
    else:
        for n in ("out", "dv", "dq", "dk"):
            b[n] = f32[n]
    if fwd_out_bound is not None:
        w = (do.abs() * fwd_out_bound).sum(-1).unsqueeze(-1)
        gp = (1.01 * math.log(2.0) * fwd_lse_bound).unsqueeze(-1)
        assert float(fwd_lse_bound.max()) < 0.01
        grow = 1 + float(gp.max())
        h = gp * ds + (1 + gp) * p * scale * w
        b["dv"] = grow * b["dv"] + (gp * p).transpose(-1, -2) @ do.abs()
        b["dq"] = grow * b["dq"] + h @ k.abs()
        b["dk"] = grow * b["dk"] + h.transpose(-1, -2) @ q.abs()
    # the magnitude terms the fp32 bounds are held against (<= 2^-10 of them, test_attn_cases_host.py): the sums of the bf16 bounds
    # above - for dQ and dK that is 2 sum |dS| |k| + ch^-0.5 D sum p |k| (sum |dS| |k| alone vanishes where dP and delta cancel,
    # while the fp32 error of dP - delta, the (ch + 4) 2^-24 term of g, does not)
    mag["dq"] = 2 * mag["dq"] + scale * D.unsqueeze(-1) * (p @ k.abs())
    mag["dk"] = 2 * mag["dk"] + scale * (p * D.unsqueeze(-1)).transpose(-1, -2) @ q.abs()
    for n in ("out", "dv", "dq", "dk"):
        b["mag_" + n], b["f32_" + n] = mag[n], f32[n]
    return b


# ----------------------------------------------------------------------------- rounding model of the bf16 kernels
MUTATIONS = ("drop_last_key", "drop_key_tile", "skip_l_rescale", "v_from_next_head", "k_from_next_head", "no_delta", "lse_of_next_block")


def mutation_applies(mut, case):
    B, T, H, ch = case
    if mut in ("v_from_next_head", "k_from_next_head"):
        return H > 1
    if mut in ("drop_key_tile", "lse_of_next_block"):
        return T > 128                    # a second query block
    if mut == "skip_l_rescale":
        return T > fwd_kt(ch)             # a second key tile
    return True


def model(case, mut=None, dtype=BF16, round_p=None):
    """Plain-torch emulation of the bf16 kernels' rounding points: logits, exp2, l and the accumulators fp32; P and dS rounded to
    bf16 where they become MFMA operands; delta from the bf16 O; outputs rounded to bf16; key tiles (forward, dQ) and query tiles
    (dK, dV) walked in the kernels' order with k_attn_bf16's tile length.  The backward is fed the reference's O (bf16) and lse
    (fp32), as the GPU test feeds the kernels.  `mut` applies one of MUTATIONS.  dtype = F32: the same walk on the fp32 operands
    without the bf16 roundings (the fp32 kernels keep P and dS in their accumulator registers); round_p = True puts the
    roundings of P, dS and the outputs back on fp32 operands: an fp32 kernel of lowered precision, which the fp32 bounds must
    reject.  Returns float64 out, lse, dq, dk, dv."""
    o, r = operands(case, dtype), reference(case, dtype)
    round_p = (dtype == BF16) if round_p is None else round_p
    _bf = (lambda t: t.to(BF16).float()) if round_p else (lambda t: t)
    B, T, H, ch = case
    KT = fwd_kt(ch)
    q, k, v, do = (o[n].float() for n in ("q", "k", "v", "do"))
    if mut == "v_from_next_head":
        v = v.roll(1, dims=1)
    if mut == "k_from_next_head":
        k = k.roll(1, dims=1)
    sc = torch.tensor(LOG2E / math.sqrt(ch), dtype=torch.float32)
    scale = torch.tensor(1.0 / math.sqrt(ch), dtype=torch.float32)
    live = torch.ones(T, T, dtype=torch.bool)                       # [query, key] pairs the (mutated) kernel looks at
    if mut == "drop_last_key":
        live[:, T - 1] = False
    if mut == "drop_key_tile":
        live[128:256, KT:2 * KT] = False                            # the second key tile, for the second query block
    # ---- forward
    m = torch.full((B, H, T), float("-inf"))
    l = torch.zeros(B, H, T)
    acc = torch.zeros(B, H, T, ch)
    for ti, kt0 in enumerate(range(0, T, KT)):
        sl = slice(kt0, min(kt0 + KT, T))
        s = (q @ k[:, :, sl].transpose(-1, -2)).masked_fill(~live[:, sl], float("-inf"))
        m_new = torch.maximum(m, s.max(-1).values * sc)
        alpha = torch.exp2(m - m_new)
        if not (mut == "skip_l_rescale" and kt0 + KT >= T):         # the last tile: what an earlier one adds to l is scaled away later
            l = l * alpha
        acc = acc * alpha.unsqueeze(-1)
        m = m_new
        pv = torch.exp2((s.double() * sc.double() - m.double().unsqueeze(-1)).float())       # one rounding, as the fma
        l = l + pv.sum(-1)
        acc = acc + _bf(pv) @ v[:, :, sl]
    out = _bf(acc / l.unsqueeze(-1))
    lse = m + torch.log2(l)
    # ---- backward from the reference's O and lse
    o_in, lse_in = r["o_in"].float(), r["lse_in"]
    if mut == "lse_of_next_block":
        lse_in = lse_in.roll(-128, -1)
    delta = torch.zeros(B, H, T) if mut == "no_delta" else (do * o_in).sum(-1)
    ndel = -(delta * scale)
    s = q @ k.transpose(-1, -2)
    pv = torch.exp2((s.double() * sc.double() - lse_in.double().unsqueeze(-1)).float()).masked_fill(~live, 0.0)
    dp = do @ v.transpose(-1, -2)
    dsv = pv * (dp.double() * scale.double() + ndel.double().unsqueeze(-1)).float()
    pb, dsb = _bf(pv), _bf(dsv)
    dq = torch.zeros(B, H, T, ch)
    for kt0 in range(0, T, KT):
        sl = slice(kt0, min(kt0 + KT, T))
        dq = dq + dsb[..., sl] @ k[:, :, sl]
    dk = torch.zeros(B, H, T, ch)
    dv = torch.zeros(B, H, T, ch)
    for qt0 in range(0, T, KT):
        sl = slice(qt0, min(qt0 + KT, T))
        dk = dk + dsb[:, :, sl].transpose(-1, -2) @ q[:, :, sl]
        dv = dv + pb[:, :, sl].transpose(-1, -2) @ do[:, :, sl]
    return dict(out=out.double(), lse=lse.double(), dq=_bf(dq).double(), dk=_bf(dk).double(), dv=_bf(dv).double())


def ratios(got, case, dtype, b=None, names=("out", "lse", "dq", "dk", "dv")):
    """Largest |got - reference| / bound per output (inf where an element is NaN)."""
    r = reference(case, dtype)
    b = bounds(case, dtype) if b is None else b
    out = {}
    for n in names:
        if n in got:
            x = ((got[n].double() - r[n]).abs() / b[n])
            out[n] = float(torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x).max())
    return out


# ----------------------------------------------------------------------------- conditions on the inputs
def forward_kts(ch):
    """Keys per tile of the forward kernels a case runs: {k_attn_bf16, k_attn_f32m} (they skip the rescale where no query of a wave
    saw a new maximum) and k_attn_f32 (it rescales on every tile)."""
    return sorted({fwd_kt(ch), 64 if ch <= 64 else 32}), (64 if ch <= 64 else (32 if ch == 128 else 16))


def input_stats(case, dtype, KT=None):
    """Judged on the fp64 reference: median effective key count per (b, h); per query, the number of key tiles after the first on
    which the running maximum rises (tiles of KT keys); 'level_tiles': the tiles after the first in which a whole 32-key level of
    the staircase begins (a tile that only continues a level, or holds a ragged last one, need not raise anything)."""
    r = reference(case, dtype)
    B, T, H, ch = case
    KT = fwd_kt(ch) if KT is None else KT
    neff = (1.0 / (r["p"] ** 2).sum(-1)).median(-1).values                  # [B, H]
    run = torch.full((B, H, T), float("-inf"), dtype=torch.float64)
    rises = torch.zeros(B, H, T, dtype=torch.long)
    for ti, kt0 in enumerate(range(0, T, KT)):
        mx = r["s2"][..., kt0:kt0 + KT].max(-1).values
        if ti > 0:
            rises += (mx > run).long()
        run = torch.maximum(run, mx)
    level_tiles = sum(1 for kt0 in range(KT, T, KT) if any(kt0 <= L < kt0 + KT and L + 32 <= T for L in range(0, T, 32)))
    return dict(neff=neff, rises=rises, level_tiles=level_tiles)
