"""Cases, operands and fp64 references of the legacy-UNet tail of csrc/unet_v1.hip (rho_groupnorm_act / _bwd, rho_act_add,
rho_act_bwd), for test_ln_cases_host.py (CPU) and test_gpu_exact_v1_tail.py (-m gpu).  Nothing here touches the GPU.

k_gn_groups_fwd / _bwd run one workgroup per (group, sample) over m = S * cpg elements, element e -> (row e / cpg, channel e % cpg),
thread tid takes e = tid, tid + 256, ...  The forward adds fp32 runs of 64 elements per thread and carries each run into fp64, so
the carry runs only where a thread has more than 64 elements, m > 16384; the backward keeps its channel sums in LDS [2 * cpg] and
walks the channels with `j += 256`, so cpg > 256 takes a second pass.

Forward operands: integer x whose groups sum to m * k, k an integer (ln_cases.zero_sum_rows), so the mean is the integer k,
x - mean is exact and both fp32 run sums are exact integers.  Backward operands: stats are inputs - integer mean, rstd in
{0.5, 1, 2} - with integer x, dy in [-2, 2], integer gamma / beta, act 0: gq = dy, xhat on a grid of 1/2, the LDS and global float
atomics add exact values in any order, so dgamma / dbeta equal fp64 bit for bit; m1 = (float)(s1 / m), m2 likewise with s1, s2 exact
fp64 sums: representable where m is a power of two (dx bit-equal, proven by the host twin), else dx is held to V1_DX_ULPS."""
from __future__ import annotations

import torch

from exact_util import int_choice, int_tensor
from ln_cases import BF16, F32, zero_sum_rows

V1_EPS = 1e-5
# rstd = (float)(1 / sqrt(var + eps)) from exact sums combined in fp64 (the one-pass var = sq / m - mean^2 loses at most
# E[x^2] / var * 2^-52 relative, far below an fp32 ulp): only the rounding to fp32 remains, so at most 1 ulp from the fp64 reference
# rounded to fp32 by derivation (the two fp64 values can straddle a rounding boundary).  eps arrives as fl32(1e-5), 2.6e-13 from
# 1e-5: nothing against var >= 0.5 (asserted by the host twin).  Measured on an MI355X: equal to the rounded reference in every
# case (at most 0.49 ulp from the unrounded one), so the tests ask for 0, as test_gpu_exact_groupnorm.py does for its statistics - an
# equality of these inputs: exactly 1 ulp after a change of the operands means the data moved.
V1_RSTD_ULPS = 0
# y = fma((x - mean) * rstd, gamma, beta) at act 0: x - mean exact, rstd carries 1 u (its rounding), the product rounds (2 u on
# |xhat gamma|), the fma rounds once (1 u on |y|): 3 u of Mag = |xhat gamma| + |beta|.
V1_Y_ULPS = 3
# dx = rstd (gamma gq - m1 - xhat m2) where m is no power of two: gamma gq exact; m1, m2 rounded once each from fp64; the first
# subtraction rounds (u (|g| + |m1|) + u |m1|), xhat m2 rounds where it is not fused (2 u |xhat m2|), the last subtraction rounds
# (u Mag): <= 3 u Mag, Mag = |g| + |m1| + |xhat m2|, times rstd (a power of two).
V1_DX_ULPS = 3


def _case(name, N, S, C, groups, why):
    cpg = C // groups
    return dict(name=name, N=N, S=S, C=C, groups=groups, cpg=cpg, m=S * cpg, why=why)


V1_CASES = [
    _case("cpg1", 2, 37, 8, 8, "cpg = 1"),
    _case("cpg1_pow2", 2, 64, 8, 8, "cpg = 1, m = 64: dx bit-equal"),
    _case("cpg3", 3, 35, 12, 4, "cpg = 3, no power of two"),
    _case("cpg32_pow2", 2, 16, 64, 2, "cpg = 32, m = 512: dx bit-equal"),
    _case("cpg32_carry", 2, 521, 64, 2, "m = 16672 > 16384: every thread has 65 or 66 elements, the fp32 run of 64 is carried"),
    _case("cpg260", 2, 5, 520, 2, "cpg = 260 > 256: a second pass of the j += 256 loops, LDS 512 * 8 + 2 * 260 * 4"),
    _case("s1", 3, 1, 24, 2, "S = 1, cpg = 12"),
]


def dx_is_exact(c) -> bool:
    return (c["m"] & (c["m"] - 1)) == 0


def lds_bytes(c) -> int:
    return 512 * 8 + 2 * c["cpg"] * 4


def per_thread(c) -> int:
    """The most elements a thread of the workgroup walks."""
    return -(-c["m"] // 256)


def _group_view(x, c):
    """[N, S, C] -> [N * groups, S * cpg] (a copy)."""
    N, S, G, cpg = c["N"], c["S"], c["groups"], c["cpg"]
    return x.reshape(N, S, G, cpg).permute(0, 2, 1, 3).reshape(N * G, S * cpg)


def _from_groups(v, c):
    N, S, G, cpg = c["N"], c["S"], c["groups"], c["cpg"]
    return v.reshape(N, G, S, cpg).permute(0, 2, 1, 3).reshape(N, S, c["C"]).contiguous()


def v1_fwd_operands(c) -> dict:
    n = c["name"]
    z = zero_sum_rows(_group_view(int_tensor((c["N"], c["S"], c["C"]), f"v1f_x_{n}", 2.0, 4.0), c))
    k = int_choice((z.shape[0], 1), f"v1f_k_{n}", (-3.0, -1.0, 0.0, 2.0))
    return dict(x=_from_groups(z + k, c), k=k[:, 0].reshape(c["N"], c["groups"]),
                gamma=int_choice((c["C"],), f"v1f_g_{n}", (-2.0, -1.0, 1.0, 3.0)),
                beta=int_choice((c["C"],), f"v1f_b_{n}", (-8.0, 0.0, 8.0, 16.0)))      # |xhat gamma| < 8: no sum cancels to near zero


def v1_fwd_reference(c, o) -> dict:
    xg = _group_view(o["x"].double(), c)
    mean = xg.sum(1) / c["m"]
    d = xg - mean[:, None]
    sq = (d * d).sum(1)
    rstd = 1.0 / torch.sqrt(sq / c["m"] + V1_EPS)
    xh = _from_groups(d * rstd[:, None], c)
    ga, be = o["gamma"].double(), o["beta"].double()
    shp = (c["N"], c["groups"])
    return dict(mean=mean.reshape(shp), rstd=rstd.reshape(shp), var=(sq / c["m"]).reshape(shp), sumsq=(xg * xg).sum(1),
                y=xh * ga + be, y_mag=(xh * ga).abs() + be.abs())


def v1_fwd_sums_model(c, o, mutation=None):
    """(sum x, sum x^2) per (n, group) the way k_gn_groups_fwd adds them: thread tid takes e = tid, tid + 256, ...; fp32 runs of 64
    elements are carried into an fp64 total, the tail run is added at the end, thread totals are added in fp64.  mutation
    "carry_not_flushed": a full run is reset without being added."""
    xg = _group_view(o["x"].float(), c)
    per = per_thread(c)
    pad = torch.zeros(xg.shape[0], per * 256, dtype=F32)
    pad[:, :c["m"]] = xg
    t = pad.reshape(-1, per, 256)                                  # [groups, i, tid]: element tid + 256 i
    cnt = torch.full((256,), c["m"] // 256) + (torch.arange(256) < c["m"] % 256)      # elements per thread
    su = torch.zeros(xg.shape[0], 256, dtype=torch.float64)
    sq = torch.zeros_like(su)
    for i0 in range(0, per, 64):
        run, runq = t[:, i0:i0 + 64].sum(1), (t[:, i0:i0 + 64] * t[:, i0:i0 + 64]).sum(1)             # fp32
        full = (cnt >= i0 + 64)[None, :]
        if mutation == "carry_not_flushed":
            run, runq = torch.where(full, torch.zeros_like(run), run), torch.where(full, torch.zeros_like(runq), runq)
        su += run.double()
        sq += runq.double()
    return su.sum(1), sq.sum(1)


def v1_bwd_operands(c) -> dict:
    n = c["name"]
    return dict(x=int_tensor((c["N"], c["S"], c["C"]), f"v1b_x_{n}", 3.0, 8.0),
                dy=int_choice((c["N"], c["S"], c["C"]), f"v1b_dy_{n}", (-2.0, -1.0, 0.0, 1.0, 2.0)),
                gamma=int_choice((c["C"],), f"v1b_g_{n}", (-2.0, -1.0, 1.0, 2.0)),
                beta=int_choice((c["C"],), f"v1b_b_{n}", (-1.0, 0.0, 3.0)),
                mean=int_choice((c["N"], c["groups"]), f"v1b_m_{n}", (-3.0, -1.0, 0.0, 2.0)),
                rstd=int_choice((c["N"], c["groups"]), f"v1b_r_{n}", (0.5, 1.0, 2.0)),
                pre_dgamma=int_choice((c["C"],), f"v1b_pg_{n}", (-7.0, 3.0, 64.0)),
                pre_dbeta=int_choice((c["C"],), f"v1b_pb_{n}", (-5.0, 11.0, 32.0)))


def v1_bwd_reference(c, o, dtype64=torch.float64) -> dict:
    """act 0 (gq = dy).  dtype64 = torch.float32 evaluates the same formulas in float32 (m1, m2 from exact sums rounded once), the
    host twin's model of the kernel."""
    cpg = c["cpg"]
    x, dy = o["x"].double(), o["dy"].double()
    mean = o["mean"].double().repeat_interleave(cpg, 1)[:, None, :]
    rstd = o["rstd"].double().repeat_interleave(cpg, 1)[:, None, :]
    ga = o["gamma"].double()
    xh = (x - mean) * rstd
    g = dy * ga
    s1 = _group_view(g, c).sum(1) / c["m"]
    s2 = _group_view(g * xh, c).sum(1) / c["m"]
    if dtype64 == F32:
        s1, s2 = s1.float().double(), s2.float().double()
    m1 = s1.reshape(c["N"], c["groups"]).repeat_interleave(cpg, 1)[:, None, :]
    m2 = s2.reshape(c["N"], c["groups"]).repeat_interleave(cpg, 1)[:, None, :]
    if dtype64 == F32:
        xm = (xh.float() * m2.float())
        dx = (rstd.float() * ((g.float() - m1.float()) - xm)).double()
    else:
        dx = rstd * (g - m1 - xh * m2)
    return dict(xhat=xh, g=g, m1=m1, m2=m2, dx=dx, dx_mag=rstd * (g.abs() + m1.abs() + (xh * m2).abs()),
                dgamma=(dy * xh).sum((0, 1)) + o["pre_dgamma"].double(), dbeta=dy.sum((0, 1)) + o["pre_dbeta"].double(),
                dgamma_mag=(dy * xh).abs().sum((0, 1)) + o["pre_dgamma"].double().abs())


# rho_act_add addends: integer operands, act 0 / 2, N > 1, C = 24 (256 % 24 != 0: a block's 256 elements start at any channel)
ACT_ADD_SHAPE = (3, 7, 24)


def act_add_operands() -> dict:
    N, S, C = ACT_ADD_SHAPE
    return dict(x=int_tensor((N, S, C), "v1aa_x", 8.0, 60.0), r=int_tensor((N, S, C), "v1aa_r", 8.0, 60.0),
                nc=int_tensor((N, C), "v1aa_nc", 8.0, 60.0))
