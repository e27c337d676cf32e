"""Cases, operands, fp64 references and a plain-torch model of the LayerNorm kernels of csrc/vit.hip (rho_layernorm_fwd / _bwd), for
test_ln_cases_host.py (CPU) and test_gpu_exact_layernorm.py (-m gpu).  Nothing here touches the GPU.

Geometry.  ln_geom / ln_bps below are Python twins of the functions of the same names in vit.hip: G lanes share a row, each holds NV
16-byte vectors (PE = 4 float32 or 8 bf16 elements), a block of 256 threads holds rpb = 256 / G rows; the backward launches
(bps, nb) blocks and block (k, b) sweeps the row groups k, k + bps, ... of sample b.  The GPU test checks the twin against
rho_layernorm_bwd_workspace_bytes = nb * bps * 3 * E * 4, so the branch each case names is known to be reached, not assumed.

Backward operands.  mean and rstd are INPUTS at the C ABI, so the cases hand the kernel an integer mean and rstd in {0.5, 1, 2} per
row, integer x (+ integer add), integer gamma and integer dy in [-2, 2].  Then xhat = (x + add - mean) * rstd lies on a grid of 1/2,
dy * xhat and dy are exact, and every column sum (dgamma, dbeta: over all rows; the partial rows: over a block's rows) is exact in
fp32 in ANY order: those outputs must equal fp64 bit for bit.  For dx = rstd (g - m1 - xhat m2), g = dy gamma, m1 = sum(g) / E,
m2 = sum(g xhat) / E: the kernel multiplies the exact row sums by fl(1 / E).  For E a power of two that factor is exact, so m1 is on
a grid of 1 / E and m2 on 1 / (2E) for ANY integer sums (no repair of the row tails is needed to put them on a grid), g - m1 has at
most 2^3 E steps, xhat m2 at most 2^24 steps of 1 / (4E) (asserted per case by the host twin), and dx - and dadd, its exact column
sum - is exact in fp32 whether or not the compiler fuses the products: bit equality.  For the other widths (96, 160, 1056)
fl(1 / E) is inexact, no choice of the sums makes m1 exact in general, and dx is held to the per-element bound DX_ULPS below.

Forward operands.  Integer x (+ integer add) whose rows sum to E * k with k an integer in [-3, 3] (the tails are repaired by
zero_sum_rows), so the mean is the integer k, x - mean is exact and the variance sum is an exact integer."""
from __future__ import annotations

import math

import torch

from exact_util import int_choice, int_tensor

F32, BF16 = torch.float32, torch.bfloat16
LN_EPS = 1e-5
LN_MAX_E = 2048
U = 2.0 ** -24

# ---- bounds, counted from the roundings of the kernels (fp32 ulps; u |v| < ulp32(v) for every relative rounding error u = 2^-24) --
# rstd = 1 / sqrtf(var + eps), var = sq / E with sq an exact integer: the division rounds (1), the addition rounds (2) - both enter
# the inverse square root halved, together 1 u -, sqrtf rounds (2 u), the final division rounds (3 u).  The kernel's eps is
# fl32(1e-5), 2.6e-13 from 1e-5: with var >= 1 (asserted by the host twin) that is below 2e-13 relative, 3e-6 ulp.
RSTD_ULPS = 3
# y = fma((x - mean) * rstd, gamma, beta): x - mean exact, rstd carries 3 u, the product rounds (4 u on |xhat gamma|), the fma rounds
# its result once (1 u on |y| <= |xhat gamma| + |beta|): 5 u of Mag = |xhat gamma| + |beta|.
Y_ULPS = 5
# dx where fl(1 / E) is inexact, against Mag = |g| + |m1| + |xhat m2| (times rstd, a power of two):
#   m1 = s1 * fl(1 / E): 2 roundings; g - m1 rounds once: <= u (|g| + |m1|) + 2 u |m1|;
#   m2 likewise 2 u; xhat * m2 rounds once where it is not fused (3 u |xhat m2|); the last subtraction rounds once (u Mag):
#   <= u (2 |g| + 4 |m1| + 4 |xhat m2|) <= 4 u Mag.
DX_ULPS = 4


def pe_of(dtype) -> int:
    return 8 if dtype == BF16 else 4


def ln_geom(e: int, dtype) -> dict:
    pe = pe_of(dtype)
    nvec = e // pe
    G = 4
    while G < nvec and G < 64:
        G *= 2
    per = -(-nvec // G)
    NV = 1
    while NV < per:
        NV *= 2
    return dict(PE=pe, nvec=nvec, G=G, NV=NV, rpb=256 // G)


def ln_bps(nb: int, rps: int, rpb: int) -> int:
    want = -(-rps // rpb)
    cap = max(1, 1024 // nb)
    return min(want, cap)


def ln_layout(c: dict, dtype) -> dict:
    """Everything the launch of case c decides: geometry, samples, blocks per sample, sweeps of the row loop."""
    g = ln_geom(c["E"], dtype)
    rps = c["rps"] if c["add"] else c["rows"]
    nb = c["rows"] // rps
    bps = ln_bps(nb, rps, g["rpb"])
    groups = -(-rps // g["rpb"])
    g.update(rps=rps, nb=nb, bps=bps, groups=groups, sweeps=-(-groups // bps), workspace_bytes=nb * bps * 3 * c["E"] * 4)
    return g


# ---- the branch each case exists for: a predicate over the layout, asserted before any launch --------------------------------------
def _last_sweep(L):
    """(blocks that run the last sweep, live slots of its last block)."""
    in_last = L["groups"] - (L["sweeps"] - 1) * L["bps"]
    tail = L["rps"] - (L["groups"] - 1) * L["rpb"]
    return in_last, tail


BRANCHES = {
    "e32": lambda c, L: c["E"] == 32 and L["G"] == (4 if L["PE"] == 8 else 8) and L["NV"] == 1,
    "idle_lanes": lambda c, L: L["NV"] == 1 and L["G"] > L["nvec"],
    # one vector index j is live in some lanes and dead in others (and, where NV exceeds ceil(nvec / G), later ones are dead in all)
    "ragged": lambda c, L: L["NV"] > 1 and L["nvec"] % L["G"] != 0,
    "max_width": lambda c, L: c["E"] == LN_MAX_E and L["NV"] == (4 if L["PE"] == 8 else 8) and L["rpb"] * c["E"] == 8192,
    "full_lanes": lambda c, L: L["NV"] == 1 and L["G"] == L["nvec"],
    "rows_not_rpb": lambda c, L: L["rps"] % L["rpb"] != 0 and L["rps"] > L["rpb"],
    "one_row": lambda c, L: c["rows"] == 1,
    # three or more sweeps; the last one has a partly live block, and (bps > 1) a block that has no row group left
    "sweeps_idle_block": lambda c, L: L["sweeps"] >= 3 and 0 < _last_sweep(L)[1] < L["rpb"] and _last_sweep(L)[0] < L["bps"],
    "sweeps_one_block": lambda c, L: L["sweeps"] >= 3 and 0 < _last_sweep(L)[1] < L["rpb"] and L["bps"] == 1,
}


def _case(name, E, rows, rps, add, branch, dadd=None, acc_dx=False, acc_params=False, dtypes=(F32, BF16)):
    return dict(name=name, E=E, rows=rows, rps=rps, add=add, dadd=add if dadd is None else dadd, acc_dx=acc_dx, acc_params=acc_params,
                branch=branch, dtypes=tuple(dtypes))


# The smallest shapes that reach each branch (rps: rows per sample; without `add` the whole tensor is one sample).
LN_CASES = [
    _case("e32_add", 32, 3 * 70, 70, True, "e32", acc_dx=True),
    _case("e32_plain_acc", 32, 77, 77, False, "e32", acc_params=True),
    _case("e96_idle", 96, 2 * 13, 13, True, "idle_lanes", dadd=False),
    _case("e160_idle", 160, 11, 11, False, "idle_lanes", acc_dx=True, acc_params=True),
    _case("e256_full", 256, 3 * 9, 9, True, "full_lanes", acc_params=True),
    _case("e1056_ragged", 1056, 2 * 7, 7, True, "ragged", acc_dx=True),
    _case("e1056_ragged_plain", 1056, 5, 5, False, "ragged"),
    _case("e2048_max", 2048, 2 * 6, 6, True, "max_width", acc_dx=True, acc_params=True),
    _case("e2048_max_plain", 2048, 7, 7, False, "max_width"),
    _case("e256_ragged_rows", 256, 2 * 21, 21, True, "rows_not_rpb"),
    _case("e32_one_row", 32, 1, 1, False, "one_row"),
    _case("e2048_one_row", 2048, 1, 1, True, "one_row", acc_dx=True),
    _case("e1024_sweeps", 1024, 512 * 19, 19, True, "sweeps_idle_block"),
    _case("e32_sweeps", 32, 1024 * 70, 70, True, "sweeps_one_block", acc_params=True, dtypes=(F32,)),
]
# widths at which dx and dadd must be bit-equal (fl(1 / E) exact): the smallest, a mid-size and the largest width, and the sweep case's
EXACT_DX_WIDTHS = (32, 256, 1024, 2048)

LN_PARAMS = [(c, dt) for c in LN_CASES for dt in c["dtypes"]]


def case_id(c, dtype) -> str:
    return f"{c['name']}-{'bf16' if dtype == BF16 else 'f32'}"


def dx_is_exact(c) -> bool:
    return c["E"] in EXACT_DX_WIDTHS


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def ln_bwd_operands(c) -> dict:
    """Integer operands of the backward (the same for both dtypes: every value is exact in bf16) and the prefills of the
    accumulating modes."""
    R, E, n = c["rows"], c["E"], c["name"]
    nb = R // c["rps"] if c["add"] else 1
    o = dict(x=int_tensor((R, E), f"lnc_x_{n}", 6.0, 15.0),
             dy=int_choice((R, E), f"lnc_dy_{n}", (-2.0, -1.0, 0.0, 1.0, 2.0)),
             gamma=int_choice((E,), f"lnc_g_{n}", (-2.0, -1.0, 1.0, 2.0)),
             mean=int_choice((R,), f"lnc_m_{n}", (-3.0, -1.0, 0.0, 2.0)),
             rstd=int_choice((R,), f"lnc_r_{n}", (0.5, 1.0, 2.0)),
             add=int_tensor((nb, E), f"lnc_a_{n}", 1.0, 2.0) if c["add"] else None,
             pre_dx=int_choice((R, E), f"lnc_pdx_{n}", (-3.0, 0.0, 1.0, 5.0)),
             pre_dgamma=int_choice((E,), f"lnc_pdg_{n}", (-7.0, 0.0, 3.0)),
             pre_dbeta=int_choice((E,), f"lnc_pdb_{n}", (-5.0, 0.0, 11.0)))
    return o


def _rows_of_samples(t, rps):
    return t.repeat_interleave(rps, 0)


def ln_bwd_reference(c, o) -> dict:
    """fp64, straight from the formulas (no block structure): xhat, g, m1, m2, dx (before and after the prefill), dgamma, dbeta,
    dadd, and the magnitude sum the DX_ULPS bound counts against."""
    E = c["E"]
    x, dy = o["x"].double(), o["dy"].double()
    if c["add"]:
        x = x + _rows_of_samples(o["add"].double(), c["rps"])
    mean, rstd = o["mean"].double()[:, None], o["rstd"].double()[:, None]
    xh = (x - mean) * rstd
    g = dy * o["gamma"].double()
    m1, m2 = g.sum(1, keepdim=True) / E, (g * xh).sum(1, keepdim=True) / E
    dx0 = rstd * (g - m1 - xh * m2)
    r = dict(xhat=xh, g=g, m1=m1, m2=m2, dx_new=dx0, dx=dx0 + o["pre_dx"].double() if c["acc_dx"] else dx0,
             dx_mag=rstd * (g.abs() + m1.abs() + (xh * m2).abs()),
             dgamma=(dy * xh).sum(0) + (o["pre_dgamma"].double() if c["acc_params"] else 0.0),
             dbeta=dy.sum(0) + (o["pre_dbeta"].double() if c["acc_params"] else 0.0))
    if c["add"]:
        r["dadd"] = dx0.reshape(-1, c["rps"], E).sum(1)
        r["dadd_mag"] = r["dx_mag"].reshape(-1, c["rps"], E).sum(1)
    return r


MUTATIONS_BWD = ("second_sweep_dropped", "slot_skipped", "m2_omitted")
MUTATIONS_FWD = ("ragged_read_as_live",)


def ln_bwd_model32(c, o, dtype, mutation=None) -> dict:
    """The kernel's operation sequence in torch float32 with the kernel's block structure: rows are dealt to (sample b, block k, sweep,
    slot), a block's rows are added into the partial row [b][k][comp][E] (comp 0: dy xhat, 1: dy, 2: dx), k_ln_bwd_fin adds the
    partial rows.  Products are not fused; where the host twin demands equality with fp64 every intermediate is exact, so fusing
    changes nothing.  `mutation` breaks the model the way a wrong kernel would (test_ln_cases_host.py proves each is noticed)."""
    L = ln_layout(c, dtype)
    E, R, rps, rpb, bps, nb = c["E"], c["rows"], L["rps"], L["rpb"], L["bps"], L["nb"]
    x, dy = o["x"].float(), o["dy"].float()
    if c["add"]:
        x = x + _rows_of_samples(o["add"].float(), rps)
    mean, rstd = o["mean"].float()[:, None], o["rstd"].float()[:, None]
    inv_e = torch.tensor(1.0, dtype=F32) / torch.tensor(float(E), dtype=F32)
    xh = (x - mean) * rstd
    g = dy * o["gamma"].float()
    m1 = g.sum(1, keepdim=True) * inv_e
    m2 = (g * xh).sum(1, keepdim=True) * inv_e
    if mutation == "m2_omitted":
        m2 = torch.zeros_like(m2)
    dx0 = rstd * (g - m1 - xh * m2)
    rl = torch.arange(R) % rps
    b = torch.arange(R) // rps
    group = rl // rpb
    k, sweep, slot = group % bps, group // bps, rl % rpb
    keep = torch.ones(R, dtype=torch.bool)
    if mutation == "second_sweep_dropped":
        keep &= sweep != 1
    if mutation == "slot_skipped":
        keep &= slot != min(1, rpb - 1)
    part = torch.zeros(nb * bps, 3, E, dtype=F32)
    idx = (b * bps + k)[keep]
    part[:, 0].index_add_(0, idx, (dy * xh)[keep])
    part[:, 1].index_add_(0, idx, dy[keep])
    part[:, 2].index_add_(0, idx, dx0[keep])
    out = dict(part=part.reshape(nb, bps, 3, E), m1=m1, m2=m2, dx_new=dx0,
               dx=dx0 + o["pre_dx"].float() if c["acc_dx"] else dx0,
               dgamma=part[:, 0].sum(0) + (o["pre_dgamma"].float() if c["acc_params"] else 0.0),
               dbeta=part[:, 1].sum(0) + (o["pre_dbeta"].float() if c["acc_params"] else 0.0))
    if c["add"]:
        out["dadd"] = part[:, 2].reshape(nb, bps, E).sum(1)
    return out


def zero_sum_rows(z: torch.Tensor) -> torch.Tensor:
    """Integer rows repaired to sum to zero: the deficit d of a row is spread as sign(d) * (|d| // E) over all and one more step over
    the first |d| % E elements."""
    E = z.shape[1]
    d = -z.sum(1).long()
    q, r = d.abs() // E, d.abs() % E
    sgn = torch.sign(d).to(z.dtype)[:, None]
    out = z + sgn * q.to(z.dtype)[:, None] + sgn * (torch.arange(E)[None, :] < r[:, None]).to(z.dtype)
    assert bool((out.sum(1) == 0).all())
    return out


def ln_fwd_operands(c) -> dict:
    """Integer x (+ integer add) with row sums E * k, k in [-3, 3]; integer gamma and beta."""
    R, E, n = c["rows"], c["E"], c["name"]
    nb = R // c["rps"] if c["add"] else 1
    k = int_choice((R, 1), f"lnf_k_{n}", (-3.0, -1.0, 0.0, 2.0))
    return dict(x=zero_sum_rows(int_tensor((R, E), f"lnf_x_{n}", 2.0, 4.0)) + k, k=k[:, 0],
                add=zero_sum_rows(int_tensor((nb, E), f"lnf_a_{n}", 1.0, 2.0)) if c["add"] else None,
                gamma=int_choice((E,), f"lnf_g_{n}", (-2.0, -1.0, 1.0, 3.0)),
                beta=int_choice((E,), f"lnf_b_{n}", (-4.0, 0.0, 1.0, 2.0)))


def ln_fwd_reference(c, o, dtype=F32, mutation=None) -> dict:
    """fp64: mean, var, rstd, y and Mag = |xhat gamma| + |beta|.  mutation "ragged_read_as_live" (needs dtype for the geometry)
    lets the lanes past the row's last vector read on into the next row, as a kernel without the `vi < nvec` test would."""
    E = c["E"]
    x = o["x"].double()
    if c["add"]:
        x = x + _rows_of_samples(o["add"].double(), c["rps"])
    mean = x.sum(1) / E
    if mutation == "ragged_read_as_live":
        L = ln_geom(E, dtype)
        span = L["G"] * L["NV"] * L["PE"]
        flat = torch.cat([x.reshape(-1), torch.zeros(span, dtype=torch.float64)])
        starts = torch.arange(x.shape[0]) * E
        mean = torch.stack([flat[s:s + span].sum() for s in starts.tolist()]) / E
    d = x - mean[:, None]
    var = (d * d).sum(1) / E
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xh = d * rstd[:, None]
    ga, be = o["gamma"].double(), o["beta"].double()
    return dict(mean=mean, var=var, sq=(d * d).sum(1), rstd=rstd, y=xh * ga + be, y_mag=(xh * ga).abs() + be.abs())
