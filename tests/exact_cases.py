"""Case tables and CPU references of the integer-operand tests: imported by test_exact_cases_host.py (which proves, without a GPU,
that every reference stays inside the representability caps and that fp32 == fp64 on the CPU) and by the -m gpu modules
test_gpu_exact_conv.py / test_gpu_exact_backward.py / test_gpu_exact_attention.py.

Every tensor is [N, C, D, H, W] on the CPU here (1-D / 2-D layers carry leading spatial axes of 1, as the kernels see them);
geometries are the smallest ones of the tolerance tests' tables (CONV_CASES, WIDE_CONV, PHASE_CASES, S2_CASES, GEMM_CASES, the conv32
edge geometries, the k-split CASES, BWD_CASES).  The GroupNorm passes (GN_CASES and below; test_gpu_exact_groupnorm.py) work on
channels-last [N, S, C] tensors, as the kernels of groupnorm.hip see them."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from detdata import det_normal, det_uniform
from exact_util import int_choice, int_tensor

F32, BF16 = torch.float32, torch.bfloat16
BOTH = (F32, BF16)


def _case(name, N, spatial, c1, cout, kernel=(3, 3, 3), c2=0, stride=(1, 1), up=(0, 0), pre=False, res=False, add=False, split=None,
          y2="cm", res2=False, skip=None, stats=False, dtypes=BOTH, w_scale=0.45, ksplit=False):
    sp = (1,) * (3 - len(spatial)) + tuple(spatial)
    return dict(name=name, N=N, spatial=sp, c1=c1, c2=c2, cout=cout, kernel=tuple(kernel), stride=tuple(stride), up=tuple(up), pre=pre,
                res=res, add=add, split=cout if split is None else split, y2=y2, res2=res2, skip=skip, stats=stats, dtypes=tuple(dtypes),
                w_scale=w_scale, ksplit=ksplit)


# ----------------------------------------------------------------------------- forward launches (one rho_conv_nd_fwd each)
FWD_CASES = [
    # k_conv 3x3x3: bf16 takes the 16x16x32 layout (M16=1) at BM = 64 / 128, fp32 and BM = 32 the 32x32 one
    _case("3d_basic", 2, (4, 8, 8), 32, 64, stats=True, w_scale=0.35),
    _case("3d_bm128", 1, (4, 8, 8), 32, 128, pre=True, add=True, w_scale=0.35),
    _case("3d_ragged", 1, (5, 6, 7), 64, 32, pre=True, res=True, stats=True, w_scale=0.27),
    _case("3d_tile512_ragged", 2, (9, 10, 13), 64, 64, c2=32, pre=True, res=True, w_scale=0.35),
    # virtual concat whose boundary falls inside a pair of K chunks (bf16: chunks 3 | 1; fp32: 48 | 16 = chunks 3 | 1)
    _case("concat_straddle_bf16", 2, (4, 8, 8), 96, 64, c2=32, pre=True, dtypes=(BF16,), w_scale=0.35),
    _case("concat_straddle_f32", 2, (4, 8, 8), 48, 64, c2=16, pre=True, dtypes=(F32,)),
    # stride (1, 2, 2) with odd extents: every tile is a large-halo one (MAXP = 28; BM = 128: MAXP = 14)
    _case("3d_down_odd", 1, (3, 7, 9), 32, 64, stride=(2, 2)),
    _case("3d_down_odd_bm128", 1, (3, 7, 9), 32, 128, stride=(2, 2)),
    _case("2d_down", 2, (16, 12), 64, 64, kernel=(1, 3, 3), stride=(2, 2)),
    _case("1d_down", 2, (32,), 32, 32, kernel=(1, 1, 3), stride=(1, 2)),
    # nearest x2 upsample fused into the loader
    _case("3d_up", 2, (4, 4, 4), 32, 32, up=(1, 1)),
    _case("2d_up", 2, (6, 8), 64, 64, kernel=(1, 3, 3), up=(1, 1)),
    _case("1d_up", 2, (16,), 32, 32, kernel=(1, 1, 3), up=(0, 1)),
    # 1x3x3 / 1x1x3 / 1x1x1
    _case("2d_basic", 3, (12, 10), 32, 64, kernel=(1, 3, 3), pre=True, res=True, add=True),
    _case("1d_basic", 2, (40,), 32, 32, kernel=(1, 1, 3), pre=True, res=True),
    _case("3d_1x1", 2, (3, 5, 7), 96, 64, kernel=(1, 1, 1), pre=True),
    _case("1d_1x1", 2, (16,), 64, 192, kernel=(1, 1, 1), pre=True, res=True),
    _case("2d_1x1_concat", 2, (8, 8), 64, 32, kernel=(1, 1, 1), c2=32),
    _case("1x1_stats", 2, (4, 8, 8), 32, 64, kernel=(1, 1, 1), pre=True, stats=True),
    # second output: channel-major y2 (bf16 / fp32 engine dtype), two cout tiles in y2, fp32 head (split == 0), y2 channels-last + res2
    _case("split_y2", 2, (8, 8), 64, 192, kernel=(1, 1, 1), split=128),
    _case("split_two_y2_tiles", 2, (4, 8, 8), 32, 192, split=64, pre=True, w_scale=0.35),
    _case("head_f32", 2, (8, 8), 64, 3, kernel=(1, 3, 3), split=0, y2="cm_f32", pre=True),
    _case("y2_cl_res2", 2, (4, 8, 8), 64, 96, split=64, y2="cl", res=True, res2=True, w_scale=0.35),
    # ResBlock skip folded into the out-conv launch (bf16 16x16x32 variants only), concatenated skip input
    _case("fold_ragged", 1, (5, 9, 11), 64, 64, pre=True, skip=(32, 32), stats=True, dtypes=(BF16,), w_scale=0.26),
    _case("fold_bm128", 1, (4, 8, 8), 128, 128, pre=True, skip=(32, 32), dtypes=(BF16,), w_scale=0.3),
    # k_conv32<bf16>: one tile touching every face; ragged tile range per workgroup; no prologue; odd batch
    _case("c32_one_tile", 1, (4, 8, 8), 32, 32, pre=True, res=True, stats=True, dtypes=(BF16,), w_scale=0.29),
    _case("c32_n3_ragged", 3, (8, 16, 24), 32, 32, pre=True, add=True, stats=True, dtypes=(BF16,), w_scale=0.29),
    _case("c32_plain", 2, (12, 8, 16), 32, 32, res=True, add=True, stats=True, dtypes=(BF16,), w_scale=0.35),
    _case("c32_n5", 5, (16, 16, 16), 32, 32, pre=True, res=True, add=True, stats=True, dtypes=(BF16,), w_scale=0.29),
    # k_gemm1x1<bf16,256x128>: the four GEMM_CASES geometries
    _case("gemm_one_tile_one_kstep", 1, (4, 8, 8), 64, 128, kernel=(1, 1, 1), dtypes=(BF16,)),
    _case("gemm_split_both_orientations", 2, (8, 8, 8), 512, 384, kernel=(1, 1, 1), split=256, dtypes=(BF16,), w_scale=0.35),
    _case("gemm_res_stats_odd", 3, (12, 8, 8), 192, 128, kernel=(1, 1, 1), res=True, stats=True, dtypes=(BF16,), w_scale=0.3),
    _case("gemm_two_y2_tiles", 2, (4, 8, 8), 64, 384, kernel=(1, 1, 1), split=128, dtypes=(BF16,)),
    # k-split with an attached workspace (2-D / 1-D / 1x1x1 launches on small grids); N is raised to the smallest batch that splits
    _case("ksplit_ragged_2d", 1, (7, 9), 192, 128, kernel=(1, 3, 3), c2=64, pre=True, res=True, add=True, ksplit=True, w_scale=0.3),
    _case("ksplit_1d_long_k", 1, (200,), 512, 128, kernel=(1, 1, 3), pre=True, res=True, ksplit=True, w_scale=0.3),
    _case("ksplit_1x1_pre_ragged", 1, (7, 9), 192, 128, kernel=(1, 1, 1), c2=64, pre=True, res=True, ksplit=True, w_scale=0.35),
]
FWD_BY_NAME = {c["name"]: c for c in FWD_CASES}
STATS_Y_CAP = 64          # |y| of the cases with fused statistics: a 256-position tile's sum of squares stays below 2^24


def conv5(x, w, b, stride=(1, 1), up=(0, 0)):
    """conv3d over [N, C, D, H, W] with padding k // 2, stride (1, sh, sw), behind a nearest x2 upsample of the flagged inner axes."""
    if up[0]:
        x = x.repeat_interleave(2, dim=3)
    if up[1]:
        x = x.repeat_interleave(2, dim=4)
    k = w.shape[2:]
    return F.conv3d(x, w, b, stride=(1, stride[0], stride[1]), padding=(k[0] // 2, k[1] // 2, k[2] // 2))


def affine(x, a, b):
    """The affine prologue a * x + b per (sample, channel), applied BEFORE the conv's zero padding."""
    sh = tuple(a.shape) + (1, 1, 1)
    return a.reshape(sh) * x + b.reshape(sh)


def fwd_operands(c, N=None):
    """Integer operands of a forward case, float32 on the CPU."""
    N = c["N"] if N is None else N
    nm, cin = c["name"], c["c1"] + c["c2"]
    o = dict(N=N)
    o["x"] = int_tensor((N, cin) + c["spatial"], nm + "x", 0.75, 2)
    o["w"] = int_tensor((c["cout"], cin) + c["kernel"], nm + "w", c["w_scale"], 1)
    o["b"] = int_tensor((c["cout"],), nm + "b", 2.0, 4)
    if c["pre"]:
        o["pa"] = int_choice((N, cin), nm + "pa", (-1, 1, 2))
        o["pb"] = int_choice((N, cin), nm + "pb", (-1, 0, 1))
    if c["skip"]:
        sc = sum(c["skip"])
        o["sx"] = int_tensor((N, sc) + c["spatial"], nm + "sx", 0.75, 2)
        o["sw"] = int_tensor((c["cout"], sc, 1, 1, 1), nm + "sw", 0.45, 1)
        o["sb"] = int_tensor((c["cout"],), nm + "sb", 2.0, 4)
    osp = fwd_out_spatial(c)
    if c["res"]:
        o["res"] = int_tensor((N, c["split"]) + osp, nm + "r", 4.0, 8)
    if c["res2"]:
        o["res2"] = int_tensor((N, c["cout"] - c["split"]) + osp, nm + "r2", 4.0, 8)
    if c["add"]:
        o["add"] = int_tensor((N, c["cout"]), nm + "add", 2.0, 4)
    return o


def fwd_out_spatial(c):
    D, H, W = c["spatial"]
    k, s, u = c["kernel"], c["stride"], c["up"]
    ho = H * 2 if u[0] else (H + 2 * (k[1] // 2) - k[1]) // s[0] + 1
    wo = W * 2 if u[1] else (W + 2 * (k[2] // 2) - k[2]) // s[1] + 1
    return (D, ho, wo)


def fwd_reference(c, o, dtype=torch.float64, act_fn=None):
    """(activated input, full output [N, cout, Do, Ho, Wo]) evaluated in `dtype` on the CPU.  act_fn: applied to the affine prologue's
    result (the loader's SiLU, see silu_operand)."""
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in o.items()}
    act = affine(t["x"], t["pa"], t["pb"]) if c["pre"] else t["x"]
    if act_fn is not None:
        act = act_fn(act)
    y = conv5(act, t["w"], t["b"], c["stride"], c["up"])
    if c["skip"]:
        y = y + conv5(t["sx"], t["sw"], t["sb"])
    if c["add"]:
        y = y + t["add"].reshape(t["add"].shape + (1, 1, 1))
    if c["res"]:
        y = torch.cat([y[:, :c["split"]] + t["res"], y[:, c["split"]:]], 1)
    if c["res2"]:
        y = torch.cat([y[:, :c["split"]], y[:, c["split"]:] + t["res2"]], 1)
    return act, y


# ----------------------------------------------------------------------------- SiLU in the conv loaders (pre_silu = 1)
# The prologue cases again with the loader's SiLU switched on.  (a, b) from SILU_AB and x in [-2, 2] keep u = a x + b an integer in
# [-2, 6] (the fma is exact; u = 6 is where a sigmoid rounded to bf16 before the product changes the operand).  silu64(u) lies
# hundreds of fp32 ulps from every bf16 rounding tie there (test_exact_cases_host.py
# re-proves the margin against four times the derived silu_f bound), while the loader's expression errs by a few ulps, so the bf16
# operand handed to the MFMA is exactly s = bf16(silu64(u)), on a grid of 2^-10 (the bf16 spacing at silu(-2) = -0.238).  The host
# twin proves sum |w s| (+ bias, residual, additive row, folded skip) stays below 2^24 steps of that grid: every fp32 partial sum is
# exact in any order and the stored output is the reference after ONE rounding to the storage type.  The float32 kernels hand the
# MFMA silu_f(u) itself, known to the silu_f bound: their output is bounded per element (silu_fwd_bound).
SILU_AB = ((1, 0), (1, 1), (-1, 0), (-1, 1), (2, 2))          # (a, b) per (sample, channel); (2, 2) reaches u = 4 and 6
SILU_U = (-2, -1, 0, 1, 2, 3, 4, 6)
SILU_GRID = 2.0 ** -10
SILU_FWD_CASES = [c for c in FWD_CASES if c["pre"] and not c["ksplit"]]
SILU_FORMS = ("exact", "bf16_of_expf", "rounded_twice")


def silu_operand(u, dtype, form="exact"):
    """float64: what the loader hands the MFMA for an integer u: bf16(silu64(u)) in the bf16 kernels, silu64(u) (to the silu_f bound)
    in the float32 ones.  The other forms are what a wrong loader would compute - SiLU through a bf16-rounded exponential, or
    x * sigmoid with the sigmoid rounded to bf16 first (rounded twice) - for the host twin's mutation test."""
    from exact_util import bf16_round
    u = u.double()
    if form == "exact":
        s = u / (1.0 + torch.exp(-u))
    elif form == "bf16_of_expf":
        s = u / (1.0 + bf16_round(torch.exp(-u).float().double()))
    elif form == "rounded_twice":
        s = u * bf16_round(1.0 / (1.0 + torch.exp(-u)))
    else:
        raise ValueError(form)
    return bf16_round(s) if dtype == BF16 else s


def silu_fwd_operands(c):
    o = fwd_operands(c)
    N, cin = o["N"], c["c1"] + c["c2"]
    idx = int_choice((N, cin), c["name"] + "sab", range(len(SILU_AB))).long()
    ab = torch.tensor(SILU_AB, dtype=torch.float32)
    o["pa"], o["pb"] = ab[idx, 0].contiguous(), ab[idx, 1].contiguous()
    return o


def silu_fwd_reference(c, o, dtype, form="exact"):
    """(u, y): the integer prologue values and the fp64 output of the case with SiLU in the loader."""
    u = affine(o["x"].double(), o["pa"].double(), o["pb"].double())
    _, y = fwd_reference(c, o, torch.float64, lambda a: silu_operand(a, dtype, form))
    return u, y


def silu_fwd_magnitude(c, o, dtype):
    """sum |w s| + |bias| + |skip terms| + |add| + |res| per output element (fp64): bounds every partial sum of the launch."""
    oa = {k: (v.abs() if torch.is_tensor(v) and k not in ("pa", "pb", "x") else v) for k, v in o.items()}
    _, m = fwd_reference(c, oa, torch.float64, lambda a: silu_operand(a, dtype).abs())
    return m


def silu_fwd_bound(c, o):
    """float32 kernels: |dy| <= sum |w| * (silu_f bound at u) + n 2^-24 (sum |w s| + ...), n = the number of terms of an output."""
    import embed_cases as EC
    u = affine(o["x"].double(), o["pa"].double(), o["pb"].double())
    _, b, _ = EC.hw_act_bound(u, 1, False)
    z = {k: (torch.zeros_like(v) if k in ("b", "sx", "sb", "res", "res2", "add") else v.abs() if k in ("w", "sw") else v)
         for k, v in o.items() if torch.is_tensor(v)}
    z["N"] = o["N"]
    _, first = fwd_reference(c, z, torch.float64, lambda a: b)
    n = (c["c1"] + c["c2"]) * math.prod(c["kernel"]) + (sum(c["skip"]) if c["skip"] else 0) + 4
    return first + n * 2.0 ** -24 * silu_fwd_magnitude(c, o, F32)


# the tile of a k_conv launch (conv_common.h choose_tile: fewest tiles, then the smallest halo, then the widest W): the fused
# statistics hold one row per tile, in (td, th, tw) order
def choose_tile(kernel, stride, up, Do, Ho, Wo, np_cap):
    best, best_cost = None, 1e300
    TD = 1
    while TD <= 256:
        TH = 1
        while TH * TD <= 256:
            TW = 256 // (TD * TH)
            if not ((up[0] and TH < 2) or (up[1] and TW < 2)):
                ID = TD + kernel[0] - 1
                IH = TH // 2 + 2 if up[0] else (TH - 1) * stride[0] + kernel[1]
                IW = TW // 2 + 2 if up[1] else (TW - 1) * stride[1] + kernel[2]
                NP = ID * IH * IW
                if NP <= np_cap:
                    tiles = -(-Do // TD) * -(-Ho // TH) * -(-Wo // TW)
                    cost = float(tiles) * (NP * 1.5 + 256.0 * kernel[0] * kernel[1] * kernel[2]) - 1e-3 * TW
                    if cost < best_cost:
                        best, best_cost = (TD, TH, TW), cost
            TH *= 2
        TD *= 2
    return best


def tile_ids(c, kind):
    """int64 [Do, Ho, Wo]: the statistics row (tile of a sample) each output position of a stats case belongs to.
    kind: 'k_conv' (3-D tiles from choose_tile, or 256 consecutive positions for 1x1x1), 'gemm' (256 consecutive positions),
    'conv32' (4 x 8 x 8 tiles dealt to wps workgroups in contiguous ranges: conv32.h)."""
    Do, Ho, Wo = fwd_out_spatial(c)
    pos = torch.arange(Do * Ho * Wo).reshape(Do, Ho, Wo)
    if kind == "gemm" or c["kernel"] == (1, 1, 1):
        return pos // 256
    d, h, w = torch.meshgrid(torch.arange(Do), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    if kind == "conv32":
        th, tw = Ho // 8, Wo // 8
        tps = (Do // 4) * th * tw
        t = ((d // 4) * th + (h // 8)) * tw + (w // 8)
        wps = min(tps, 1 if c["N"] >= 256 else (256 + c["N"] - 1) // c["N"])
        owner = torch.zeros(tps, dtype=torch.long)
        for wg in range(wps):
            owner[tps * wg // wps: tps * (wg + 1) // wps] = wg
        return owner[t]
    TD, TH, TW = choose_tile(c["kernel"], c["stride"], c["up"], Do, Ho, Wo, 640)
    return ((d // TD) * -(-Ho // TH) + (h // TH)) * -(-Wo // TW) + (w // TW)


def stats_reference(y, ids, x=None):
    """[N, tiles, 2, C] float64: per tile the channel sums and sums of squares of y [N, C, Do, Ho, Wo]; with x (same shape) the
    second row holds the sums of y * x instead (the product form a data-gradient launch writes through rho_conv_desc.gnb_*)."""
    N, C = y.shape[:2]
    tiles = int(ids.max()) + 1
    out = torch.zeros(N, tiles, 2, C, dtype=torch.float64)
    yf = y.double().reshape(N, C, -1).permute(0, 2, 1)          # [N, S, C]
    xf = yf if x is None else x.double().reshape(N, C, -1).permute(0, 2, 1)
    idx = ids.reshape(-1)
    for n in range(N):
        out[n, :, 0].index_add_(0, idx, yf[n])
        out[n, :, 1].index_add_(0, idx, yf[n] * xf[n])
    return out


# ----------------------------------------------------------------------------- sub-pixel phases / parity splits
# (kernel, (N, D, H, W), up, cin, cout): Upsample + conv as one 2-tap launch per output parity (3x2x2, 1x2x2, 1x1x2)
PHASE_CASES = [((3, 3, 3), (2, 3, 5, 7), (1, 1), 32, 32), ((1, 3, 3), (3, 1, 9, 11), (1, 1), 32, 64), ((1, 1, 3), (2, 1, 1, 100), (0, 1), 32, 32)]
# ((N, D, H, W), cin, cout): stride (1, 2, 2) 3x3x3 conv as four stride-1 launches (3x1x1, 3x1x2, 3x2x1, 3x2x2) accumulated in place
S2_CASES = [((2, 3, 6, 10), 32, 64)]
S2_FWD_SEL = {0: (1,), 1: (0, 2)}          # input parity -> taps of the 3-tap axis that read it
S2_BWD_SEL = {0: (1,), 1: (2, 0)}


def phase_operands(kernel, shape, cin, cout, tag="ph"):
    N, D, H, W = shape
    return dict(x=int_tensor((N, cin, D, H, W), tag + "x", 0.75, 2), w=int_tensor((cout, cin) + tuple(kernel), tag + "w", 0.45, 1),
                b=int_tensor((cout,), tag + "b", 2.0, 4))


def s2_partial_weights(w):
    """The four tap selections of the parity split, as full 3x3x3 weights with the other taps zeroed, in launch order."""
    out = []
    for a in (0, 1):
        for c in (0, 1):
            m = torch.zeros_like(w)
            for i in S2_FWD_SEL[a]:
                for j in S2_FWD_SEL[c]:
                    m[:, :, :, i, j] = w[:, :, :, i, j]
            out.append(m)
    return out


# ----------------------------------------------------------------------------- backward
def _bcase(name, N, spatial, c1, cout, kernel=(3, 3, 3), c2=0, stride=(1, 1), up=(0, 0), pre=False, dtypes=BOTH, w_scale=0.45):
    sp = (1,) * (3 - len(spatial)) + tuple(spatial)
    return dict(name=name, N=N, spatial=sp, c1=c1, c2=c2, cout=cout, kernel=tuple(kernel), stride=tuple(stride), up=tuple(up), pre=pre,
                dtypes=tuple(dtypes), w_scale=w_scale)


BWD_CASES = [
    _bcase("3d_basic", 2, (4, 8, 8), 32, 64),
    _bcase("3d_ragged", 1, (5, 6, 7), 64, 32),
    _bcase("3d_concat", 2, (4, 8, 8), 64, 64, c2=32),
    _bcase("3d_multi_ragged", 2, (9, 20, 12), 32, 64),
    _bcase("3d_multi_whole", 1, (12, 24, 16), 64, 64),          # whole 4 x 8 x 8 tiles: k_wgrad<bf16,...,GEO=1>
    _bcase("2d_multi_ragged", 2, (40, 36), 64, 64, kernel=(1, 3, 3)),
    _bcase("3d_pre", 2, (4, 6, 8), 64, 32, pre=True),
    _bcase("3d_down", 2, (4, 8, 8), 32, 32, stride=(2, 2)),
    _bcase("3d_down_odd", 1, (3, 7, 9), 32, 64, stride=(2, 2)),
    _bcase("2d_down", 2, (16, 12), 64, 64, kernel=(1, 3, 3), stride=(2, 2)),
    _bcase("3d_up", 2, (4, 4, 4), 32, 32, up=(1, 1)),
    _bcase("2d_basic", 3, (12, 10), 32, 64, kernel=(1, 3, 3)),
    _bcase("1d_basic", 2, (40,), 32, 32, kernel=(1, 1, 3)),
    _bcase("3d_1x1", 2, (3, 5, 7), 96, 64, kernel=(1, 1, 1)),                          # bf16: k_wgrad1 with 210 positions, cin 96
    _bcase("1x1_straddle_odd", 3, (9, 13), 48, 64, kernel=(1, 1, 1), c2=32, dtypes=(F32,)),
    _bcase("1x1_single_chunk", 3, (9, 13), 16, 64, kernel=(1, 1, 1), dtypes=(F32,)),
    _bcase("1x1_straddle_odd_pre", 3, (9, 13), 48, 64, kernel=(1, 1, 1), c2=32, pre=True, dtypes=(F32,)),
    _bcase("3d_cout48", 2, (4, 6, 8), 32, 48),                                          # coutp = 64: dbias has a padded tail (weight gradient only)
    _bcase("1x1_wgrad1_wide", 3, (9, 13), 160, 96, kernel=(1, 1, 1), c2=32, dtypes=(BF16,)),   # 351 positions, cin 192: two cin blocks
]
BWD_BY_NAME = {c["name"]: c for c in BWD_CASES}


def bwd_operands(c):
    nm, cin, N = "b_" + c["name"], c["c1"] + c["c2"], c["N"]
    o = dict(N=N)
    o["x"] = int_tensor((N, cin) + c["spatial"], nm + "x", 0.75, 2)
    o["w"] = int_tensor((c["cout"], cin) + c["kernel"], nm + "w", c["w_scale"], 1)
    if c["pre"]:
        o["pa"] = int_choice((N, cin), nm + "pa", (-1, 1, 2))
        o["pb"] = int_choice((N, cin), nm + "pb", (-1, 0, 1))
    o["dy"] = int_tensor((N, c["cout"]) + fwd_out_spatial(c), nm + "dy", 0.45, 1)          # |dy| <= 1, about 28 % non-zero
    if c["c2"] and not c["pre"]:
        o["base"] = int_tensor((N, c["c2"]) + c["spatial"], nm + "base", 4.0, 8)            # the gradient the second source accumulates onto
    return o


def bwd_reference(c, o, dtype=torch.float64, act_fn=None):
    """dict(act, dx = gradient w.r.t. the activated input, dw, db) by autograd in `dtype` on the CPU.  act_fn: applied to the affine
    prologue's result (the loader's SiLU, see silu_operand)."""
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in o.items()}
    act = affine(t["x"], t["pa"], t["pb"]) if c["pre"] else t["x"]
    if act_fn is not None:
        act = act_fn(act)
    act = act.clone().requires_grad_(True)
    w = t["w"].clone().requires_grad_(True)
    b = torch.zeros(c["cout"], dtype=dtype, requires_grad=True)
    conv5(act, w, b, c["stride"], c["up"]).backward(t["dy"])
    return dict(act=act.detach(), dx=act.grad, dw=w.grad, db=b.grad)


# ----------------------------------------------------------------------------- attention as a permutation
# (B, T, heads, ch): the shapes of test_attention / test_attention_backward; T = 100 and T = 300 end in a partial key tile
ATTN_CASES = [(2, 64, 4, 16), (2, 256, 2, 32), (1, 100, 1, 32), (2, 4, 1, 256), (1, 300, 4, 64), (1, 192, 2, 128)]
ATTN_MIN_GAP = 160.0      # base-2 units: exp2(-160) < 2^-149, every unmatched probability is exactly 0 in fp32


def attn_codes(T, ch):
    """[T, ch] of +-1: row s = the binary digits of s, extended by a fixed pattern - distinct for distinct s (T <= 2^ch)."""
    nb = max(1, (T - 1).bit_length())
    assert nb <= ch
    s = torch.arange(T)
    bits = torch.stack([(s >> i) & 1 for i in range(nb)], 1)
    ext = torch.tensor([(i * i + i // 3) & 1 for i in range(ch - nb)], dtype=torch.long).expand(T, ch - nb)
    return (1 - 2 * torch.cat([bits, ext], 1)).float()


def attn_perm(T, b, h, heads):
    """pi(t) = (a t + o) mod T with a coprime to T and o different for every (batch, head)."""
    a = next(v for v in (7, 11, 13, 17, 19, 23, 1) if math.gcd(v, T) == 1)
    return (a * torch.arange(T) + 3 + 5 * (b * heads + h)) % T


def attn_operands(B, T, heads, ch):
    """q, k, v, dO as [B, heads, ch, T] float32 (exact in bf16), pi [B, heads, T], and the q amplitude."""
    amp = 512.0
    if 2 * amp / math.sqrt(ch) * math.log2(math.e) < ATTN_MIN_GAP:
        amp = 1024.0
    codes = attn_codes(T, ch)                                             # [T, ch]
    pi = torch.stack([torch.stack([attn_perm(T, b, h, heads) for h in range(heads)]) for b in range(B)])      # [B, heads, T]
    k = codes.t().expand(B, heads, ch, T).contiguous()
    q = amp * codes[pi].permute(0, 1, 3, 2).contiguous()                  # q[b, h, :, t] = amp * c_{pi(t)}
    tag = f"at{B}_{T}_{heads}_{ch}"
    v = int_tensor((B, heads, ch, T), tag + "v", 60.0, 127)
    do = int_tensor((B, heads, ch, T), tag + "do", 0.9, 2)
    return dict(q=q, k=k, v=v, do=do, pi=pi, amp=amp)


def attn_reference(o, ch):
    """fp64: scaled base-2 logits [B, heads, T(query), T(key)], the matched logit m [B, heads, T] and the gap to the runner-up."""
    logits = torch.einsum("bhct,bhcs->bhts", o["q"].double(), o["k"].double()) * (math.log2(math.e) / math.sqrt(ch))
    m = torch.gather(logits, 3, o["pi"].unsqueeze(-1)).squeeze(-1)
    rest = logits.scatter(3, o["pi"].unsqueeze(-1), float("-inf"))
    gap = m - rest.max(-1).values if logits.shape[-1] > 1 else torch.full_like(m, float("inf"))
    return dict(logits=logits, m=m, gap=gap)


# ----------------------------------------------------------------------------- GroupNorm passes (groupnorm.hip)
# 32 groups over the channel concat of x1 (c1 channels) and x2 (c2), biased variance, eps = 1e-5.  Every tensor is channels-last
# [N, S, C]; the references are plain reductions over (positions, channels of a group) and know nothing of position blocks, octets
# or lanes.
GN_EPS = 1e-5


def _gcase(name, N, c1, c2, S, reach):
    return dict(name=name, N=N, c1=c1, c2=c2, S=S, C=c1 + c2, cpg=(c1 + c2) // 32, reach=reach, dtypes=BOTH)


GN_CASES = [
    _gcase("one_pos", 1, 32, 0, 1, "one position, one live lane row"),
    _gcase("cpg3_straddle", 3, 40, 56, 7, "cpg = 3, OCT = 12 does not divide 256, a group spans both sources, S < ppi"),
    _gcase("nblk2_tails", 2, 64, 0, 257, "nblk = 2, odd tails of the 4x and 2x unrolled loops"),
    _gcase("oct48", 2, 256, 128, 1600, "OCT = 48, ppi = 5, nblk = 7"),
    # (N = 1 means gpb = 1 in k_gn_finalize2: CB = cpg there; its KP = 1 / CB = 256 and CB = 132 need N >= 32: the last two entries)
    _gcase("c2048", 1, 2048, 0, 9, "ppi = 1 in the position passes; KP = 1, CB = 256 in k_gn_bwd_finalize (k_gn_finalize2: CB = 64, KP = 4)"),
    _gcase("c2048_split", 1, 1024, 1024, 5, "as c2048 with the concat boundary at a workgroup edge of k_gn_bwd_finalize"),
    _gcase("c1056_idle", 1, 1056, 0, 6, "OCT = 132: threads 132 - 255 idle in the position passes, cpg = 33; CB = 132, KP = 1 in "
           "k_gn_bwd_finalize (k_gn_finalize2: CB = 33, KP = 7)"),
    _gcase("gpb4", 32, 32, 0, 64, "gpb = 4 in k_gn_finalize2 (CB = 4, KP = 64)"),
    _gcase("gpb4_straddle", 33, 40, 56, 9, "gpb = 4 with a group that spans both sources (CB = 12, KP = 21)"),
    _gcase("gpb4_c2048", 32, 1000, 1048, 2, "gpb = 4 at C = 2048: KP = 1, CB = 256 in k_gn_finalize2, the concat boundary inside a workgroup"),
    _gcase("gpb4_c1056", 32, 1056, 0, 2, "gpb = 4 at C = 1056: CB = 132, KP = 1 in k_gn_finalize2, threads 132 - 255 idle"),
    _gcase("nblk_cap", 1, 32, 0, 65537, "the nblk = 256 cap of rho_gn_nblk, 257 positions per block"),
]
GN_BY_NAME = {c["name"]: c for c in GN_CASES}


def gn_nblk(S):
    """rho_gn_nblk: 256-position blocks, at most 256 of them."""
    return max(1, min(256, -(-S // 256)))


def gn_reduce_stream(S, C, pos):
    """Which accumulation of k_gn_bwd_reduce takes position `pos`: lane pl = q % ppi of block pos / per walks q = pl, pl + ppi, ...
    (q relative to the block) in pairs - "gq" the first, "gr" the second of a pair - and a last unpaired one in the "tail" loop."""
    ppi = 256 // (C // 8)
    per = -(-S // gn_nblk(S))
    blk = pos // per
    length = min(S, (blk + 1) * per) - blk * per
    q = pos - blk * per
    pl, k = q % ppi, q // ppi
    n = -(-(length - pl) // ppi)                       # positions of this lane
    if n % 2 == 1 and k == n - 1:
        return "tail"
    return "gq" if k % 2 == 0 else "gr"


def gn_reduce_stream_positions(S, C):
    """{stream: first position that falls into it} for the streams a shape reaches."""
    out = {}
    for pos in range(S):
        out.setdefault(gn_reduce_stream(S, C, pos), pos)
    return out


def gn_int(shape, tag, lo, hi):
    """Deterministic float32 tensor of integers uniform on [lo, hi]."""
    return det_uniform(tuple(shape), tag, 0.0, float(hi - lo + 1)).floor().clamp_(0, hi - lo) + lo


def per_channel(v, cpg):
    """[N, 32] per group -> [N, 1, C] per channel."""
    return v.repeat_interleave(cpg, 1).unsqueeze(1)


def gn_stats_operands(c):
    """x = integers in +-4 plus an integer offset per (sample, group) in +-3 (so the means are not 0); real-valued gamma, beta
    and FiLM rows [N, 2C] = (scale | shift)."""
    nm, N, S, C = "gn_" + c["name"], c["N"], c["S"], c["C"]
    x = gn_int((N, S, C), nm + "x", -4, 4) + per_channel(gn_int((N, 32), nm + "off", -3, 3), c["cpg"])
    return dict(x=x, gamma=1 + 0.2 * det_uniform((C,), nm + "ga"), beta=0.1 * det_uniform((C,), nm + "be"),
                film=0.3 * det_normal((N, 2 * C), nm + "film"))


def gn_stats_reference(x, dtype=torch.float64):
    """dict(sum, sumsq [N, C]; mean, rstd [N, 32]) of x [N, S, C]: two-pass biased variance in `dtype`."""
    N, S, C = x.shape
    xd = x.to(dtype)
    xg = xd.reshape(N, S, 32, C // 32)
    mean = xg.mean((1, 3))
    var = ((xg - mean.reshape(N, 1, 32, 1)) ** 2).mean((1, 3))
    return dict(sum=xd.sum(1), sumsq=(xd * xd).sum(1), mean=mean, rstd=1.0 / torch.sqrt(var + GN_EPS))


def gn_fold_reference(mean, rstd, gamma, beta, scale=None, shift=None):
    """The folded affine of rho_hip.h in fp64: a = rstd gamma (1 + scale), b = (beta - mean rstd gamma)(1 + scale) + shift, each
    [N, C], and the sum of the magnitudes of b's terms (the scale of its rounding errors: the terms may cancel)."""
    C = gamma.numel()
    cpg = C // 32
    mu, rs = per_channel(mean.double(), cpg)[:, 0], per_channel(rstd.double(), cpg)[:, 0]
    ga, be = gamma.double().unsqueeze(0), beta.double().unsqueeze(0)
    sc = 1.0 if scale is None else 1.0 + scale.double()
    sh = 0.0 if shift is None else shift.double()
    a = rs * ga * sc
    b = (be - mu * rs * ga) * sc + sh
    mag = (be.abs() + (mu * rs * ga).abs()) * abs(sc) + abs(sh)
    return a, b, mag + torch.zeros_like(b)


def gn_apply_operands(c, tag="ap"):
    """Integer operands of the apply passes: x in +-4, folded affine a in +-2, b in +-3 per (sample, channel)."""
    nm, N, S, C = f"gn{tag}_" + c["name"], c["N"], c["S"], c["C"]
    return dict(x=gn_int((N, S, C), nm + "x", -4, 4), a=gn_int((N, C), nm + "a", -2, 2), b=gn_int((N, C), nm + "b", -3, 3))


def gn_apply_reference(x, a, b, dtype=torch.float64):
    """a x + b per (sample, channel) over [N, S, C] (act code 0)."""
    return a.to(dtype).unsqueeze(1) * x.to(dtype) + b.to(dtype).unsqueeze(1)


def gn_bwd_operands(c):
    """Backward operands: g in +-2, x in +-4, SUPPLIED statistics (integer mean in +-3, rstd in {0.5, 1, 2}), integer gamma / beta in
    +-2, FiLM rows [N, 2C] with an integer scale in -2 .. 2 (so 1 + scale may be 0 or negative), the folded affine (a, b) (read, but
    without effect at act code 0), integer gradients that dgamma / dbeta accumulate onto, and the coefficients / addends of the
    apply pass: cA in +-2 [N, C], cP in +-3, cQ in +-1 [N, 32], the running gradients dx and the residual addend in +-8."""
    nm, N, S, C = "gnb_" + c["name"], c["N"], c["S"], c["C"]
    o = gn_apply_operands(c, "bw")
    o.update(g=gn_int((N, S, C), nm + "g", -2, 2), mean=gn_int((N, 32), nm + "mean", -3, 3),
             rstd=int_choice((N, 32), nm + "rstd", (0.5, 1.0, 2.0)), gamma=gn_int((C,), nm + "ga", -2, 2),
             beta=gn_int((C,), nm + "be", -2, 2),
             film=torch.cat([gn_int((N, C), nm + "sc", -2, 2), gn_int((N, C), nm + "sh", -3, 3)], 1),
             dgamma0=gn_int((C,), nm + "dg0", -16, 16), dbeta0=gn_int((C,), nm + "db0", -16, 16),
             cA=gn_int((N, C), nm + "cA", -2, 2), cP=gn_int((N, 32), nm + "cP", -3, 3), cQ=gn_int((N, 32), nm + "cQ", -1, 1),
             dx0=gn_int((N, S, C), nm + "dx0", -8, 8), add1=gn_int((N, S, c["c1"]), nm + "add1", -8, 8))
    o["stats"] = torch.stack([o["mean"], o["rstd"]], -1).contiguous()
    return o


def gn_bwd_coeffs_reference(R1, R2, mean, rstd, gamma, beta, scale, S, dtype=torch.float64):
    """What rho_gn_bwd_finalize derives from the per-(sample, channel) sums R1, R2 [N, C] (formulas: gn_bwd_reference)."""
    N, C = R1.shape
    cpg = C // 32
    R1, R2, mean, rstd, gamma, beta = (t.to(dtype) for t in (R1, R2, mean, rstd, gamma, beta))
    sc = torch.ones(N, C, dtype=dtype) if scale is None else 1.0 + scale.to(dtype)
    gp = gamma.unsqueeze(0) * sc
    M = float(cpg * S)
    s1, s2 = (gp * R1).reshape(N, 32, cpg).sum(2), (gp * R2).reshape(N, 32, cpg).sum(2)
    return dict(R1=R1, R2=R2, cA=per_channel(rstd, cpg)[:, 0] * gp, cP=(-rstd * s1 + rstd * rstd * s2 * mean) / M,
                cQ=-rstd * rstd * s2 / M, dgamma=(R2 * sc).sum(0), dbeta=(R1 * sc).sum(0), dgamma_n=R2 * sc, dbeta_n=R1 * sc,
                dscale=gamma.unsqueeze(0) * R2 + beta.unsqueeze(0) * R1, dshift=R1, M=M)


def gn_bwd_reference(gq, x, mean, rstd, gamma, beta, scale=None, dtype=torch.float64):
    """The formulas above k_gn_bwd_reduce, for gq = g act'(u) [N, S, C] (act code 0: g itself, times the dropout multiplier):
        xhat = (x - mean) rstd, gamma' = gamma (1 + scale), R1 = sum_pos gq, R2 = sum_pos gq xhat, M = cpg S
        dx = rstd (gamma' gq - mean_grp(gamma' gq) - xhat mean_grp(gamma' gq xhat)) = cA gq + cP + cQ x  with
        cA = rstd gamma',  cQ = -rstd^2 sum_grp(gamma' R2) / M,  cP = (-rstd sum_grp(gamma' R1) + rstd^2 mean sum_grp(gamma' R2)) / M
        dgamma = sum_n R2 (1 + scale), dbeta = sum_n R1 (1 + scale), dscale = gamma R2 + beta R1, dshift = R1.
    absR2 = sum_pos |gq xhat| bounds every partial sum of R2."""
    N, S, C = x.shape
    cpg = C // 32
    gq, x = gq.to(dtype), x.to(dtype)
    xhat = (x - per_channel(mean.to(dtype), cpg)) * per_channel(rstd.to(dtype), cpg)
    r = gn_bwd_coeffs_reference(gq.sum(1), (gq * xhat).sum(1), mean, rstd, gamma, beta, scale, S, dtype)
    r["absR2"] = (gq * xhat).abs().sum(1)
    return r


def gn_bwd_apply_reference(gq, x, cA, cP, cQ, dtype=torch.float64):
    """cA gq + cP + cQ x over [N, S, C] (cA per channel, cP / cQ per group)."""
    cpg = x.shape[2] // 32
    return (cA.to(dtype).unsqueeze(1) * gq.to(dtype) + per_channel(cP.to(dtype), cpg)
            + per_channel(cQ.to(dtype), cpg) * x.to(dtype))


def is_pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


# (N, C, blocks): rho_gn_bwd_finalize fed synthetic per-tile sums (fmt 1) against the same sums as reduce partials (fmt 0)
GN_FIN1_CASES = [(3, 96, 1), (3, 96, 1025), (33, 96, 3), (2, 1056, 3), (1, 2048, 3), (2, 64, 2)]
# (N, c1, c2, blocks of source 1, blocks of source 2): rho_gn_finalize2 on synthetic partials.  k_gn_finalize2 gives a workgroup
# CB = gpb * cpg channels and KP = 256 / CB lanes per channel, gpb = 4 from N = 32 on: 40 + 56 channels run CB = 3, KP = 85 (N = 3) and
# CB = 12, KP = 21 (N = 32); 1000 + 1048 and 1024 + 1024 at N = 32 run KP = 1, CB = 256 (the concat boundary inside a workgroup / at
# a workgroup edge); 520 + 536 at N = 32 runs CB = 132, KP = 1 with threads 132 - 255 idle; 1024 + 1024 at N = 3 runs CB = 64, KP = 4
GN_FIN2_CASES = ([(N, 40, 56, b1, b2) for N in (3, 32) for b1, b2 in ((1, 3), (3, 1025), (1025, 1))]
                 + [(32, 1000, 1048, 3, 1), (32, 1024, 1024, 1, 3), (32, 520, 536, 3, 1), (3, 1024, 1024, 3, 1)])


def gn_fin2_operands(N, c1, c2, nb1, nb2):
    """Integer per-block channel sums (+-8) and sums of squares (64 .. 127) of two sources (c1, c2 channels) and of one source of
    c1 + c2 channels with nb1 blocks, as [N, blocks, C]; S positions per sample (only a divisor to the kernel); real gamma / beta /
    FiLM rows."""
    nm, C = f"gnf2_{N}_{c1}_{c2}_{nb1}_{nb2}", c1 + c2
    o = dict(S=8 * max(nb1, nb2), C=C)
    for key, nb, cc in (("1", nb1, c1), ("2", nb2, c2), ("0", nb1, C)):
        o["s" + key] = gn_int((N, nb, cc), nm + "s" + key, -8, 8)
        o["q" + key] = gn_int((N, nb, cc), nm + "q" + key, 64, 127)
    o.update(gamma=1 + 0.2 * det_uniform((C,), nm + "ga"), beta=0.1 * det_uniform((C,), nm + "be"),
             film=0.3 * det_normal((N, 2 * C), nm + "film"))
    return o


def gn_fin1_operands(N, C, nb):
    """Integer per-tile sums dz (+-16) and dz * x (+-64) as [N, tiles, C], the statistics / parameters of gn_bwd_operands."""
    nm = f"gnf1_{N}_{C}_{nb}"
    g = gn_bwd_operands(dict(name=nm, N=N, S=1, C=C, c1=C, cpg=C // 32))
    o = {k: g[k] for k in ("mean", "rstd", "stats", "gamma", "beta", "film", "dgamma0", "dbeta0")}
    o.update(dz=gn_int((N, nb, C), nm + "dz", -16, 16), dzx=gn_int((N, nb, C), nm + "dzx", -64, 64), S=256 * nb)
    return o


def gn_moments_reference(sums, sumsq, S):
    """mean, rstd [N, 32] in fp64 from exact integer channel sums / sums of squares [N, C] (one-pass form, exact operands)."""
    N, C = sums.shape
    cnt = float((C // 32) * S)
    mean = sums.double().reshape(N, 32, -1).sum(2) / cnt
    var = (sumsq.double().reshape(N, 32, -1).sum(2) / cnt - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + GN_EPS)


def partials_fmt0(s, q):
    """[N, blocks, C] sums and second sums -> rho_gn_partial's layout [N, blocks, C / 8, 16] (8 sums, then 8 second sums)."""
    N, nb, C = s.shape
    return torch.cat([s.reshape(N, nb, C // 8, 8), q.reshape(N, nb, C // 8, 8)], 3).contiguous()


def partials_fmt1(s, q):
    """... -> the conv epilogue's layout [N, tiles, 2, C]."""
    return torch.stack([s, q], 2).contiguous()


# ----------------------------------------------------------------------------- GroupNorm backward inside data-gradient launches
# rho_conv_desc.gnb_*: a 3x3x3 data gradient (the output = d act(a x0 + b) over the concat of two sources, gnb_c1 < split) that
# also writes per tile sum dz and sum dz * x0; act code 0, so dz is the stored output.
GNB_CASES = [
    _bcase("gnb_bm64", 2, (4, 8, 8), 32, 32, c2=32),
    _bcase("gnb_bm128", 1, (4, 8, 8), 64, 32, c2=64),
    _bcase("gnb_ragged", 1, (5, 6, 7), 32, 32, c2=32),
]


def gnb_operands(c):
    """bwd_operands of the launch plus the norm's forward input x0 [N, C, D, H, W] in +-4 and the GroupNorm-backward operands
    (gn_bwd_operands' statistics, parameters and FiLM rows) for C = c1 + c2 channels."""
    o = bwd_operands(c)
    C = c["c1"] + c["c2"]
    S = math.prod(c["spatial"])
    o["x0"] = gn_int((c["N"], C) + c["spatial"], "gnbx0_" + c["name"], -4, 4)
    g = gn_bwd_operands(dict(name="conv_" + c["name"], N=c["N"], S=1, C=C, c1=c["c1"], cpg=C // 32))
    for k in ("a", "b", "mean", "rstd", "stats", "gamma", "beta", "film"):
        o[k] = g[k]
    o["S"] = S
    return o


def gnb_silu_operands(c):
    """gnb_operands with integer folded-affine rows a in {-2, -1, 1, 2}, b in -2 .. 2: u = a x0 + b is an integer in [-10, 10]."""
    o = gnb_operands(c)
    C = c["c1"] + c["c2"]
    o["a"] = int_choice((c["N"], C), "gnbsa_" + c["name"], (-2.0, -1.0, 1.0, 2.0))
    o["b"] = gn_int((c["N"], C), "gnbsb_" + c["name"], -2, 2)
    return o


def gnb_silu_reference(c, o, ids):
    """gnb_silu = 1 on a data-gradient launch: the stored dX stays the integer conv result z; the per-tile rows hold sum dz and
    sum dz x0 with dz = z * dsilu(u).  Returns (z, rows [N, tiles, 2, C], bound on the rows), fp64.  Bound: each dz = fl(z * dsilu_f(u))
    is within |z| (dsilu_f bound at u) + 2^-24 |z| Mag(u) (embed_cases.hw_act_bound; the product rounds once); a row adds the n
    terms of its tile in some order, every addition rounding at most once against a partial sum bounded by the magnitude sum:
    n 2^-24 sum |z| Mag (times |x0| in the second row, whose fma adds dz * x0 unrounded)."""
    import embed_cases as EC
    z = bwd_reference(c, o)["dx"]
    u = affine(o["x0"].double(), o["a"].double(), o["b"].double())
    d, bound, mag = EC.hw_act_bound(u, 1, True)
    n = int(torch.bincount(ids.reshape(-1)).max())
    term = z.abs() * bound + 2.0 ** -24 * z.abs() * mag
    rows = stats_reference(z * d, ids, o["x0"])
    rb = stats_reference(term, ids, o["x0"].abs()) + n * 2.0 ** -24 * stats_reference(z.abs() * mag, ids, o["x0"].abs())
    return z, rows, rb


def to_nsc(t):
    """[N, C, D, H, W] -> [N, S, C]."""
    return t.reshape(t.shape[0], t.shape[1], -1).permute(0, 2, 1)


# rho_conv_desc.gna_*: the 1x1x1 skip convolution's data gradient (dy of cy channels -> both concat regions, y2 channels-last) plus
# cA g + cQ x0 + cP in its epilogue.  (name, dtype, cy, c1, c2, BM, (N, D, H, W)): the geometries of GNA_CASES in
# test_gpu_bench_shapes.py
GNA_CASES = [("gna_bf16_bm32", BF16, 64, 64, 32, 32, (2, 4, 8, 8)), ("gna_bf16_bm64", BF16, 64, 128, 64, 64, (2, 8, 8, 8)),
             ("gna_bf16_bm128", BF16, 128, 256, 128, 128, (3, 4, 8, 8)), ("gna_f32_bm32", F32, 32, 64, 32, 32, (2, 1, 16, 16)),
             ("gna_f32_bm64", F32, 32, 64, 64, 64, (2, 1, 16, 16)), ("gna_f32_bm128", F32, 64, 128, 128, 128, (2, 1, 16, 16))]


def gna_operands(case):
    name, _, cy, c1, c2, _, (N, D, H, W) = case
    C = c1 + c2
    return dict(dy=int_tensor((N, D, H, W, cy), name + "dy", 0.45, 1), w=int_tensor((cy, C, 1, 1, 1), name + "w", 0.45, 1),
                g=gn_int((N, D, H, W, C), name + "g", -2, 2), x0=gn_int((N, D, H, W, C), name + "x0", -4, 4),
                a=gn_int((N, C), name + "a", -2, 2), b=gn_int((N, C), name + "b", -3, 3), cA=gn_int((N, C), name + "cA", -2, 2),
                cP=gn_int((N, 32), name + "cP", -3, 3), cQ=gn_int((N, 32), name + "cQ", -1, 1))


def gna_reference(o, dtype=torch.float64):
    """conv + cA g + cQ x0 + cP, channels-last [N, D, H, W, C]."""
    N, D, H, W, C = o["g"].shape
    conv = torch.einsum("ndhwk,kc->ndhwc", o["dy"].to(dtype), o["w"].to(dtype).reshape(-1, C))
    term = gn_bwd_apply_reference(o["g"].reshape(N, -1, C), o["x0"].reshape(N, -1, C), o["cA"], o["cP"], o["cQ"], dtype)
    return conv + term.reshape(N, D, H, W, C)


def gna_silu_operands(case):
    """gna_operands with gnb_silu = 1 in mind: integer folded-affine rows a in {-2, -1, 1, 2}, b in -2 .. 2 (u = a x0 + b an integer in
    [-10, 10]), cA = 1, cP = cQ = 0 and g in {0, +-1/4, +-1/2}, so that the stored output is conv + g * dsilu(u) element for element."""
    name, _, cy, c1, c2, _, (N, D, H, W) = case
    C = c1 + c2
    o = gna_operands(case)
    o["a"] = int_choice((N, C), name + "sa", (-2.0, -1.0, 1.0, 2.0))
    o["b"] = gn_int((N, C), name + "sb", -2, 2)
    o["cA"], o["cP"], o["cQ"] = torch.ones(N, C), torch.zeros(N, 32), torch.zeros(N, 32)
    o["g"] = o["g"] * 0.25            # |g dsilu(u)| < 0.56: the term never cancels a nonzero integer conv result down to near zero
    return o


def gna_silu_reference(o):
    """(u, conv, want, float32 bound) channels-last, fp64.  The GNA epilogue computes gq = g * dsilu_f(u) (g a power of two or 0: an exact
    scaling, so gq carries |g| times the derived dsilu_f bound of embed_cases.hw_act_bound), fma(1, gq, fma(0, x0, 0)) = gq, and adds
    it to the exact integer accumulator: one rounding of the sum, 2^-24 (|conv| + |g| Mag(u))."""
    import embed_cases as EC
    N, D, H, W, C = o["g"].shape
    conv = torch.einsum("ndhwk,kc->ndhwc", o["dy"].double(), o["w"].double().reshape(-1, C))
    u = o["a"].double().reshape(N, 1, 1, 1, C) * o["x0"].double() + o["b"].double().reshape(N, 1, 1, 1, C)
    d, bound, mag = EC.hw_act_bound(u, 1, True)
    g = o["g"].double()
    return u, conv, conv + g * d, g.abs() * bound + 2.0 ** -24 * (conv.abs() + g.abs() * mag)


# ----------------------------------------------------------------------------- k_wgrad with the prologue and pre_silu = 1
# The prologue cases of BWD_CASES with the (a, b) rows of SILU_AB: dW = sum dY s with dY in +-1 and s = bf16(silu64(u)) is exact on
# the 2^-10 grid in the bf16 kernels (bit-equal after rho_wgrad_finalize); the float32 kernels are bounded per element by
# sum |dY| (silu_f bound at u) + n 2^-24 sum |dY s|, n = the positions an element sums over.
SILU_BWD_CASES = [c for c in BWD_CASES if c["pre"]]


def silu_bwd_operands(c):
    o = bwd_operands(c)
    N, cin = o["N"], c["c1"] + c["c2"]
    idx = int_choice((N, cin), "b_" + c["name"] + "sab", range(len(SILU_AB))).long()
    ab = torch.tensor(SILU_AB, dtype=torch.float32)
    o["pa"], o["pb"] = ab[idx, 0].contiguous(), ab[idx, 1].contiguous()
    return o


def silu_wgrad_reference(c, o, dtype, form="exact"):
    """(dw, magnitude sum |dY s|, float32 bound) in fp64."""
    import embed_cases as EC
    dw = bwd_reference(c, o, torch.float64, lambda a: silu_operand(a, dtype, form))["dw"]
    oa = dict(o, dy=o["dy"].abs())
    mag = bwd_reference(c, oa, torch.float64, lambda a: silu_operand(a, dtype).abs())["dw"]
    first = bwd_reference(c, oa, torch.float64, lambda a: EC.hw_act_bound(a, 1, False)[1])["dw"]
    n = o["N"] * math.prod(fwd_out_spatial(c))
    return dw, mag, first + n * 2.0 ** -24 * mag
