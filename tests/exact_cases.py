"""Case tables and CPU references of the integer-operand tests: imported by test_exact_cases_host.py (which proves, without a GPU,
that every reference stays inside the representability caps and that fp32 == fp64 on the CPU) and by the -m gpu modules
test_gpu_exact_conv.py / test_gpu_exact_backward.py / test_gpu_exact_attention.py.

Every tensor is [N, C, D, H, W] on the CPU here (1-D / 2-D layers carry leading spatial axes of 1, as the kernels see them);
geometries are the smallest ones of the tolerance tests' tables (CONV_CASES, WIDE_CONV, PHASE_CASES, S2_CASES, GEMM_CASES, the conv32
edge geometries, the k-split CASES, BWD_CASES)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

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


def fwd_reference(c, o, dtype=torch.float64):
    """(activated input, full output [N, cout, Do, Ho, Wo]) evaluated in `dtype` on the CPU."""
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in o.items()}
    act = affine(t["x"], t["pa"], t["pb"]) if c["pre"] else t["x"]
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


def stats_reference(y, ids):
    """[N, tiles, 2, C] float64: per tile the channel sums and sums of squares of y [N, C, Do, Ho, Wo]."""
    N, C = y.shape[:2]
    tiles = int(ids.max()) + 1
    out = torch.zeros(N, tiles, 2, C, dtype=torch.float64)
    yf = y.double().reshape(N, C, -1).permute(0, 2, 1)          # [N, S, C]
    idx = ids.reshape(-1)
    for n in range(N):
        out[n, :, 0].index_add_(0, idx, yf[n])
        out[n, :, 1].index_add_(0, idx, yf[n] * yf[n])
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


def bwd_reference(c, o, dtype=torch.float64):
    """dict(act, dx = gradient w.r.t. the activated input, dw, db) by autograd in `dtype` on the CPU."""
    t = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in o.items()}
    act = (affine(t["x"], t["pa"], t["pb"]) if c["pre"] else t["x"]).clone().requires_grad_(True)
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
