"""Case tables and CPU references of the exact tests of the two table-driven launches (rho_prep_batch, rho_wgrad_finalize_batch:
test_gpu_weight_tables.py) and of the one-channel ends (rho_stem_conv3d, rho_head_conv3d: test_gpu_ends.py).  Nothing here touches
the GPU or calls the library: every reference is plain torch indexing of the layout include/rho_hip.h documents, and
test_weight_table_cases_host.py ties each of them to a convolution identity on the CPU (so that none is a transcription of the
kernel it judges) and proves that every reference value is an integer the stored format holds exactly."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from detdata import det_normal
from exact_util import int_choice, int_tensor

CK = {"bf16": 32, "f32": 16}                       # channels per 64-byte chunk: the padding of a layout's contiguous axis
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
KIND_CODE = {"fwd": 0, "dgrad": 1, "phase": 2, "sel": 3, "vec": 4}        # RHO_PREP_* (include/rho_hip.h)

# sub-pixel phases of a 3-tap axis behind a nearest x2 upsample: phase code -> source taps summed into each of its 2 taps
PHASE_SETS = {1: ((0,), (1, 2)), 2: ((0, 1), (2,))}
# stride-2 parity split of a 3-tap axis: parity -> source taps (forward: on the input's parity; backward: on dX's parity)
S2_FWD = {0: (1,), 1: (0, 2)}
S2_BWD = {0: (1,), 1: (2, 0)}


def ceil_to(v: int, m: int) -> int:
    return -(-v // m) * m


def k3(shape) -> tuple:
    """(kd, kh, kw) of a parameter [cout, cin, *k]."""
    k = [int(v) for v in shape[2:]]
    return tuple([1] * (3 - len(k)) + k)


# ============================================================================================ layout references (pure indexing)
def _src_row(table, i: int, n: int) -> int:
    s = int(table[i]) if table is not None else (i if i < n else -1)
    return s if 0 <= s < n else -1


def ref_fwd(w: torch.Tensor, k, coutp: int, cinp: int, row_src=None) -> torch.Tensor:
    """out[tap][co][ci] = w[src(co)][ci][tap]; src = row_src[co] (rows whose source is outside [0, cout) are zero), padding zero."""
    cout, cin, taps = w.shape[0], w.shape[1], math.prod(k)
    w3 = w.reshape(cout, cin, taps)
    out = torch.zeros(taps, coutp, cinp, dtype=w.dtype)
    for co in range(coutp):
        s = _src_row(row_src, co, cout)
        if s >= 0:
            out[:, co, :cin] = w3[s].t()
    return out


def ref_dgrad(w: torch.Tensor, k, rowsp: int, colsp: int, col_src=None) -> torch.Tensor:
    """out[tap][ci][col] = w[src(col)][ci][taps - 1 - tap]: flipped taps, transposed channels (col_src is read for col < cout)."""
    cout, cin, taps = w.shape[0], w.shape[1], math.prod(k)
    w3 = w.reshape(cout, cin, taps)
    out = torch.zeros(taps, rowsp, colsp, dtype=w.dtype)
    for col in range(cout):
        s = _src_row(col_src, col, cout)
        if s >= 0:
            out[:, :cin, col] = w3[s].flip(-1).t()
    return out


def phase_taps(w5: torch.Tensor, ph) -> torch.Tensor:
    """[cout, cin, kd, kh', kw']: the taps of phase ``ph`` = (phase_h, phase_w) - on a phased axis the 3 taps fold into 2 by PHASE_SETS."""
    for dim, p in ((3, ph[0]), (4, ph[1])):
        if p:
            w5 = torch.stack([w5.index_select(dim, torch.tensor(s)).sum(dim) for s in PHASE_SETS[p]], dim)
    return w5


def ref_phase(w5: torch.Tensor, ph, d1: int, d2: int, dgrad: bool) -> torch.Tensor:
    w2 = phase_taps(w5, ph)
    return ref_dgrad(w2, w2.shape[2:], d1, d2) if dgrad else ref_fwd(w2, w2.shape[2:], d1, d2)


def sel_taps(w5: torch.Tensor, sel_hw, flip_d: bool) -> torch.Tensor:
    """[cout, cin, kd, len(sel_h), len(sel_w)]: new tap r of an axis = source tap sel[r] (None keeps the axis); flip_d mirrors D."""
    if flip_d:
        w5 = w5.flip(2)
    for dim, s in ((3, sel_hw[0]), (4, sel_hw[1])):
        if s is not None:
            w5 = w5.index_select(dim, torch.tensor(list(s)))
    return w5


def ref_sel(w5: torch.Tensor, sel_hw, flip_d: bool, dgrad: bool, d1: int, d2: int) -> torch.Tensor:
    """Forward: [tap][co][ci];  dgrad: [tap][ci][co] - channels transposed, the taps exactly as selected (the selection and flip_d
    carry the mirroring)."""
    w2 = sel_taps(w5, sel_hw, flip_d)
    cout, cin = w2.shape[:2]
    if not dgrad:
        return ref_fwd(w2, w2.shape[2:], d1, d2)
    out = torch.zeros(math.prod(w2.shape[2:]), d1, d2, dtype=w5.dtype)
    out[:, :cin, :cout] = w2.reshape(cout, cin, -1).permute(2, 1, 0)
    return out


def ref_vec(src: torch.Tensor, numel: int, perm=None, n=None) -> torch.Tensor:
    """out[i] = src[perm[i] if perm else i] for i < n (an index outside src: zero), zero up to numel."""
    src = src.reshape(-1)
    n = src.numel() if n is None else n
    out = torch.zeros(numel, dtype=src.dtype)
    for i in range(n):
        s = int(perm[i]) if perm is not None else i
        if 0 <= s < src.numel():
            out[i] = src[s]
    return out


def conv_weight_of(layout: torch.Tensor, rows: int, cols: int, k) -> torch.Tensor:
    """A [tap][row][col] layout read back as the conv weight [rows, cols, *k] the forward kernel applies."""
    return layout[:, :rows, :cols].permute(1, 2, 0).reshape(rows, cols, *k).contiguous()


# ============================================================================================ permutations
def qkv_row_src(c: int, heads: int) -> torch.Tensor:
    """UNetEngine._qkv_row_src for the legacy attention order: canonical row [Q heads | K heads | V heads] <- interleaved q, k, v per head."""
    ch = c // heads
    idx = torch.arange(3 * c, dtype=torch.int64)
    return ((idx % c) // ch * 3 * ch + idx // c * ch + idx % ch).to(torch.int32)


def holes_row_src(n: int, cout: int) -> torch.Tensor:
    """int32[n]: a scrambled injection into [0, cout) with -1 entries, one index == cout and one far beyond (all three: zero rows)."""
    idx = torch.full((n,), -1, dtype=torch.int32)
    for r in range(min(n, cout)):
        idx[r] = (7 * r + 3) % cout                # 7 is coprime to the couts used here: injective
    idx[1], idx[5], idx[min(n, cout) - 1] = -1, cout, 1000
    return idx


def head_as_gemm_perm(C: int, cinp: int, taps: int = 27) -> torch.Tensor:
    """_HeadAsGemm._perm: out[0][r = tap][c] = weight[0][c][r] for r < taps, c < C (flat index c * taps + r), else zero."""
    r, c = torch.arange(32).view(-1, 1), torch.arange(cinp).view(1, -1)
    return torch.where((r < taps) & (c < C), c * taps + r, torch.full_like(r + c, -1)).reshape(-1).to(torch.int32)


def head_dgrad_perm(C: int, taps: int = 27) -> torch.Tensor:
    """_HeadDgradW._perm: out[0][c][t] = weight[0][c][taps - 1 - t] for t < taps, else zero."""
    c, t = torch.arange(C).view(-1, 1), torch.arange(32).view(1, -1)
    return torch.where(t < taps, c * taps + (taps - 1 - t), torch.full_like(c + t, -1)).reshape(-1).to(torch.int32)


# ============================================================================================ B: rho_prep_batch
W_CLAMP = 60            # |w| <= 60: a phase tap sums up to 4 of them (<= 240 <= 256, exact in bf16)


def _wd(name, kind, wshape, **kw):
    return dict(name=f"{kind}_{name}", kind=kind, wshape=tuple(wshape), **kw)


def _prep_cases():
    cs = []
    for kind in ("fwd", "dgrad"):
        # cout 40 -> 64 padded rows; cin 72 -> a ragged second 64-group and a padded contiguous axis
        cs += [_wd("t1", kind, (40, 72, 1, 1, 1)),                       # elementwise
               _wd("t3", kind, (40, 72, 3)), _wd("t9", kind, (40, 72, 3, 3)), _wd("t27", kind, (40, 72, 3, 3, 3)),       # LDS
               _wd("t3_wide", kind, (72, 40, 3)),                        # the ragged group on the other axis
               _wd("t36", kind, (40, 72, 1, 6, 6)),                      # past the LDS tile: elementwise
               _wd("qkv_t1", kind, (96, 32, 1), perm="qkv"), _wd("qkv_t3", kind, (96, 32, 3), perm="qkv"),
               _wd("holes_t1", kind, (40, 72, 1), perm="holes"), _wd("holes_t3", kind, (40, 72, 3), perm="holes")]
    # 32 taps, the upper edge of the LDS path: forward through add_fwd's k override on a [cout, cin, 32] view
    cs += [_wd("t32", "fwd", (40, 72, 32), k=(1, 4, 8)), _wd("t32", "dgrad", (40, 72, 1, 4, 8)),
           _wd("t36k", "fwd", (40, 72, 36), k=(1, 6, 6))]
    for dg in (False, True):
        for ph in ((1, 1), (1, 2), (2, 1), (2, 2)):
            cs.append(_wd(f"333_{ph[0]}{ph[1]}{'_dgrad' if dg else ''}", "phase", (40, 72, 3, 3, 3), ph=ph, dgrad=dg))
        for ph in ((0, 1), (0, 2)):
            cs.append(_wd(f"133_{ph[0]}{ph[1]}{'_dgrad' if dg else ''}", "phase", (40, 72, 3, 3), ph=ph, dgrad=dg))
        for ab in ((0, 0), (0, 1), (1, 0), (1, 1)):
            sel = (S2_BWD[ab[0]], S2_BWD[ab[1]]) if dg else (S2_FWD[ab[0]], S2_FWD[ab[1]])
            cs.append(_wd(f"{ab[0]}{ab[1]}{'_dgrad' if dg else ''}", "sel", (40, 72, 3, 3, 3), sel=sel, flip_d=dg, dgrad=dg))
    cs += [_wd("bias_pad", "vec", (40,), out=(64,), out_dtype="f32"),
           _wd("perm_holes", "vec", (50,), out=(64,), perm="vec_holes", n=64, out_dtype="f32"),
           _wd("short_n", "vec", (100,), out=(128,), n=70, out_dtype="f32"),
           _wd("bf16_out", "vec", (72,), out=(96,), out_dtype="bf16"),
           _wd("head_as_gemm", "vec", (1, 32, 3, 3, 3), out=(1, 32, 32), perm="head_as_gemm", n=1024),
           _wd("head_dgrad", "vec", (1, 32, 3, 3, 3), out=(1, 32, 32), perm="head_dgrad", n=1024)]
    return cs


PREP_CASES = _prep_cases()
PREP_ONE_OP = "fwd_t27"           # the one-op table


@functools.lru_cache(maxsize=None)
def prep_io(name: str, dtype: str) -> dict:
    """Operands and reference of one op for a table of ``dtype``: w (float32), perm (int32 or None), out_shape, out_dtype, ref
    (float32, the values the layout must hold), k.  Cached: the tests share it and leave it unchanged."""
    c = next(c for c in PREP_CASES if c["name"] == name)
    kind, ws = c["kind"], c["wshape"]
    w = int_tensor(ws, "wt_" + name, 25.0, W_CLAMP)
    ck = CK[dtype]
    io = dict(case=c, w=w, perm=None, out_dtype=dtype, k=None)
    if kind == "vec":
        perm = {"vec_holes": lambda: torch.tensor([(11 * i + 5) % 50 if i % 5 else -1 for i in range(64)], dtype=torch.int32),
                "head_as_gemm": lambda: head_as_gemm_perm(32, 32), "head_dgrad": lambda: head_dgrad_perm(32), None: lambda: None}[c.get("perm")]()
        io.update(perm=perm, out_shape=c["out"], out_dtype=c.get("out_dtype") or dtype, n=c.get("n"),
                  ref=ref_vec(w, math.prod(c["out"]), perm, c.get("n")).reshape(c["out"]))
        return io
    cout, cin = ws[0], ws[1]
    k = tuple(c["k"]) if c.get("k") else k3(ws)
    io["k"] = k
    w5 = w.reshape(cout, cin, *k)
    d_f, d_b = (ceil_to(cout, 32), ceil_to(cin, ck)), (ceil_to(cin, 32), ceil_to(cout, ck))       # [rows][contiguous] of fwd / dgrad
    if kind in ("fwd", "dgrad"):
        n_perm = d_f[0] if kind == "fwd" else d_b[1]
        perm = {"qkv": lambda: qkv_row_src(cout // 3, 2), "holes": lambda: holes_row_src(n_perm, cout), None: lambda: None}[c.get("perm")]()
        assert perm is None or perm.numel() == n_perm
        io["perm"] = perm
        if kind == "fwd":
            io.update(out_shape=(math.prod(k),) + d_f, ref=ref_fwd(w, k, d_f[0], d_f[1], perm))
        else:
            io.update(out_shape=(math.prod(k),) + d_b, ref=ref_dgrad(w, k, d_b[0], d_b[1], perm))
        return io
    d1, d2 = d_b if c["dgrad"] else d_f
    if kind == "phase":
        ref = ref_phase(w5, c["ph"], d1, d2, c["dgrad"])
    else:
        ref = ref_sel(w5, c["sel"], c["flip_d"], c["dgrad"], d1, d2)
    io.update(out_shape=tuple(ref.shape), ref=ref)
    return io


def prep_into(sink, names, dtype: str, alloc, device="cpu") -> dict:
    """The ops ``names`` into ``sink`` - anything with the add_fwd / add_dgrad / add_phase / add_sel / add_vec methods of ops.PrepTable -
    with operands on ``device`` and each output from ``alloc(shape, torch dtype) -> (flat, view)``;  -> {name: (flat, view)}."""
    outs = {}
    for name in names:
        io = prep_io(name, dtype)
        c, w = io["case"], io["w"].to(device)
        perm = io["perm"].to(device) if io["perm"] is not None else None
        flat, out = alloc(io["out_shape"], TORCH_DTYPE[io["out_dtype"]])
        if c["kind"] == "fwd":
            sink.add_fwd(w, out, perm, k=c.get("k"))
        elif c["kind"] == "dgrad":
            sink.add_dgrad(w, out, perm)
        elif c["kind"] == "phase":
            sink.add_phase(w, out, c["ph"], dgrad=c["dgrad"])
        elif c["kind"] == "sel":
            sink.add_sel(w, out, c["sel"], flip_d=c["flip_d"], dgrad=c["dgrad"])
        else:
            sink.add_vec(w.reshape(-1), out, perm=perm, n=io["n"])
        outs[name] = (flat, out)
    return outs


def prep_geometry(io: dict, max_blocks: int = 2048) -> dict:
    """The launch geometry PrepTable gives the op: nblk blocks, and on the LDS path (FWD / DGRAD, 1 < taps <= 32) the units they walk."""
    total = math.prod(io["out_shape"])
    nblk = max(1, min((total + 1023) // 1024, max_blocks))
    taps = math.prod(io["k"]) if io["k"] else 1
    lds = io["case"]["kind"] in ("fwd", "dgrad") and 1 < taps <= 32
    units = io["out_shape"][1] * -(-io["out_shape"][2] // 64) if lds else None
    return dict(total=total, nblk=nblk, lds=lds, units=units)


# ============================================================================================ C: rho_wgrad_finalize_batch
def _fd(name, kind, cout, cin, coutp, cinb, k, **kw):
    return dict(name=name, kind=kind, cout=cout, cin=cin, coutp=coutp, cinb=cinb, k=tuple(k), **kw)


WFIN_CASES = [
    _fd("k0_t1", 0, 40, 72, 64, 80, (1, 1, 1)),                                  # elementwise
    _fd("k0_t3", 0, 40, 72, 64, 80, (1, 1, 3)),                                  # LDS: ragged second channel group
    _fd("k0_t27", 0, 40, 72, 64, 80, (3, 3, 3)),
    _fd("k0_t32", 0, 40, 72, 64, 80, (1, 4, 8)),                                 # upper edge of the LDS path
    _fd("k0_t36", 0, 40, 72, 64, 80, (1, 6, 6)),                                 # past it: elementwise
    _fd("k0_t27_nblk1", 0, 40, 72, 64, 80, (3, 3, 3), nblk=1),                   # one block walks every unit
    _fd("k0_t36_nblk1", 0, 40, 72, 64, 80, (1, 6, 6), nblk=1),
    _fd("k0_qkv_t1", 0, 96, 32, 96, 32, (1, 1, 1), rs="qkv"),
    _fd("k0_qkv_t3", 0, 96, 32, 96, 32, (1, 1, 3), rs="qkv"),
    _fd("k0_holes_t1", 0, 40, 72, 64, 80, (1, 1, 1), rs="holes"),
    _fd("k0_holes_t3", 0, 40, 72, 64, 80, (1, 1, 3), rs="holes"),
    _fd("k0_bias", 0, 40, 1, 64, 1, (1, 1, 1)),                                  # a bias: cin = 1, coutp = the width of dY
    _fd("k0_bias_qkv", 0, 96, 1, 96, 1, (1, 1, 1), rs="qkv"),
    _fd("k0_stem", 0, 32, 27, 32, 32, (1, 1, 1)),                                # the stem's im2col form
    _fd("k0_head_bias", 0, 1, 1, 1, 1, (1, 1, 1), off_extra=13),                 # centre column of the head's im2col sums
    _fd("k1_333_11", 1, 40, 72, 64, 96, (3, 3, 3), up=(1, 1)),
    _fd("k1_333_01", 1, 40, 72, 64, 96, (3, 3, 3), up=(0, 1)),
    _fd("k1_333_10", 1, 40, 72, 64, 96, (3, 3, 3), up=(1, 0)),
    _fd("k1_133_11", 1, 40, 72, 64, 96, (1, 3, 3), up=(1, 1)),
    _fd("k1_133_01", 1, 40, 72, 64, 96, (1, 3, 3), up=(0, 1)),
    _fd("k1_133_10", 1, 40, 72, 64, 96, (1, 3, 3), up=(1, 0)),
    _fd("k2_c32", 2, 1, 32, 32, 32, (3, 3, 3)),
    _fd("k2_c64", 2, 1, 64, 32, 64, (3, 3, 3)),
]
WFIN_ONE_OP = "k0_t27"
PHASE_PAD = 192         # floats between the end of one phase buffer and the next: phase_stride > one buffer


def wfin_phases(up):
    """Phase codes of one upsampled conv in the order their buffers lie in the arena: (a, b) for a in H phases for b in W phases."""
    return [(a, b) for a in ((1, 2) if up[0] else (0,)) for b in ((1, 2) if up[1] else (0,))]


def wfin_buffer_floats(c: dict) -> int:
    """One accumulation buffer of the op (kind 1: one phase's)."""
    k, up = c["k"], c.get("up", (0, 0))
    if c["kind"] == 2:                               # [32 rows = taps, padded][cinb]
        return c["coutp"] * c["cinb"]
    taps = k[0] * (2 if up[0] else k[1]) * (2 if up[1] else k[2])
    return taps * c["coutp"] * c["cinb"]


def wfin_stride(c: dict) -> int:
    return wfin_buffer_floats(c) + PHASE_PAD if c["kind"] == 1 else 0


def wfin_region_floats(c: dict) -> int:
    if c["kind"] == 1:
        return len(wfin_phases(c["up"])) * wfin_stride(c)
    return wfin_buffer_floats(c) + (32 if c.get("off_extra") else 0)


def wfin_row_src(c: dict):
    return {"qkv": lambda: qkv_row_src(c["cout"] // 3, 2), "holes": lambda: holes_row_src(c["cout"], c["cout"]), None: lambda: None}[c.get("rs")]()


def ref_wfin(c: dict, region: torch.Tensor, grad0: torch.Tensor, row_src=None) -> torch.Tensor:
    """grad0 + the op's reading of its arena region.  kind 0: grad[row_src(r)][ci][tap] += dw[tap][r][ci] (a row whose target is
    outside [0, cout) is skipped);  kind 1: every phase's taps added to the 3-tap parameter taps they were summed from (the transpose
    of PHASE_SETS);  kind 2: grad[0][ci][tap] += dw[taps - 1 - tap][ci] (rows past the taps are not read)."""
    cout, cin, coutp, cinb, k = c["cout"], c["cin"], c["coutp"], c["cinb"], c["k"]
    taps = math.prod(k)
    g = grad0.clone().reshape(cout, cin, taps)
    region = region[c.get("off_extra", 0):]
    if c["kind"] == 0:
        dw = region[:taps * coutp * cinb].view(taps, coutp, cinb)
        for r in range(cout):
            d = _src_row(row_src, r, cout)
            if d >= 0:
                g[d] += dw[:, r, :cin].t()
    elif c["kind"] == 2:
        dw = region[:coutp * cinb].view(coutp, cinb)
        g[0] += dw[:taps, :cin].flip(0).t()
    else:
        g5 = g.view(cout, cin, *k)
        for p, (a, b) in enumerate(wfin_phases(c["up"])):
            kh2, kw2 = (2 if a else k[1]), (2 if b else k[2])
            dw = region[p * wfin_stride(c):][:k[0] * kh2 * kw2 * coutp * cinb].view(k[0], kh2, kw2, coutp, cinb)
            hs = PHASE_SETS[a] if a else tuple((t,) for t in range(k[1]))
            ws = PHASE_SETS[b] if b else tuple((t,) for t in range(k[2]))
            for r2, hset in enumerate(hs):
                for ky in hset:
                    for c2, wset in enumerate(ws):
                        for kx in wset:
                            g5[:, :, :, ky, kx] += dw[:, r2, c2, :cout, :cin].permute(1, 2, 0)
    return g.reshape(grad0.shape)


@functools.lru_cache(maxsize=None)
def wfin_io(names: tuple) -> dict:
    """A synthetic arena for the ops ``names`` (regions 64-float aligned, in order): arena (integer-valued float32), per op the
    region offset, the prefilled gradient, the row table and the reference result."""
    cases = [next(c for c in WFIN_CASES if c["name"] == n) for n in names]
    offs, total = [], 0
    for c in cases:
        offs.append(total)
        total += ceil_to(wfin_region_floats(c), 64)
    arena = int_tensor((total,), "wfin_arena" + names[0], 20.0, 50)
    arena = torch.where(arena == 0, torch.full_like(arena, 3.0), arena)          # no zeros: a row that must not be read holds a value
    ops = []
    for c, off in zip(cases, offs):
        shape = (c["cout"], c["cin"]) + c["k"]
        g0 = int_tensor(shape, "wfin_g" + c["name"], 4.0, 9)
        rs = wfin_row_src(c)
        ops.append(dict(case=c, off=off, grad0=g0, rs=rs, ref=ref_wfin(c, arena[off:off + wfin_region_floats(c)], g0, rs)))
    return dict(arena=arena, ops=ops)


def wfin_nblk(total: int) -> int:
    return max(1, min(-(-total // 256), 512))


# ============================================================================================ D: the one-channel ends
TD, TH, TW = 4, 8, 8                                # the output tile of k_stem3d / k_head3d
STEM_SHAPES = [(1, 1, 1, 1), (1, 4, 8, 8), (2, 5, 9, 11), (3, 4, 8, 16)]          # one position; one exact tile; ragged, 8 tiles; 2 tiles
STEM_COUTS = [32, 64]
RAGGED = (2, 5, 9, 11)
HEAD_DGRAD_CS = [32, 64]
HEAD_CS = [32, 64, 96, 128]
HEAD_SHAPES = STEM_SHAPES[:3]
HEAD_PROLOGUES = [None, "affine"]


def ends_tiles(D, H, W) -> int:
    return -(-D // TD) * -(-H // TH) * -(-W // TW)


@functools.lru_cache(maxsize=None)
def stem_case(shape, cout) -> dict:
    """x, w, b (integer-valued float32) and the fp64 reference y [N, cout, D, H, W] with its per-tile statistics."""
    N, D, H, W = shape
    x = int_tensor((N, 1, D, H, W), f"stem_ex_x{shape}", 1.0, 2)
    w = int_tensor((cout, 1, 3, 3, 3), f"stem_ex_w{cout}", 1.0, 2)
    b = int_tensor((cout,), f"stem_ex_b{cout}", 1.5, 3)
    y = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    return dict(x=x, w=w, b=b, y=y, stats=tile_stats(y))


def tile_stats(y: torch.Tensor) -> torch.Tensor:
    """[N, tiles, 2, C] float64: per 4 x 8 x 8 tile (index (td * tiles_h + th) * tiles_w + tw) the sum and the sum of squares over the
    tile's positions inside the volume."""
    N, C, D, H, W = y.shape
    nd, nh, nw = -(-D // TD), -(-H // TH), -(-W // TW)
    st = torch.zeros(N, nd * nh * nw, 2, C, dtype=torch.float64)
    for td in range(nd):
        for th in range(nh):
            for tw in range(nw):
                blk = y[:, :, td * TD:(td + 1) * TD, th * TH:(th + 1) * TH, tw * TW:(tw + 1) * TW].double()
                st[:, (td * nh + th) * nw + tw, 0] = blk.sum((2, 3, 4))
                st[:, (td * nh + th) * nw + tw, 1] = (blk * blk).sum((2, 3, 4))
    return st


def stem_weight_layout(w: torch.Tensor) -> torch.Tensor:
    """[1, cout, 32]: the im2col form rho_stem_conv3d reads, W[co][tap] with taps 27 .. 31 zero."""
    cout = w.shape[0]
    out = torch.zeros(1, cout, 32)
    out[0, :, :27] = w.reshape(cout, 27)
    return out


def head_weight_layout(w: torch.Tensor) -> torch.Tensor:
    """[1, 32, C]: the taps-as-rows form rho_head_conv3d reads, W[tap][c] with rows 27 .. 31 zero."""
    C = w.shape[1]
    out = torch.zeros(1, 32, C)
    out[0, :27] = w[0].reshape(C, 27).t()
    return out


@functools.lru_cache(maxsize=None)
def head_dgrad_case(C) -> dict:
    """Integer head parameter [1, C, 3, 3, 3], dpred [N, 1, D, H, W] and dact = d(conv3d(act, w, padding=1)) / d(act) by fp64 autograd."""
    N, D, H, W = RAGGED
    w = int_tensor((1, C, 3, 3, 3), f"hdg_w{C}", 1.0, 2)
    dpred = int_tensor((N, 1, D, H, W), "hdg_dp", 1.0, 2)
    act = torch.zeros(N, C, D, H, W, dtype=torch.float64, requires_grad=True)
    F.conv3d(act, w.double(), None, padding=1).backward(dpred.double())
    return dict(w=w, dpred=dpred, dact=act.grad.detach())


@functools.lru_cache(maxsize=None)
def head_case(C, shape, prologue) -> dict:
    """Integer operands of the head: x [N, C, D, H, W] in [-2, 2], a sparse w [1, C, 3, 3, 3] in {-1, 0, 1}, an integer bias, and
    (prologue) a per-(sample, channel) affine a in {1, 2, -1}, b a NON-ZERO integer, no SiLU.  References in fp64: the activated
    input, the per-tap partials T [N, 27, D, H, W] (what the kernel rounds to bf16) and out with / without the bias."""
    N, D, H, W = shape
    tag = f"head_ex{C}{shape}"
    x = int_tensor((N, C, D, H, W), tag + "x", 1.0, 2)
    w = int_choice((1, C, 3, 3, 3), tag + "w", (0, 0, 0, 1, 0, 0, 0, -1, 0, 0))
    bias = torch.tensor([5.0])
    c = dict(x=x, w=w, bias=bias, pre_a=None, pre_b=None)
    act = x.double()
    if prologue is not None:
        c["pre_a"] = int_choice((N, C), tag + "a", (1, 2, -1))
        c["pre_b"] = int_choice((N, C), tag + "b", (-2, -1, 1, 2))
        act = c["pre_a"].double().view(N, C, 1, 1, 1) * act + c["pre_b"].double().view(N, C, 1, 1, 1)
    c["act"] = act
    c["T"] = torch.einsum("ct,ncdhw->ntdhw", w[0].reshape(C, 27).double(), act)
    c["out_nobias"] = F.conv3d(act, w.double(), None, padding=1)
    c["out"] = c["out_nobias"] + bias.double()
    return c


V_CAP = 16.0            # |a x + b| of the SiLU case stays below this (the slack of its bound is counted for it)


@functools.lru_cache(maxsize=None)
def head_silu_case(C) -> dict:
    """Real-valued operands on the ragged shape (x and w bf16-representable) with the fp64 reference and the two magnitude sums of
    the bound: sum_tap sum_c |w * act| and sum_tap |T| at each output position (the conv pads the ACTIVATED tensor with zeros)."""
    N, D, H, W = RAGGED
    bf = lambda t: t.to(torch.bfloat16).float()                                                # noqa: E731
    x = bf(det_normal((N, C, D, H, W), f"hs_x{C}"))
    w = bf(det_normal((1, C, 3, 3, 3), f"hs_w{C}") / math.sqrt(27.0 * C))
    a = 1 + 0.3 * det_normal((N, C), f"hs_a{C}")
    b = 0.2 * det_normal((N, C), f"hs_b{C}")
    bias = torch.tensor([0.25])
    v = a.double().view(N, C, 1, 1, 1) * x.double() + b.double().view(N, C, 1, 1, 1)
    act = v * torch.sigmoid(v)
    wd = w.double()
    out = F.conv3d(act, wd, bias.double(), padding=1)
    mag_prod = F.conv3d(act.abs(), wd.abs(), None, padding=1)
    T = torch.einsum("ct,ncdhw->ntdhw", wd[0].reshape(C, 27), act)                             # [N, 27, D, H, W]
    eye = torch.eye(27, dtype=torch.float64).view(1, 27, 3, 3, 3)                              # tap t of T read at its own offset
    mag_T = F.conv3d(T.abs(), eye, None, padding=1)
    return dict(x=x, w=w, pre_a=a, pre_b=b, bias=bias, v=v, out=out, mag_prod=mag_prod, mag_T=mag_T)


# silu_f (csrc/common.h) = x * rcp(1 + exp2(-1.4426950408889634f * x)) on v = fmaf(a, x, b), against the fp64 a * x + b and sigmoid, in
# units of U = 2^-24 relative to |silu(v)|:  v itself 1 (the fmaf rounding, carried by the leading factor x);  the exponent's argument
# 3 relative roundings (v, the constant, the product), which exp2 turns into 3 |c v| ln 2 = 3 |v| relative in e;  v_exp_f32 1 ulp = 2;
# e / (1 + e) <= 1 of those reach the sum;  the add 1;  v_rcp_f32 1 ulp = 2;  the final product 1:  (7 + 3 |v|) U <= 55 U at |v| <= 16.
# The activation is then rounded to bf16 (the 2^-9 of the bound), so against that unit the slack is 55 * 2^-24 / 2^-9.
SILU_SLACK = (7 + 3 * V_CAP) * 2.0 ** -24 / 2.0 ** -9


def head_silu_bound(c: dict) -> torch.Tensor:
    return 2.0 ** -9 * (c["mag_prod"] + c["mag_T"]) * (1 + SILU_SLACK) + 27 * 2.0 ** -24 * c["mag_T"]
