"""Case tables and CPU references of the embedding-path tests: rho_linear / rho_linear_bwd, rho_timestep_embed with its MLP and
rho_multi_embed / rho_multi_embed_bwd.  Imported by test_embed_cases_host.py (which checks the references against torch autograd and
the oracle, the representability of every integer case and the coverage of the tables, without a GPU) and by the -m gpu module
test_gpu_exact_embedding.py.  Nothing here imports the package under test.

Two kinds of operands:
  int   x, w in [-8, 8], bias / add / dout in [-64, 64], prefilled gradients in [-64, 64]: |sum| <= 2048 * 64 + 128 < 2^24, so every
        product, every partial sum in ANY order (wave butterfly, atomic slices, ordered walk) and every result is exact in fp32 and the
        kernel must equal the fp64 reference bit for bit.  Activation codes 0 and 2 only (ReLU keeps integers).
  real  det_normal operands and a derived per-element bound |got - ref| <= n * 2^-24 * (sum of the terms' magnitudes):
          rho_linear        a lane's chain is ceil(K / 64) fmas, 6 butterfly adds, bias, add:  n = ceil(K / 64) + 8
          dw, db            a thread's chain over the batch (+ the value accumulated onto):    n = batch + 1
          dx                out_dim fmas in ceil(out_dim / 64) slices, the act' product, the atomic adds:  n = out_dim + ceil(out_dim / 64) + 3
        An activation other than identity / ReLU adds the device libm's error: `act_ulps[code] = (forward, derivative)` fp32 ulps of
        the activation's term magnitude (act_mag64 / dact_mag64: where the expression cancels - GELU and 1 + erf, SiLU' and 1 - s,
        Tanh' and 1 - t^2 - the magnitudes of the terms, not of their difference).  The allowances are measured on the device once and
        stand in test_gpu_exact_embedding.py; they are an argument here."""
from __future__ import annotations

import math

import numpy as np
import torch

from detdata import det_normal
from exact_util import f32_ulp as _f32_ulp, int_tensor

U = 2.0 ** -24                 # unit roundoff of fp32
ACTS = (0, 1, 2, 3, 4, 5, 6)   # identity, SiLU, ReLU, GELU (erf), Tanh, Sigmoid, ELU(1)
INT_ACTS = (0, 2)
ACT_NAMES = ("id", "silu", "relu", "gelu", "tanh", "sigmoid", "elu")
LIP = 1.13                     # sup |act'| over the seven codes (GELU': 1.129 at u = sqrt(2); SiLU': 1.0998)
# code -> (forward, derivative) allowance of the device libm expressions (act_other_f / dact_other_f and the embedding path's SiLU) in
# fp32 ulps of the term magnitude; measured and derived in the docstring of test_gpu_exact_embedding.py, shared by every exact suite
ACT_ULPS = {1: (3, 3), 3: (3, 3), 4: (2, 2), 5: (4, 4), 6: (2, 2)}
_SQRT1_2 = 0.7071067811865476
_INV_SQRT_2PI = 0.3989422804014327


# ----------------------------------------------------------------------------- activations in float64
def _sig(u):
    return 1.0 / (1.0 + torch.exp(-u))


def _phi(u):
    return _INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def act64(u: torch.Tensor, code: int) -> torch.Tensor:
    u = u.double()
    if code == 0:
        return u
    if code == 1:
        return u * _sig(u)
    if code == 2:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if code == 3:
        return 0.5 * u * (1.0 + torch.erf(u * _SQRT1_2))
    if code == 4:
        return torch.tanh(u)
    if code == 5:
        return _sig(u)
    if code == 6:
        return torch.where(u > 0, u, torch.expm1(u))
    raise ValueError(code)


def dact64(u: torch.Tensor, code: int) -> torch.Tensor:
    u = u.double()
    if code == 0:
        return torch.ones_like(u)
    if code == 1:
        s = _sig(u)
        return s * (1.0 + u * (1.0 - s))
    if code == 2:
        return (u > 0).double()
    if code == 3:
        return 0.5 * (1.0 + torch.erf(u * _SQRT1_2)) + u * _phi(u)
    if code == 4:
        return 1.0 - torch.tanh(u) ** 2
    if code == 5:
        s = _sig(u)
        return s * (1.0 - s)
    if code == 6:
        return torch.where(u > 0, torch.ones_like(u), torch.exp(u))
    raise ValueError(code)


def act_mag64(u: torch.Tensor, code: int) -> torch.Tensor:
    """Magnitude of the terms of act(u) as the kernels write it (>= |act(u)|; larger only where the expression cancels)."""
    u = u.double()
    if code == 3:                                       # 0.5 u (1 + erf): 1 + erf cancels for u < 0
        return 0.5 * u.abs() * (1.0 + torch.erf(u * _SQRT1_2).abs())
    return act64(u, code).abs()


def dact_mag64(u: torch.Tensor, code: int) -> torch.Tensor:
    """Magnitude of the terms of act'(u) as the kernels write it."""
    u = u.double()
    if code == 1:                                       # s (1 + u (1 - s)): terms 1, u, u s
        s = _sig(u)
        return s * (1.0 + u.abs() * (1.0 + s))
    if code == 3:
        return 0.5 * (1.0 + torch.erf(u * _SQRT1_2).abs()) + u.abs() * _phi(u)
    if code == 4:                                       # 1 - t t
        return 1.0 + torch.tanh(u) ** 2
    if code == 5:                                       # s (1 - s)
        s = _sig(u)
        return s * (1.0 + s)
    return dact64(u, code).abs()


# ----------------------------------------------------------------------------- the kernels that use common.h's silu_f / act_other_f
# (rho_bias_act, the GroupNorm passes, the conv loaders).  Code 1 is silu_f / dsilu_f of common.h: x * rcp(1 + exp2(t)), t = fl(c * x),
# c = fl32(-log2 e).  With u = 2^-24, w = 1 - sigmoid(x):
#   t: c is 0.15 u from -log2 e and the product rounds once: |dt| <= 1.15 u |t|, which is ln2 * 1.15 u |t| < 0.8 u |t| relative in 2^t;
#   v_exp_f32: 1 ulp <= 2 u relative; so e = exp2(t) carries (2 + 0.8 |t|) u, and enters 1 + e with weight e / (1 + e) = w;
#   the addition rounds (1 u), v_rcp_f32: 1 ulp <= 2 u: s = rcp(1 + e) carries rho u, rho = w (2 + 0.8 |t|) + 3;
#   silu: the product with x rounds once more: (rho + 1) u |silu(x)|, i.e. SILU_F_ULPS(x) = w (2 + 0.8 |t|) + 4 ulps;
#   dsilu = s (1 + x (1 - s)): a = 1 - s: s's error + 1 rounding; x a: 1 rounding; 1 + x a: 1 rounding; the product with s: its error
#   on |c| <= 1 + |x| a and 1 rounding: in all rho u s (1 + |x| a + |x| s) + u s (4 |x| a + 2) <= (rho + 4) u Mag with
#   Mag = s (1 + |x| (1 + s)) = dact_mag64: DSILU_F_ULPS(x) = w (2 + 0.8 |t|) + 7 ulps of Mag.
# The bound grows with |x| on the negative side only (w -> 1); at x = -6 it is 12.9 / 15.9 ulps, at x = +6 it is 4.0 / 7.0.
# Codes 2 - 6 are act_other_f / dact_other_f, the libm expressions of the embedding path: ACT_ULPS (code 2: exact).
_LOG2E = 1.4426950408889634


def silu_f_ulps(u64: torch.Tensor, derivative: bool) -> torch.Tensor:
    w = 1.0 / (1.0 + torch.exp(u64))
    return w * (2.0 + 0.8 * _LOG2E * u64.abs()) + (7.0 if derivative else 4.0)


def hw_act_bound(u64: torch.Tensor, code: int, derivative: bool):
    """(reference, absolute fp32 bound, term magnitude) of act(u) or act'(u), per element."""
    want = (dact64 if derivative else act64)(u64, code)
    mag = (dact_mag64 if derivative else act_mag64)(u64, code)
    if code == 1:
        return want, silu_f_ulps(u64, derivative) * _f32_ulp(mag), mag
    ulps = 0.0 if code in INT_ACTS else float(ACT_ULPS[code][int(derivative)])
    return want, ulps * _f32_ulp(mag), mag


def _ulps(act_ulps, code: int, which: int) -> float:
    if code in INT_ACTS:
        return 0.0
    return float(act_ulps[code][which])


# ----------------------------------------------------------------------------- rho_linear
LIN_K = (1, 63, 64, 65, 256, 257, 1024, 1025, 2048)     # under one wave; k_linear<4> | <16> at 256 | 257; <16> | <32> at 1024 | 1025; limit
LIN_O = (1, 3, 4, 5, 130)                               # 4 output features per workgroup: partial last workgroup unless O % 4 == 0
LIN_B = (1, 3)


def _linear_cases():
    out, n_real = [], 0
    for ik, K in enumerate(LIN_K):
        for io, O in enumerate(LIN_O):
            j = ik * len(LIN_O) + io
            kind = "int" if (ik + io) % 2 == 0 else "real"
            B = LIN_B[(ik + (io >> 1)) % 2]
            bias, add = (j % 3) != 1, ((j + ik) % 4) < 2
            if kind == "int":
                ai, ao = INT_ACTS[(j >> 1) % 2], INT_ACTS[(j >> 2) % 2]
            else:
                ai, ao = ACTS[n_real % 7], ACTS[(3 * n_real + 1) % 7]
                n_real += 1
            out.append(dict(name=f"K{K}_O{O}_B{B}_{'b' if bias else '-'}{'a' if add else '-'}_{ACT_NAMES[ai]}_{ACT_NAMES[ao]}_{kind}",
                            K=K, O=O, B=B, bias=bias, add=add, act_in=ai, act_out=ao, kind=kind))
    return out


LINEAR_CASES = _linear_cases()


# w = I, K = O = 64: out = act(x) element for element - the cases the libm allowances are measured and asserted on
def code_inputs() -> torch.Tensor:
    """[16, 64]: half the rows drawn like the real cases' x, half a grid over [-6, 6] (the range 1.5 * det_normal can reach)."""
    g = torch.linspace(-6.0, 6.0, 8 * 64, dtype=torch.float64).float().view(8, 64)
    return torch.cat([det_normal((8, 64), "codex") * 1.5, g], 0).contiguous()


def linear_operands(c) -> dict:
    K, O, B, n = c["K"], c["O"], c["B"], "lin_" + c["name"]
    if c["kind"] == "int":
        x, w = int_tensor((B, K), n + "x", 3.0, 8), int_tensor((O, K), n + "w", 3.0, 8)
        bias = int_tensor((O,), n + "b", 24.0, 64) if c["bias"] else None
        add = int_tensor((B, O), n + "a", 24.0, 64) if c["add"] else None
    else:
        x, w = det_normal((B, K), n + "x") * 1.5, det_normal((O, K), n + "w") / math.sqrt(K)
        bias = det_normal((O,), n + "b") * 0.5 if c["bias"] else None
        add = det_normal((B, O), n + "a") * 0.5 if c["add"] else None
    return dict(x=x, w=w, bias=bias, add=add)


def linear_ref(x, w, bias, add, act_in: int, act_out: int, act_ulps=None):
    """(out, bound): the float64 forward and the per-element bound of the module docstring (act_ulps None: integer codes only)."""
    x64, w64 = x.double(), w.double()
    a = act64(x64, act_in)
    r = a @ w64.T
    S = a.abs() @ w64.abs().T
    if bias is not None:
        r, S = r + bias.double(), S + bias.double().abs()
    if add is not None:
        r, S = r + add.double(), S + add.double().abs()
    n = math.ceil(x.shape[1] / 64) + 8
    br = n * U * S
    if act_in not in INT_ACTS:
        br = br + _ulps(act_ulps, act_in, 0) * 2 * U * (act_mag64(x64, act_in) @ w64.abs().T)
    if act_out in INT_ACTS:                             # identity; ReLU is exact and 1-Lipschitz
        return act64(r, act_out), br
    # act_f32(r_dev) vs act64(r_ref): the activation's slope times the error of r, plus the libm allowance at the term magnitude
    return act64(r, act_out), LIP * br + _ulps(act_ulps, act_out, 0) * 2 * U * (act_mag64(r, act_out) + 2 * br)


# ----------------------------------------------------------------------------- rho_linear_bwd
BWD_K = (1, 65, 257)
BWD_O = (1, 63, 64, 65, 130)                            # k_linear_bwd_x deals out_dim to atomic slices of 64
BWD_B = (1, 5)
BWD_ABSENT = (None, "dw", "db", "dx")


def _bwd_cases():
    out, n_real = [], 0
    for ik, K in enumerate(BWD_K):
        for io, O in enumerate(BWD_O):
            for ib, B in enumerate(BWD_B):
                j = (ik * len(BWD_O) + io) * 2 + ib
                kind = "int" if (ik + io + ib) % 2 == 0 else "real"
                strided = (io + ib + (ik >> 1)) % 2 == 1
                absent = BWD_ABSENT[(io + 2 * ib + ik) % 4] if j % 3 != 2 else None
                acc_params, acc_dx = (j // 3) % 2 == 1, ((j >> 1) + ik) % 2 == 1
                if kind == "int":
                    ai = INT_ACTS[(j >> 2) % 2]
                else:
                    ai = ACTS[n_real % 7]
                    n_real += 1
                out.append(dict(name=f"K{K}_O{O}_B{B}_{'s' if strided else 'c'}_{ACT_NAMES[ai]}_no{absent}_"
                                     f"{'P' if acc_params else 'p'}{'X' if acc_dx else 'x'}_{kind}",
                                K=K, O=O, B=B, stride=O + 7 if strided else 0, act_in=ai, absent=absent, acc_params=acc_params,
                                acc_dx=acc_dx, kind=kind))
    return out


LINEAR_BWD_CASES = _bwd_cases()
BWD_COL0 = 3                   # first column of the slice inside the [B, O + 7] tensor of a strided case


def linear_bwd_operands(c) -> dict:
    K, O, B, n = c["K"], c["O"], c["B"], "lbw_" + c["name"]
    if c["kind"] == "int":
        x, w = int_tensor((B, K), n + "x", 3.0, 8), int_tensor((O, K), n + "w", 3.0, 8)
        dout = int_tensor((B, O), n + "g", 24.0, 64)
    else:
        x, w = det_normal((B, K), n + "x") * 1.5, det_normal((O, K), n + "w") / math.sqrt(K)
        dout = det_normal((B, O), n + "g")
    # the values accumulated onto are integers in both kinds
    pre = dict(dw=int_tensor((O, K), n + "pw", 24.0, 64), db=int_tensor((O,), n + "pb", 24.0, 64),
               dx=int_tensor((B, K), n + "px", 24.0, 64))
    return dict(x=x, w=w, dout=dout, pre=pre)


def linear_bwd_ref(dout, x, w, act_in: int, pre_dw=None, pre_db=None, pre_dx=None, act_ulps=None):
    """{dw, db, dx: (float64 value, bound)}; pre_*: what the launch accumulates onto (None: it writes)."""
    g, x64, w64 = dout.double(), x.double(), w.double()
    B, O = g.shape
    a, da = act64(x64, act_in), dact64(x64, act_in)
    z = lambda t, like: torch.zeros_like(like) if t is None else t.double()
    dw, Sw = g.T @ a, g.abs().T @ a.abs()
    bw = (B + 1) * U * (Sw + z(pre_dw, dw).abs())
    if act_in not in INT_ACTS:
        bw = bw + _ulps(act_ulps, act_in, 0) * 2 * U * (g.abs().T @ act_mag64(x64, act_in))
    db = g.sum(0)
    bb = (B + 1) * U * (g.abs().sum(0) + z(pre_db, db).abs())
    s, G = g @ w64, g.abs() @ w64.abs()
    dx = da * s
    bx = (O + math.ceil(O / 64) + 3) * U * (da.abs() * G + z(pre_dx, dx).abs())
    if act_in not in INT_ACTS:
        bx = bx + _ulps(act_ulps, act_in, 1) * 2 * U * (dact_mag64(x64, act_in) * G)
    return dict(dw=(dw + z(pre_dw, dw), bw), db=(db + z(pre_db, db), bb), dx=(dx + z(pre_dx, dx), bx))


# ----------------------------------------------------------------------------- rho_timestep_embed
TE_DIM = (2, 6, 64, 130, 320)                           # dim / 2 frequencies; the dot products stride dim by 64
TE_EDIM = (1, 3, 4, 5, 70, 256, 260)                    # four waves stride the outputs by 4; the second linear strides edim by 64
TE_B = (1, 3)
TE_T = (0, 1, 999, 100000)
PE_ABS = 5e-7                                           # the project's bar for the sinusoid (test_gpu_kernels.py)


def _te_cases():
    out = []
    for idim, dim in enumerate(TE_DIM):
        for ie, edim in enumerate(TE_EDIM):
            j = idim * len(TE_EDIM) + ie
            B = TE_B[(idim + ie) % 2]
            act, t_scalar = ACTS[(idim + ie) % 7], (2 * idim + ie) % 3 == 1
            t = [TE_T[(j + (0 if t_scalar else b)) % 4] for b in range(B)]      # t_scalar_dev: one value for every row
            out.append(dict(name=f"dim{dim}_e{edim}_B{B}_{ACT_NAMES[act]}", dim=dim, edim=edim, B=B, t=t, act=act,
                            t_scalar=t_scalar, cond=(j % 4) != 2,
                            pe_out=((j >> 1) + idim) % 2 == 0, h_out=(j + (ie >> 1)) % 2 == 0))
    return out


TE_CASES = _te_cases()


def te_omega(dim: int, wavelength: int = 10000) -> torch.Tensor:
    """float32 [dim / 2]: wavelength^(2i / dim), the expression of the reference (models/common.py:38)."""
    i = torch.arange(dim // 2)
    return torch.pow(wavelength, 2 * i / dim).to(torch.float32).contiguous()


def te_operands(c) -> dict:
    dim, edim, B, n = c["dim"], c["edim"], c["B"], "te_" + c["name"]
    return dict(omega=te_omega(dim), t=torch.tensor(c["t"], dtype=torch.int64),
                w0=det_normal((edim, dim), n + "w0") * math.sqrt(2.0 / dim), b0=det_normal((edim,), n + "b0") * 0.3,
                w2=det_normal((edim, edim), n + "w2") / math.sqrt(edim), b2=det_normal((edim,), n + "b2") * 0.3,
                cond=det_normal((B, edim), n + "c") * 0.5)


def te_sinusoid64(t: torch.Tensor, omega: torch.Tensor) -> torch.Tensor:
    """float64 [B, dim]: sin / cos (float64) of the float32 quotient float32(t) / omega the kernel forms, interleaved."""
    arg = (t.to(torch.float32)[:, None] / omega[None, :]).double()
    return torch.stack([torch.sin(arg), torch.cos(arg)], -1).reshape(t.shape[0], -1)


def te_chain_ref(pe_dev: torch.Tensor, o: dict, act: int, cond, act_ulps):
    """(emb, bound) of the two linears in float64 from the sinusoid the DEVICE produced: the bound of linear_ref applied twice, the
    first linear's error carried through the activation (slope <= LIP, libm allowance) and the second weight's magnitudes."""
    h, bh = linear_ref(pe_dev, o["w0"], o["b0"], None, 0, 0)
    w2 = o["w2"].double()
    a = act64(h, act)
    ea = bh if act == 0 else LIP * bh                                       # |act64(h_dev) - act64(h_ref)|
    if act not in INT_ACTS:
        ea = ea + _ulps(act_ulps, act, 0) * 2 * U * (act_mag64(h, act) + 2 * bh)
    emb = a @ w2.T + o["b2"].double()
    S = a.abs() @ w2.abs().T + o["b2"].double().abs()
    if cond is not None:
        emb, S = emb + cond.double(), S + cond.double().abs()
    n = math.ceil(h.shape[1] / 64) + 8
    return emb, ea @ w2.abs().T + n * U * (S + ea @ w2.abs().T)


# ----------------------------------------------------------------------------- rho_multi_embed / rho_multi_embed_bwd
ME_NKEYS = (1, 2, 16)                                   # 16: the kernel's limit (cat[16])
ME_DIM = (1, 255, 256, 257, 600)                        # 256 threads stride dim
ME_B = (1, 7, 64)
ME_LIST_LEN = (1, 2, 3, 5, 8, 13, 71)


def _me_cases():
    out = []
    for ink, nkeys in enumerate(ME_NKEYS):
        for idd, dim in enumerate(ME_DIM):
            j = ink * len(ME_DIM) + idd
            B = ME_B[(ink + idd) % 3]
            lens = [ME_LIST_LEN[(j + 3 * i) % 7] for i in range(nkeys)]
            out.append(dict(name=f"k{nkeys}_d{dim}_B{B}_n{lens[0]}", nkeys=nkeys, dim=dim, B=B, lens=lens, dropped=()))
    # all 64 samples on the one row of each key (maximal contention); samples dropped as rho_cond_drop writes them (idx = -1 in all keys)
    out.append(dict(name="k2_d257_B64_one_row", nkeys=2, dim=257, B=64, lens=[1, 1], dropped=()))
    out.append(dict(name="k2_d256_B7_dropped", nkeys=2, dim=256, B=7, lens=[3, 5], dropped=(0, 3, 6)))
    out.append(dict(name="k16_d600_B64_dropped", nkeys=16, dim=600, B=64, lens=[2, 71] * 8, dropped=tuple(range(1, 64, 5))))
    out.append(dict(name="k1_d1_B64_n71", nkeys=1, dim=1, B=64, lens=[71], dropped=()))
    return out


ME_CASES = _me_cases()


def me_operands(c, integer: bool) -> dict:
    """space: per key, distinct float32 values (with 0.0, negatives, non-integers); idx [B, nkeys] the categories the labels y name;
    tables real-valued (forward) or integer-valued (the prefill of the backward); demb integer or real."""
    nkeys, dim, B, n = c["nkeys"], c["dim"], c["B"], "me_" + c["name"]
    space = [(torch.arange(L, dtype=torch.float32) - (L // 2)) * (0.25 * (i + 1)) for i, L in enumerate(c["lens"])]
    idx = torch.stack([(det_normal((B,), f"{n}i{i}").mul(997.0).abs().floor().long() % L) for i, L in enumerate(c["lens"])], 1)
    y = torch.stack([space[i][idx[:, i]] for i in range(nkeys)], 1).contiguous()
    if integer:
        tables = [int_tensor((L, dim), f"{n}T{i}", 24.0, 64) for i, L in enumerate(c["lens"])]
        demb = int_tensor((B, dim), n + "g", 24.0, 64)
    else:
        tables = [det_normal((L, dim), f"{n}t{i}") for i, L in enumerate(c["lens"])]
        demb = det_normal((B, dim), n + "r")
    idx = idx.to(torch.int32)
    for b in c["dropped"]:
        idx[b, :] = -1
    return dict(space=space, y=y, idx=idx, tables=tables, demb=demb)


def me_lookup(y: torch.Tensor, space) -> torch.Tensor:
    """int32 [B, nkeys]: per key the FIRST position whose value equals the label (IEEE equality: -0.0 == 0.0, NaN equals nothing),
    -1 where there is none.  y [B, nkeys], or [B] (one label for all keys)."""
    B, nkeys = y.shape[0], len(space)
    idx = np.full((B, nkeys), -1, dtype=np.int32)
    for b in range(B):
        for i in range(nkeys):
            v = np.float32(y[b] if y.dim() == 1 else y[b, i])
            for q, s in enumerate(space[i].numpy()):
                if np.float32(s) == v:
                    idx[b, i] = q
                    break
    return torch.from_numpy(idx)


def me_forward_ref(idx: torch.Tensor, tables, dim: int) -> torch.Tensor:
    """float32 [B, dim]: e_0, then += e_i in key order, float32 adds (exact by construction: the kernel does these very adds);
    a key with idx -1 contributes nothing, a sample with none is the zero row."""
    B, nkeys = idx.shape
    out = np.zeros((B, dim), dtype=np.float32)
    for b in range(B):
        first = True
        for i in range(nkeys):
            j = int(idx[b, i])
            if j < 0:
                continue
            e = tables[i][j].numpy().astype(np.float32)
            out[b] = e if first else (out[b] + e).astype(np.float32)
            first = False
    return torch.from_numpy(out)


def me_backward_ref(idx: torch.Tensor, demb: torch.Tensor, pre):
    """(ordered, exact, mag) per key: the float32 running sum onto `pre` in batch order (what the ordered kernel computes, bit for
    bit), the same sum in float64, and the sum of the terms' magnitudes (for the atomic kernel's bound B * 2^-24 * mag)."""
    B, nkeys = idx.shape
    g32 = demb.numpy().astype(np.float32)
    ordered = [p.numpy().astype(np.float32).copy() for p in pre]
    exact = [p.numpy().astype(np.float64).copy() for p in pre]
    mag = [np.abs(p.numpy().astype(np.float64)) for p in pre]
    for b in range(B):
        for i in range(nkeys):
            j = int(idx[b, i])
            if j < 0:
                continue
            ordered[i][j] = (ordered[i][j] + g32[b]).astype(np.float32)
            exact[i][j] += g32[b].astype(np.float64)
            mag[i][j] += np.abs(g32[b].astype(np.float64))
    return [torch.from_numpy(a) for a in ordered], [torch.from_numpy(a) for a in exact], [torch.from_numpy(a) for a in mag]

