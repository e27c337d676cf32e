"""Deterministic rho_conv_desc values for the host-side dispatch table (tests/golden/conv_dispatch.json).

The descriptors are built directly as hip.ConvDesc with fake, 16-byte-aligned, non-null addresses: the variant, statistics-tile and
workspace queries of the library read the descriptor and never what it points to, so neither tensors nor a GPU are needed.
tests/golden/make_dispatch_table.py recorded the answers of one build once; tests/test_conv_dispatch_host.py runs this file as a
fresh process (python dispatch_cases.py prints the table as JSON) and compares.

Three layers, each a filtered cross product:
  A  every tap shape / stride / phase mode x every geometry x both dtypes, with three (cin, cout) combinations that rotate through
     the whole channel list as the mode and geometry change;
  B  the plain modes x every geometry x both dtypes x the channel widths the pinned kernel names of the GPU tests need;
  C  every attachment (prologue, statistics, residuals, folded skip, GroupNorm backward, workspace), attached where it is legal and
     where it is not, on a small set of base descriptors.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, BF16 = 0, 1                       # RHO_F32 / RHO_BF16
E_ARG, E_ALIGN, E_SHAPE = -1, -2, -3   # RHO_E_*

GEOMS = [
    (2, 4, 8, 8), (1, 8, 16, 16), (2, 5, 9, 12), (1, 16, 32, 32), (1, 8, 64, 64),      # 3-D
    (2, 1, 16, 16), (64, 1, 4, 4), (2, 1, 9, 12), (8, 1, 32, 32),                      # 2-D
    (4, 1, 1, 256), (3, 1, 1, 100),                                                    # 1-D
    (2, 1024, 1024, 1024),                                                             # 2^31 positions
]

# (c1, c2); (48, 0) is an alignment error for bf16 (32-channel chunks)
CINS = [(32, 0), (64, 0), (64, 64), (128, 64), (512, 0), (48, 0)]

# (cout, coutp, split, y2): y2 = None (whole output channels-last), "cm" / "cm_f32" (channel-major), "cl" (channels-last)
COUTS = [(c, c, c, None) for c in (32, 64, 96, 128, 192, 512, 1536)] + [
    (64, 64, 0, "cm"), (96, 96, 0, "cm_f32"), (40, 64, 0, "cm"), (100, 128, 0, "cm"),           # split = 0, padded coutp
    (128, 128, 64, "cm"), (128, 128, 64, "cl"), (96, 96, 32, "cl"), (192, 192, 128, "cl"),      # mixed
    (96, 128, 32, "cl"), (96, 128, 32, "cm"), (70, 96, 32, "cl"),                               # ... padded: legal, E_ARG, E_ALIGN
    (64, 96, 64, None),                                                                         # channels-last rows are not padded
]


def _mode(kernel, **kw):
    return dict(kd=kernel[0], kh=kernel[1], kw=kernel[2], **kw)


def _modes():
    m = []
    for k in ((3, 3, 3), (1, 3, 3)):
        m += [_mode(k), _mode(k, sh=2, sw=2), _mode(k, up_h=1, up_w=1), _mode(k, zs_h=1, zs_w=1)]
    m += [_mode((1, 1, 3)), _mode((1, 1, 3), sw=2), _mode((1, 1, 3), up_w=1), _mode((1, 1, 3), zs_w=1)]
    m += [_mode((1, 1, 1)), _mode((1, 1, 1), sh=2, sw=2)]                                       # (a strided 1x1x1 is refused)
    # sub-pixel phases of a conv behind a nearest x2 upsample (ph_*), parity split of a stride-2 conv (phd_*)
    m += [_mode((3, 2, 2), ph_h=a, ph_w=b) for a in (1, 2) for b in (1, 2)]
    m += [_mode((1, 2, 2), ph_h=1, ph_w=1), _mode((1, 2, 2), ph_h=2, ph_w=2), _mode((1, 1, 2), ph_w=1), _mode((1, 1, 2), ph_w=2)]
    m += [_mode((3, 1, 1), phd_h=1, phd_w=1), _mode((3, 1, 2), phd_h=1, phd_w=2), _mode((3, 2, 1), phd_h=2, phd_w=1),
          _mode((3, 2, 2), phd_h=2, phd_w=2), _mode((1, 2, 2), phd_h=2, phd_w=2), _mode((1, 1, 2), phd_w=2)]
    # the same tap shapes without the phase values they need, and shapes no kernel has
    m += [_mode((3, 2, 2)), _mode((1, 1, 2)), _mode((3, 1, 1)), _mode((3, 3, 2), ph_w=1), _mode((2, 3, 3))]
    return m


MODES = _modes()
PLAIN = [_mode((3, 3, 3)), _mode((3, 3, 3), sh=2, sw=2), _mode((1, 3, 3)), _mode((1, 1, 3)), _mode((1, 1, 1))]

_PTR_FIELDS = None


def addr(field):
    """A fake address for pointer field `field`: distinct per field, 16-byte aligned, non-null, never dereferenced."""
    global _PTR_FIELDS
    if _PTR_FIELDS is None:
        from rho_diffusion_amd.hip import ConvDesc
        _PTR_FIELDS = [n for n, t in ConvDesc._fields_ if t is C.c_void_p]
    return 0x7E0000100000 + 0x10000 * _PTR_FIELDS.index(field)


def base(dtype, mode, geom, cin, co):
    n, d, h, w = geom
    f = dict(dtype=dtype, n=n, d=d, h=h, w_=w, sh=1, sw=1)
    f.update(mode)
    if f.get("zs_h"):
        f["out_h"] = 2 * h
    if f.get("zs_w"):
        f["out_w"] = 2 * w
        f.setdefault("out_h", h)              # (zero-stuffed launches pass both extents)
    c1, c2 = cin
    cout, coutp, split, y2 = co
    f.update(c1=c1, x1=addr("x1"), w=addr("w"), bias=addr("bias"), cout=cout, coutp=coutp, split=split)
    if c2:
        f.update(c2=c2, x2=addr("x2"))
    if split > 0:
        f["y"] = addr("y")
    if split < cout:
        f["y2"] = addr("y2")
        f["y2_cl"] = int(y2 == "cl")
        f["y2_f32"] = int(y2 == "cm_f32")
    return f


def _attachments(f):
    """[(tag, fields)]: `f` with each attachment, in its legal form and in an illegal one."""
    ck = 32 if f["dtype"] == BF16 else 16
    gnb = dict(gnb_x1=addr("gnb_x1"), gnb_a=addr("gnb_a"), gnb_b=addr("gnb_b"))
    gna = dict(gna_g=addr("gna_g"), gna_cA=addr("gna_cA"), gna_cP=addr("gna_cP"), gna_cQ=addr("gna_cQ"), gnb_c1=f["cout"], **gnb)
    sk = dict(sk_x1=addr("sk_x1"), sk_w=addr("sk_w"), sk_bias=addr("sk_bias"), sk_c1=64)
    out = [
        ("pre", dict(pre_a=addr("pre_a"), pre_b=addr("pre_b"), pre_silu=1)),
        ("pre_a_only", dict(pre_a=addr("pre_a"))),
        ("stats", dict(stats=addr("stats"))),
        ("res", dict(res=addr("res"), res_add=addr("res_add"), res_add_stride=f["cout"])),
        ("res2", dict(res2=addr("res2"))),
        ("skip", sk),
        ("skip2", dict(sk, sk_x2=addr("sk_x2"), sk_c2=2 * ck)),
        ("skip_bad", dict(sk, sk_c1=ck + 8)),
        ("gnb", dict(gnb, stats=addr("stats"), gnb_c1=max(f["split"], 32), gnb_silu=1)),
        ("gnb_no_stats", dict(gnb, gnb_c1=max(f["split"], 32))),
        ("gna", gna),
        ("gna_res", dict(gna, res=addr("res"))),
        ("ws", dict(ws=addr("ws"), ws_bytes=1 << 32)),
        ("ws_small", dict(ws=addr("ws"), ws_bytes=4096)),
        ("ws_stats", dict(ws=addr("ws"), ws_bytes=1 << 32, stats=addr("stats"))),
    ]
    return [(tag, dict(f, **extra)) for tag, extra in out]


def cases():
    """The descriptors, as dicts of the non-zero rho_conv_desc fields, in the order of the table."""
    out = []
    combos = [(ci, co) for ci in CINS for co in COUTS]
    for di, dtype in enumerate((F32, BF16)):                                                   # layer A
        for mi, mode in enumerate(MODES):
            for gi, geom in enumerate(GEOMS):
                for j in range(3):
                    ci, co = combos[(7 * mi + 13 * gi + 5 * di + 29 * j) % len(combos)]
                    out.append(base(dtype, mode, geom, ci, co))
    for dtype in (F32, BF16):                                                                  # layer B
        for mode in PLAIN:
            for geom in GEOMS:
                for ci in ((32, 0), (64, 64)):
                    for c in (32, 64, 128):
                        out.append(base(dtype, mode, geom, ci, (c, c, c, None)))
    att_modes = PLAIN + [_mode((3, 2, 2), ph_h=1, ph_w=1), _mode((3, 1, 1), phd_h=1, phd_w=1)]
    att_geoms = [(2, 4, 8, 8), (2, 5, 9, 12), (4, 1, 1, 256)]
    for dtype in (F32, BF16):                                                                  # layer C
        for mode in att_modes:
            for geom in att_geoms:
                for ci, co in (((64, 0), (128, 128, 128, None)), ((64, 64), (64, 64, 64, None)), ((128, 64), (128, 128, 64, "cl"))):
                    out += [f for _, f in _attachments(base(dtype, mode, geom, ci, co))]
    return out


def make_desc(fields):
    from rho_diffusion_amd.hip import ConvDesc
    d = ConvDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def show(fields):
    """A descriptor on one line (pointer fields as 'set')."""
    return " ".join(f"{k}={'set' if k in _PTR_FIELDS else v}" for k, v in fields.items())


def query(lib, fields):
    """[variant rc, variant text, statistics tiles, workspace bytes, then (rc, text) of the wgrad variant for dy_width = coutp and
    coutp + one 16-byte piece]."""
    d = make_desc(fields)
    buf = C.create_string_buffer(128)
    rc = lib.rho_conv_variant(C.byref(d), buf, 128)
    row = [rc, buf.value.decode(), int(lib.rho_conv_stats_tiles(C.byref(d))), int(lib.rho_conv_workspace_bytes(C.byref(d)))]
    piece = 8 if fields["dtype"] == BF16 else 4
    for dyw in (fields["coutp"], fields["coutp"] + piece):
        rc = lib.rho_conv_wgrad_variant(C.byref(d), dyw, buf, 128)
        row += [rc, buf.value.decode()]
    return row


def run(lib_path=None):
    """{"names": [...], "rows": [...]}: one row per descriptor in cases() order, texts replaced by their index in names."""
    from rho_diffusion_amd import hip
    lib = hip.load(lib_path) if lib_path else hip.load()
    names, index, rows = [], {}, []
    for f in cases():
        row = query(lib, f)
        for i in (1, 5, 7):
            if row[i] not in index:
                index[row[i]] = len(names)
                names.append(row[i])
            row[i] = index[row[i]]
        rows.append(row)
    return {"names": names, "rows": rows}


if __name__ == "__main__":
    json.dump(run(sys.argv[1] if len(sys.argv) > 1 else None), sys.stdout, separators=(",", ":"))
