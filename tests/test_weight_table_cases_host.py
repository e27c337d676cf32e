"""CPU: the references of weight_table_cases.py are tied to convolution identities (so that none of them is a transcription of the
kernel it judges), every reference value is an integer its stored format holds exactly, the case tables reach every branch the
issue of the GPU tests names, and ops.WfinTable lays its records out by the documented formula."""
import math

import pytest
import torch
import torch.nn.functional as F

import weight_table_cases as X
from exact_util import assert_bit_equal, check_bf16_exact, check_f32_exact, int_tensor

DTYPES = ["bf16", "f32"]


def _names(cases):
    return [c["name"] for c in cases]


def _pads(k):
    return tuple(v // 2 for v in k)


# ============================================================================================ the references against convolutions
@pytest.mark.parametrize("shape", [(5, 6, 3), (5, 6, 3, 3), (5, 6, 3, 3, 3), (5, 6, 1, 1, 1)], ids=["t3", "t9", "t27", "t1"])
def test_fwd_and_dgrad_references_are_the_conv_and_its_autograd(shape):
    w = int_tensor(shape, "wth_w", 2.0, 4).double()
    k = X.k3(shape)
    w5 = w.reshape(5, 6, *k)
    x = int_tensor((2, 6, 3, 4, 5), "wth_x", 1.0, 2).double().requires_grad_(True)
    y = F.conv3d(x, w5, None, padding=_pads(k))
    wf = X.conv_weight_of(X.ref_fwd(w, k, 32, 16), 5, 6, k)
    assert_bit_equal(wf, w5, "forward layout read back")
    dy = int_tensor(tuple(y.shape), "wth_dy", 1.0, 2).double()
    y.backward(dy)
    wd = X.conv_weight_of(X.ref_dgrad(w, k, 32, 16), 6, 5, k)             # rows = input channels: a conv from cout to cin channels
    assert_bit_equal(F.conv3d(dy, wd, None, padding=_pads(k)), x.grad, "forward conv of dY with the dgrad layout vs autograd")


def test_row_and_col_src_permute_the_output_channels():
    """A conv with the permuted layout gives the permuted output channels (zero where the source is outside the parameter), and the
    data gradient with col_src takes dY in that permuted order."""
    w = int_tensor((40, 6, 3), "wth_pw", 2.0, 4).double()
    k = (1, 1, 3)
    rs = X.holes_row_src(64, 40)
    assert sorted(int(v) for v in rs if 0 <= v < 40) == sorted(set(int(v) for v in rs if 0 <= v < 40))           # injective
    assert (rs == -1).any() and (rs == 40).any() and (rs > 40).any()
    x = int_tensor((1, 6, 1, 1, 9), "wth_px", 1.0, 2).double().requires_grad_(True)
    y = F.conv3d(x, w.reshape(40, 6, 1, 1, 3), None, padding=(0, 0, 1))
    yp = F.conv3d(x, X.conv_weight_of(X.ref_fwd(w, k, 64, 16, rs), 64, 6, k), None, padding=(0, 0, 1))
    for r in range(64):
        s = int(rs[r])
        assert_bit_equal(yp[:, r], y[:, s] if 0 <= s < 40 else torch.zeros_like(y[:, 0]), f"row {r}")
    dyp = int_tensor((1, 48, 1, 1, 9), "wth_pdy", 1.0, 2).double()
    dy = torch.zeros_like(y)
    for col in range(40):
        if 0 <= int(rs[col]) < 40:
            dy[:, int(rs[col])] = dyp[:, col]
    y.backward(dy)
    wd = X.conv_weight_of(X.ref_dgrad(w, k, 32, 48, rs), 6, 48, k)
    assert_bit_equal(F.conv3d(dyp, wd, None, padding=(0, 0, 1)), x.grad, "dgrad with col_src")
    q = X.qkv_row_src(32, 2)
    assert sorted(q.tolist()) == list(range(96)) and q[:4].tolist() == [0, 1, 2, 3] and q[16:18].tolist() == [48, 49] and int(q[32]) == 16


@pytest.mark.parametrize("kshape,phases", [((3, 3, 3), [(1, 1), (1, 2), (2, 1), (2, 2)]), ((1, 3, 3), [(0, 1), (0, 2)]), ((3, 3, 3), [(1, 0), (2, 0)])],
                         ids=["333_hw", "133_w", "333_h"])
def test_phase_reference_is_the_conv_of_the_upsampled_input(kshape, phases):
    """conv(upsample2x(x), w) interleaves conv(x, w_phase): parity 0 (phase code 1) reads x[i - 1], x[i]; parity 1 (code 2) x[i], x[i + 1]."""
    w5 = int_tensor((5, 6) + kshape, "wth_phw", 2.0, 4).double()
    x = int_tensor((2, 6, 3, 4, 5), "wth_phx", 1.0, 2).double()
    up = (bool(phases[0][0]), bool(phases[0][1]))
    xu = x
    if up[0]:
        xu = xu.repeat_interleave(2, 3)
    if up[1]:
        xu = xu.repeat_interleave(2, 4)
    full = F.conv3d(xu, w5, None, padding=_pads(kshape))
    for ph in phases:
        lay = X.ref_phase(w5, ph, 32, 16, False)
        k2 = (kshape[0], 2 if ph[0] else kshape[1], 2 if ph[1] else kshape[2])
        assert lay.shape[0] == math.prod(k2)
        wp = X.conv_weight_of(lay, 5, 6, k2)
        pad_w = {0: (kshape[2] // 2,) * 2, 1: (1, 0), 2: (0, 1)}[ph[1]]
        pad_h = {0: (kshape[1] // 2,) * 2, 1: (1, 0), 2: (0, 1)}[ph[0]]
        yp = F.conv3d(F.pad(x, pad_w + pad_h + (kshape[0] // 2,) * 2), wp, None)
        sl_h = slice(ph[0] - 1, None, 2) if ph[0] else slice(None)
        sl_w = slice(ph[1] - 1, None, 2) if ph[1] else slice(None)
        assert_bit_equal(yp, full[:, :, :, sl_h, sl_w], f"phase {ph}")
        # its data-gradient layout: the same phase conv's autograd (a forward conv of dY with the flipped, transposed taps)
        xr = x.clone().requires_grad_(True)
        dy = int_tensor(tuple(yp.shape), "wth_phdy", 1.0, 2).double()
        F.conv3d(F.pad(xr, pad_w + pad_h + (kshape[0] // 2,) * 2), wp, None).backward(dy)
        wd = X.conv_weight_of(X.ref_phase(w5, ph, 32, 16, True), 6, 5, k2)
        rev = lambda p: (p[1], p[0])                                                           # noqa: E731  (the transposed conv pads the other side)
        dx = F.conv3d(F.pad(dy, rev(pad_w) + rev(pad_h) + (kshape[0] // 2,) * 2), wd, None)
        assert_bit_equal(dx, xr.grad, f"phase {ph} dgrad")


def test_sel_reference_is_the_parity_split_of_the_stride_2_conv():
    """y = conv(x, w, stride (1, 2, 2), padding 1) is the sum over the four input parities of a stride-1 conv with the selected taps
    (S2_FWD), and dX's parity (a, b) is a stride-1 conv of dY with the S2_BWD taps, D mirrored, channels transposed."""
    from rho_diffusion_amd.engine.weights import _ConvW
    assert X.S2_FWD == _ConvW.S2_FWD and X.S2_BWD == _ConvW.S2_BWD
    w5 = int_tensor((5, 6, 3, 3, 3), "wth_sw", 2.0, 4).double()
    x = int_tensor((2, 6, 3, 8, 6), "wth_sx", 1.0, 2).double().requires_grad_(True)
    y = F.conv3d(x, w5, None, stride=(1, 2, 2), padding=1)
    acc = torch.zeros_like(y)
    lead = {0: (0, 0), 1: (1, 0)}                                    # odd input rows: taps (0, 2) read x_odd[i - 1], x_odd[i]
    for a in (0, 1):
        for b in (0, 1):
            sel = (X.S2_FWD[a], X.S2_FWD[b])
            k2 = (3, len(sel[0]), len(sel[1]))
            wp = X.conv_weight_of(X.ref_sel(w5, sel, False, False, 32, 16), 5, 6, k2)
            acc += F.conv3d(F.pad(x.detach()[:, :, :, a::2, b::2], lead[b] + lead[a] + (1, 1)), wp, None)
    assert_bit_equal(acc, y, "sum of the parity convs")
    dy = int_tensor(tuple(y.shape), "wth_sdy", 1.0, 2).double()
    y.backward(dy)
    trail = {0: (0, 0), 1: (0, 1)}                                   # odd rows of dX: taps (2, 0) read dY[j], dY[j + 1]
    for a in (0, 1):
        for b in (0, 1):
            sel = (X.S2_BWD[a], X.S2_BWD[b])
            k2 = (3, len(sel[0]), len(sel[1]))
            wd = X.conv_weight_of(X.ref_sel(w5, sel, True, True, 32, 16), 6, 5, k2)
            dx = F.conv3d(F.pad(dy, trail[b] + trail[a] + (1, 1)), wd, None)
            assert_bit_equal(dx, x.grad[:, :, :, a::2, b::2], f"dX parity {(a, b)}")


def test_vec_reference_and_the_head_gathers():
    src = torch.arange(1.0, 11.0)
    assert X.ref_vec(src, 12).tolist() == list(range(1, 11)) + [0, 0]
    assert X.ref_vec(src, 6, torch.tensor([3, -1, 10, 0, 9, 2]), n=5).tolist() == [4, 0, 0, 1, 10, 0]
    w = int_tensor((1, 32, 3, 3, 3), "wth_hw", 2.0, 4)
    assert_bit_equal(X.ref_vec(w, 1024, X.head_as_gemm_perm(32, 32), 1024).reshape(1, 32, 32), X.head_weight_layout(w), "_HeadAsGemm gather")
    hd = X.ref_vec(w, 1024, X.head_dgrad_perm(32), 1024).reshape(32, 32)
    assert_bit_equal(hd[:, :27], w[0].reshape(32, 27).flip(1), "_HeadDgradW gather: mirrored taps")
    assert float(hd[:, 27:].abs().max()) == 0.0


# ============================================================================================ B: the prep table's cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_case_references_are_exactly_representable(dtype):
    for c in X.PREP_CASES:
        io = X.prep_io(c["name"], dtype)
        assert tuple(io["ref"].shape) == tuple(io["out_shape"]), c["name"]
        check_bf16_exact(io["ref"], c["name"])                          # (holds for the fp32 outputs too: they are copies and short sums)
        check_bf16_exact(io["w"], c["name"] + " w")
        assert float(io["ref"].abs().max()) > 0, c["name"]
    ph = X.prep_io("phase_333_11", dtype)
    assert float(ph["ref"].abs().max()) > X.W_CLAMP                       # a phase tap that really sums several source taps


def test_prep_cases_cover_every_kind_and_branch():
    from rho_diffusion_amd import hip
    kinds = {getattr(hip, n) for n in dir(hip) if n.startswith("PREP_")}
    assert kinds == {X.KIND_CODE[c["kind"]] for c in X.PREP_CASES} and len(kinds) == 5
    assert len(X.PREP_CASES) >= 20 and len(set(_names(X.PREP_CASES))) == len(X.PREP_CASES)
    for dtype in DTYPES:
        geo = {c["name"]: X.prep_geometry(X.prep_io(c["name"], dtype)) for c in X.PREP_CASES}
        lds = [g for g in geo.values() if g["lds"]]
        assert any(g["nblk"] > g["units"] for g in lds) and any(g["nblk"] < g["units"] for g in lds)
        for kind in ("fwd", "dgrad"):
            taps = {math.prod(X.prep_io(c["name"], dtype)["k"]) for c in X.PREP_CASES if c["kind"] == kind}
            assert {1, 3, 9, 27, 32, 36} <= taps, (kind, taps)
            assert any(c["kind"] == kind and c.get("perm") == p and geo[c["name"]]["lds"] == lds_ for c in X.PREP_CASES
                       for p in ("qkv", "holes") for lds_ in (True, False))
        # under a cap of 3 blocks every op but the smallest takes several trips of its walk
        for c in X.PREP_CASES:
            g = X.prep_geometry(X.prep_io(c["name"], dtype), max_blocks=3)
            if g["total"] > 3 * 1024:
                assert (g["units"] > g["nblk"]) if g["lds"] else (g["total"] > g["nblk"] * 256), c["name"]
        fw = X.prep_io("fwd_t3", dtype)
        assert fw["out_shape"][1] == 64 > 40 and fw["out_shape"][2] > 72 and fw["out_shape"][2] % 64 != 0          # padded rows, ragged group
    assert X.prep_geometry(X.prep_io(X.PREP_ONE_OP, "bf16"))["lds"]


# ============================================================================================ C: the finalize table's cases
def test_wfin_references_are_exact_and_transpose_the_prep_layouts():
    io = X.wfin_io(tuple(_names(X.WFIN_CASES)))
    check_f32_exact(io["arena"], "arena")
    for op in io["ops"]:
        c = op["case"]
        check_f32_exact(op["ref"], c["name"])
        assert not torch.equal(op["ref"], op["grad0"]), c["name"]
        region = io["arena"][op["off"]:op["off"] + X.wfin_region_floats(c)].double()
        delta = X.ref_wfin(c, region, torch.zeros_like(op["grad0"]).double(), op["rs"])
        w = int_tensor(tuple(op["grad0"].shape), "wth_adj" + c["name"], 2.0, 4).double()
        if c["kind"] == 0 and not c.get("off_extra"):
            # <prep(w), dw> = <w, finalize(dw)>: the finalize is the transpose of the forward layout (row table included)
            rs = None if op["rs"] is None else torch.cat([op["rs"], torch.full((c["coutp"] - c["cout"],), -1, dtype=torch.int32)])
            lay = X.ref_fwd(w, c["k"], c["coutp"], c["cinb"], rs)
            assert float((lay * region[:lay.numel()].view_as(lay)).sum()) == float((w * delta).sum()), c["name"]
        elif c["kind"] == 1:
            tot = 0.0
            for p, ph in enumerate(X.wfin_phases(c["up"])):
                lay = X.ref_phase(w.reshape(c["cout"], c["cin"], *c["k"]), ph, c["coutp"], c["cinb"], False)
                tot += float((lay * region[p * X.wfin_stride(c):][:lay.numel()].view_as(lay)).sum())
            assert tot == float((w * delta).sum()), c["name"]
            assert X.wfin_stride(c) > X.wfin_buffer_floats(c)
        elif c["kind"] == 2:
            # the head's rows are taps of the im2col of dpred, mirrored: row r carries the gradient of tap 26 - r; rows 27 .. 31 unread
            assert_bit_equal(delta[0].reshape(c["cin"], 27), region.view(32, c["cin"])[:27].flip(0).t(), c["name"])
            assert float(region.view(32, c["cin"])[27:].abs().min()) > 0


def test_wfin_cases_cover_every_kind_and_branch():
    kinds = {c["kind"] for c in X.WFIN_CASES}
    assert kinds == {0, 1, 2} and len(X.WFIN_CASES) >= 12
    taps0 = {math.prod(c["k"]) for c in X.WFIN_CASES if c["kind"] == 0}
    assert {1, 3, 27, 32, 36} <= taps0
    assert any(1 < t <= 32 for t in taps0) and any(t == 1 or t > 32 for t in taps0)                 # LDS and elementwise branches
    for lds in (True, False):
        assert {"qkv", "holes"} <= {c.get("rs") for c in X.WFIN_CASES if c["kind"] == 0 and (1 < math.prod(c["k"]) <= 32) == lds}
        assert any(c.get("nblk") == 1 and (1 < math.prod(c["k"]) <= 32) == lds for c in X.WFIN_CASES)
    assert {(c["up"], c["k"]) for c in X.WFIN_CASES if c["kind"] == 1} == {(u, k) for u in ((1, 1), (0, 1), (1, 0)) for k in ((3, 3, 3), (1, 3, 3))}
    assert {c["cin"] for c in X.WFIN_CASES if c["kind"] == 2} == {32, 64}
    assert any(c.get("off_extra") == 13 for c in X.WFIN_CASES)
    # the LDS walk both ways round: more blocks than units and fewer
    lds = [c for c in X.WFIN_CASES if c["kind"] == 0 and 1 < math.prod(c["k"]) <= 32]
    units = lambda c: c["cout"] * -(-c["cin"] // 64)                                                # noqa: E731
    nblk = lambda c: c.get("nblk") or X.wfin_nblk(c["cout"] * c["cin"] * math.prod(c["k"]))         # noqa: E731
    assert any(nblk(c) > units(c) for c in lds) and any(nblk(c) < units(c) for c in lds)


def test_wfin_table_lays_out_blocks_by_the_documented_formula():
    """ops.WfinTable (what BackwardBuilder.fin_close emits): total = cout * cin * taps, nblk = max(1, min(ceil(total / 256), 512)),
    blk0 ascending and contiguous from 0; the pointers are the arena base plus 4 bytes per float of offset."""
    from rho_diffusion_amd.engine import ops
    entries = [dict(kind=0, off=0, param="p0", rs=None, cout=40, cin=72, coutp=64, cinb=96, k=(3, 3, 3)),                 # 77760 -> 304
               dict(kind=0, off=64, param="p1", rs=0x5000, cout=40, cin=1, coutp=64, cinb=1, k=(1, 1, 1)),                  # 40 -> 1
               dict(kind=1, off=128, param="p2", rs=None, cout=128, cin=128, coutp=128, cinb=128, k=(3, 3, 3), up_h=1, up_w=1, stride=4096),   # cap 512
               dict(kind=2, off=192, param="p3", rs=None, cout=1, cin=32, coutp=32, cinb=32, k=(3, 3, 3)),                  # 864 -> 4
               dict(kind=0, off=256, param="p4", rs=None, cout=1, cin=1, coutp=1, cinb=1, k=(1, 1, 1)),                     # 1 -> 1
               dict(kind=0, off=320, param="p5", rs=None, cout=16, cin=16, coutp=32, cinb=16, k=(1, 1, 1))]                 # 256 -> 1
    t = ops.WfinTable("cpu")
    for e in entries:
        t.add(**e)
    t.add(kind=0, off=384, rs=None, cout=40, cin=72, coutp=64, cinb=96, k=(3, 3, 3), nblk=1)
    grads = [0x10000 * (i + 1) for i in range(7)]
    recs = t.records(0x1000, grads)
    blk = 0
    for r, e, g in zip(recs, entries + [dict(entries[0], off=384)], grads):
        total = e["cout"] * e["cin"] * math.prod(e["k"])
        assert r.total == total and r.blk0 == blk and r.dw == 0x1000 + 4 * e["off"] and r.grad == g
        assert (r.kind, r.kd, r.kh, r.kw, r.cout, r.cin, r.coutp, r.cinb) == (e["kind"],) + tuple(e["k"]) + (e["cout"], e["cin"], e["coutp"], e["cinb"])
        assert (r.up_h, r.up_w, r.phase_stride) == (e.get("up_h", 0), e.get("up_w", 0), e.get("stride", 0))
        if r is not recs[-1]:
            assert r.nblk == max(1, min(-(-total // 256), 512)) == X.wfin_nblk(total)
        blk += r.nblk
    assert [r.nblk for r in recs] == [304, 1, 512, 4, 1, 1, 1] and t._blocks == blk == 824
    assert recs[1].row_src == 0x5000 and recs[0].row_src is None
    with pytest.raises(Exception):
        t.records(0x1000, grads[:3])
    # the bytes of the table are those of the loop BackwardBuilder.fin_close ran before it used WfinTable
    from rho_diffusion_amd import hip
    raw, blk = [], 0
    for e, g in zip(entries, grads):
        op = hip.WfinOp()
        op.dw, op.grad, op.row_src = 0x1000 + 4 * e["off"], g, e["rs"]
        op.cout, op.cin, op.coutp, op.cinb = e["cout"], e["cin"], e["coutp"], e["cinb"]
        op.kd, op.kh, op.kw = e["k"]
        op.total = e["cout"] * e["cin"] * e["k"][0] * e["k"][1] * e["k"][2]
        op.kind, op.up_h, op.up_w, op.phase_stride = e["kind"], e.get("up_h", 0), e.get("up_w", 0), e.get("stride", 0)
        op.nblk = max(1, min((op.total + 255) // 256, 512))
        op.blk0 = blk
        blk += op.nblk
        raw.append(bytes(op))
    assert b"".join(raw) == b"".join(bytes(r) for r in recs[:-1])


# ============================================================================================ D: the one-channel ends
@pytest.mark.parametrize("cout", X.STEM_COUTS)
@pytest.mark.parametrize("shape", X.STEM_SHAPES, ids=str)
def test_stem_case_reference_is_exactly_representable(shape, cout):
    c = X.stem_case(shape, cout)
    check_bf16_exact(c["x"], "x"), check_bf16_exact(c["w"], "w")
    check_bf16_exact(c["y"], "y")
    check_f32_exact(c["stats"], "tile statistics")
    N, D, H, W = shape
    assert c["stats"].shape[1] == X.ends_tiles(D, H, W)
    assert_bit_equal(c["stats"][:, :, 0].sum(1), c["y"].sum((2, 3, 4)), "tile rows partition the sample")
    assert_bit_equal(F.conv3d(c["x"], c["w"], c["b"], padding=1), c["y"], "fp32 vs fp64 on the CPU")
    assert_bit_equal(X.stem_weight_layout(c["w"])[0, :, :27], c["w"].reshape(cout, 27), "im2col form")


def test_ends_shapes_reach_the_edges():
    assert [X.ends_tiles(*s[1:]) for s in X.STEM_SHAPES] == [1, 1, 8, 2]
    N, D, H, W = X.RAGGED
    assert D % X.TD and H % X.TH and W % X.TW and N > 1


@pytest.mark.parametrize("C", X.HEAD_DGRAD_CS)
def test_head_dgrad_case_is_exactly_representable_and_mirrors_the_taps(C):
    c = X.head_dgrad_case(C)
    check_bf16_exact(c["dact"], "dact"), check_bf16_exact(c["w"], "w"), check_bf16_exact(c["dpred"], "dpred")
    # the stem kernel run on dpred with mirrored taps: y[c] = sum_tap w[0][c][26 - tap] dpred[p + off(tap)]
    wm = c["w"][0].reshape(C, 1, 27).flip(2).reshape(C, 1, 3, 3, 3).double()
    assert_bit_equal(F.conv3d(c["dpred"].double(), wm, None, padding=1), c["dact"], "mirrored-tap conv vs autograd")


@pytest.mark.parametrize("prologue", X.HEAD_PROLOGUES, ids=["raw", "affine"])
@pytest.mark.parametrize("C", X.HEAD_CS)
@pytest.mark.parametrize("shape", X.HEAD_SHAPES, ids=str)
def test_head_case_partials_stay_within_bf16(shape, C, prologue):
    c = X.head_case(C, shape, prologue)
    check_bf16_exact(c["x"], "x"), check_bf16_exact(c["w"], "w"), check_bf16_exact(c["act"], "activated input")
    check_bf16_exact(c["T"], "per-tap partials T[q][tap]")                # the kernel stores them as bf16
    check_f32_exact(c["out"], "out")
    if prologue:
        assert set(c["pre_a"].unique().tolist()) <= {1.0, 2.0, -1.0} and float(c["pre_b"].abs().min()) >= 1
        # a kernel that padded BEFORE activating would read pre_b, not zero, outside the volume: the reference differs there
        N, D, H, W = shape
        xp = F.pad(c["x"].double(), (1,) * 6)
        wrong = F.conv3d(c["pre_a"].double().view(N, C, 1, 1, 1) * xp + c["pre_b"].double().view(N, C, 1, 1, 1), c["w"].double(), None)
        assert not torch.equal(wrong, c["out_nobias"])
    N, D, H, W = shape
    sh = torch.zeros_like(c["out_nobias"])
    Tp = F.pad(c["T"], (1,) * 6)
    for tap in range(27):
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        sh[:, 0] += Tp[:, tap, kd:kd + D, kh:kh + H, kw:kw + W]
    assert_bit_equal(sh, c["out_nobias"], "out = sum over taps of T read at the tap's offset")


def test_ends_cases_cover_every_dispatched_instance():
    """rho_stem_conv3d dispatches k_stem3d<NCT> for cout = 32 NCT, NCT in {1, 2}; rho_head_conv3d k_head3d<NKS> for C = 16 NKS, NKS in
    {2, 4, 6, 8} (csrc/ends.hip; every other width is refused, which test_gpu_ends.py checks on the library)."""
    assert {c // 32 for c in X.STEM_COUTS} == {1, 2} and {c // 32 for c in X.HEAD_DGRAD_CS} == {1, 2}
    assert {c // 16 for c in X.HEAD_CS} == {2, 4, 6, 8}
    assert set(X.HEAD_PROLOGUES) == {None, "affine"}


@pytest.mark.parametrize("C", X.HEAD_CS)
def test_head_silu_case_bound_terms(C):
    c = X.head_silu_case(C)
    assert float(c["v"].abs().max()) < X.V_CAP
    assert_bit_equal(c["x"].to(torch.bfloat16).float(), c["x"], "x is bf16"), assert_bit_equal(c["w"].to(torch.bfloat16).float(), c["w"], "w is bf16")
    b = X.head_silu_bound(c)
    assert b.shape == c["out"].shape and float(b.min()) > 0
    assert bool((c["mag_prod"] + 1e-12 >= c["mag_T"]).all())                 # |T| <= sum_c |w act|, tap by tap
    assert X.SILU_SLACK == 55 * 2.0 ** -15
    # the bound is a per-element one of a few 2^-9 of the output's scale: far below what one missing tap would change
    assert float(b.max()) < 0.05 * float(c["out"].abs().max())
