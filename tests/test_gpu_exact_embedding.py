"""-m gpu: the conditioning path element by element - rho_linear / rho_linear_bwd, rho_timestep_embed with its MLP, rho_multi_embed and
rho_multi_embed_bwd - against the plain float64 / float32-ordered references of tests/embed_cases.py (checked on the CPU by
test_embed_cases_host.py).  Integer operands must come out bit-equal in any summation order; real operands stay inside the derived
per-element bound n * 2^-24 * (sum of the terms' magnitudes) of embed_cases.py.  Every output and every buffer a launch accumulates
onto lies between guard bands; outputs that are written start as NaN, so an element no thread wrote fails.

Activation allowances (ACT_ULPS).  Codes 1, 3, 4, 5, 6 add the device libm's error.  Measured once on an MI355X as the worst
per-element error of rho_linear (act_in and act_out) and of rho_linear_bwd's dx (both modes) with identity weights, K = O = 64, on
embed_cases.code_inputs() (1024 values: 1.5 * det_normal and a grid over [-6, 6]) against the float64 activation, in fp32 ulps of the
activation's term magnitude (act_mag64 / dact_mag64: |act(x)| except where the kernel's expression cancels).  The allowance is twice
the measured worst, rounded up to an integer:

    code          forward measured   allowed      derivative measured   allowed
    1 SiLU        1.455              3            1.416                 3
    3 GELU (erf)  1.125              3            1.100                 3
    4 Tanh        0.774              2            0.681                 2
    5 Sigmoid     1.528              4            1.633                 4
    6 ELU(1)      0.718              2            0.632                 2

test_activation_code_forward / _backward assert these allowances on the very inputs they were measured on and print the figure they
meet; the real-operand cases of the tables carry them into their bounds (embed_cases.linear_ref / linear_bwd_ref / te_chain_ref)."""
import numpy as np
import pytest
import torch

import embed_cases as E
from detdata import det_normal
from exact_util import (GUARD, assert_bit_equal, assert_within_abs, assert_within_ulps, check_f32_exact, f32_ulp, guarded, guarded_copy,
                        guards_intact)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32

ACT_ULPS = E.ACT_ULPS          # code -> (forward, derivative) allowance in fp32 ulps of the term magnitude: see the module docstring


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


@pytest.fixture(scope="module")
def hip():
    from rho_diffusion_amd import hip as h
    h.load()
    return h


@pytest.fixture
def det_mode(ops):
    """Sets the library's reproducibility switch for one test and puts it back."""
    was = ops.deterministic()
    yield ops.set_deterministic
    ops.set_deterministic(was)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded_i32(shape, fill=-99):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), 12345, dtype=torch.int32, device=DEV)
    flat[GUARD:GUARD + n] = fill
    return flat, flat[GUARD:GUARD + n].view(*shape)


def guards_intact_i32(flat) -> bool:
    return bool((flat[:GUARD] == 12345).all()) and bool((flat[-GUARD:] == 12345).all())


def worst_ulps(got, want64, mag64) -> float:
    return float(((got.detach().cpu().double() - want64).abs() / f32_ulp(mag64)).max())


_ids = lambda c: c["name"]


# ----------------------------------------------------------------------------- rho_linear
@pytest.mark.parametrize("c", E.LINEAR_CASES, ids=_ids)
def test_linear_forward(ops, c):
    """Integer cases bit-equal, real cases inside the derived bound, element by element: in_dim at the template boundaries and below
    one wave, a partial last workgroup, batch 1, bias / add absent, every activation code on either side."""
    o = E.linear_operands(c)
    ref, bound = E.linear_ref(o["x"], o["w"], o["bias"], o["add"], c["act_in"], c["act_out"], ACT_ULPS)
    flat, out = guarded((c["B"], c["O"]), F32)
    ops.linear(dev(o["x"]), dev(o["w"]), dev(o["bias"]), dev(o["add"]), act_in=c["act_in"], act_out=c["act_out"], out=out)
    torch.cuda.synchronize()
    assert guards_intact(flat)
    if c["kind"] == "int":
        check_f32_exact(ref, c["name"])
        assert_bit_equal(out, ref, f"linear {c['name']}")
    else:
        assert_within_abs(out, ref, bound, f"linear {c['name']}")


@pytest.mark.parametrize("where", ["act_in", "act_out"])
@pytest.mark.parametrize("code", sorted(ACT_ULPS))
def test_activation_code_forward(ops, code, where):
    """w = I, K = O = 64: out = act(x) element for element (the products by 1 and the sums with 0 are exact)."""
    x = E.code_inputs()
    flat, out = guarded(tuple(x.shape), F32)
    ops.linear(dev(x), torch.eye(64, device=DEV), None, None, out=out, **{where: code})
    torch.cuda.synchronize()
    assert guards_intact(flat)
    want, mag = E.act64(x, code), E.act_mag64(x, code)
    print(f"measured: forward code {code} as {where}: worst {worst_ulps(out, want, mag):.3f} ulp (allowed {ACT_ULPS[code][0]})")
    assert_within_ulps(out, want, ACT_ULPS[code][0], f"act {E.ACT_NAMES[code]} as {where}", mag=mag)


def test_linear_refuses_in_dim_2049(ops, hip):
    flat, out = guarded((2, 3), F32)
    with pytest.raises(hip.RhoHipError):
        ops.linear(torch.zeros(2, 2049, device=DEV), torch.zeros(3, 2049, device=DEV), torch.zeros(3, device=DEV), out=out)
    torch.cuda.synchronize()
    assert guards_intact(flat) and bool(torch.isnan(out).all())


# ----------------------------------------------------------------------------- rho_linear_bwd
_BWD_SHAPES = lambda c: (("dw", (c["O"], c["K"]), c["acc_params"]), ("db", (c["O"],), c["acc_params"]), ("dx", (c["B"], c["K"]), c["acc_dx"]))


def _run_linear_bwd(ops, c, o):
    """One launch of the case: {name: cpu result or None when absent}.  A strided dout is a column slice of a wider NaN-filled tensor
    passed as a raw pointer; an absent output's buffer must come back untouched."""
    B, O = c["B"], c["O"]
    if c["stride"]:
        wide = torch.full((B, c["stride"]), float("nan"), device=DEV)
        wide[:, E.BWD_COL0:E.BWD_COL0 + O] = o["dout"].to(DEV)
        dout = wide.data_ptr() + 4 * E.BWD_COL0
    else:
        wide = dev(o["dout"])
        dout = wide
    bufs = {}
    for name, shape, acc in _BWD_SHAPES(c):
        bufs[name] = guarded_copy(o["pre"][name], F32) if acc else guarded(shape, F32)
    before = {name: v.clone() for name, (_, v) in bufs.items()}
    arg = {name: (None if c["absent"] == name else v) for name, (_, v) in bufs.items()}
    ops.linear_bwd(dout, dev(o["x"]), dev(o["w"]), arg["dw"], arg["db"], arg["dx"], act_in=c["act_in"], acc_params=c["acc_params"],
                   acc_dx=c["acc_dx"], dout_stride=c["stride"])
    torch.cuda.synchronize()
    for name, (flat, v) in bufs.items():
        assert guards_intact(flat), f"{name}: guard band written"
        if c["absent"] == name:
            assert same_bits(v, before[name]), f"{name} was not requested and has been written"
    return {name: (None if c["absent"] == name else v.cpu()) for name, (_, v) in bufs.items()}


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("c", E.LINEAR_BWD_CASES, ids=_ids)
def test_linear_backward(ops, det_mode, c, det):
    """dw, db and dx, each absent in turn (db is computed when dw is not requested, as include/rho_hip.h states), written or
    accumulated onto integers, from a contiguous dout or a column slice, through the atomic 64-wide slices of k_linear_bwd_x and
    through the ordered k_linear_bwd_x_det: integer cases bit-equal in both, real cases inside the bound; the ordered mode twice
    gives the same bits."""
    det_mode(det)
    o = E.linear_bwd_operands(c)
    p = o["pre"]
    ref = E.linear_bwd_ref(o["dout"], o["x"], o["w"], c["act_in"], p["dw"] if c["acc_params"] else None,
                           p["db"] if c["acc_params"] else None, p["dx"] if c["acc_dx"] else None, ACT_ULPS)
    got = _run_linear_bwd(ops, c, o)
    for name in ("dw", "db", "dx"):
        if got[name] is None:
            continue
        what = f"linear_bwd {c['name']} {'ordered' if det else 'atomic'} {name}"
        if c["kind"] == "int":
            check_f32_exact(ref[name][0], what)
            assert_bit_equal(got[name], ref[name][0], what)
        else:
            assert_within_abs(got[name], ref[name][0], ref[name][1], what)
    if det:
        again = _run_linear_bwd(ops, c, o)
        for name in ("dw", "db", "dx"):
            assert got[name] is None or same_bits(got[name], again[name]), f"{name}: two ordered runs differ"


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("code", sorted(ACT_ULPS))
def test_activation_code_backward(ops, det_mode, code, det):
    """w = I, dout = 1, K = O = 64: dx = act'(x) element for element."""
    det_mode(det)
    x = E.code_inputs()
    flat, dx = guarded(tuple(x.shape), F32)
    ops.linear_bwd(torch.ones(x.shape[0], 64, device=DEV), dev(x), torch.eye(64, device=DEV), None, None, dx, act_in=code)
    torch.cuda.synchronize()
    assert guards_intact(flat)
    want, mag = E.dact64(x, code), E.dact_mag64(x, code)
    print(f"measured: derivative code {code} {'ordered' if det else 'atomic'}: worst {worst_ulps(dx, want, mag):.3f} ulp "
          f"(allowed {ACT_ULPS[code][1]})")
    assert_within_ulps(dx, want, ACT_ULPS[code][1], f"act' {E.ACT_NAMES[code]}", mag=mag)


# ----------------------------------------------------------------------------- rho_timestep_embed
def _te_raw(hip, om, t, t_scalar, g, cond, pe, h, emb, B, dim, edim, act):
    p = hip.ptr
    hip.check(hip.lib().rho_timestep_embed(p(om), p(t), p(t_scalar), p(g["w0"]), p(g["b0"]), p(g["w2"]), p(g["b2"]), p(cond), p(pe), p(h),
                                           p(emb), B, dim, edim, act, hip.stream()), "rho_timestep_embed")


@pytest.mark.parametrize("c", E.TE_CASES, ids=_ids)
def test_timestep_embed_mlp(ops, hip, c):
    """The fused sinusoid + MLP: pe within the project's 5e-7 of the float64 sinusoid; h and emb BIT-equal to rho_linear on the
    kernel's own pe / h (the property its comment states); emb inside the twice-applied linear bound of the float64 chain from the
    device's pe.  Then the case's own form - t_scalar_dev, cond / pe_out / h_out absent - must give the same bits."""
    B, dim, edim, act = c["B"], c["dim"], c["edim"], c["act"]
    o = E.te_operands(c)
    g = {k: dev(o[k]) for k in ("w0", "b0", "w2", "b2")}
    om, t = dev(o["omega"]), dev(o["t"])
    cond = dev(o["cond"]) if c["cond"] else None
    (fpe, pe), (fh, h), (fe, emb) = guarded((B, dim), F32), guarded((B, edim), F32), guarded((B, edim), F32)
    _te_raw(hip, om, t, None, g, cond, pe, h, emb, B, dim, edim, act)
    torch.cuda.synchronize()
    assert guards_intact(fpe) and guards_intact(fh) and guards_intact(fe)
    what = f"timestep_embed {c['name']}"
    assert_within_abs(pe, E.te_sinusoid64(o["t"], o["omega"]), E.PE_ABS, what + " pe")
    assert_bit_equal(h, ops.linear(pe.contiguous(), g["w0"], g["b0"]), what + " h vs rho_linear(pe)")
    assert_bit_equal(emb, ops.linear(h.contiguous(), g["w2"], g["b2"], add=cond, act_in=act), what + " emb vs rho_linear(act(h))")
    ref, bound = E.te_chain_ref(pe.cpu(), o, act, o["cond"] if c["cond"] else None, ACT_ULPS)
    assert_within_abs(emb, ref, bound, what + " emb vs the float64 chain")
    # the case's own call
    ts = torch.tensor([c["t"][0]], dtype=torch.int32, device=DEV) if c["t_scalar"] else None
    fpe2, pe2 = guarded((B, dim), F32) if c["pe_out"] else (None, None)
    fh2, h2 = guarded((B, edim), F32) if c["h_out"] else (None, None)
    fe2, emb2 = guarded((B, edim), F32)
    _te_raw(hip, om, None if c["t_scalar"] else t, ts, g, cond, pe2, h2, emb2, B, dim, edim, act)
    torch.cuda.synchronize()
    assert guards_intact(fe2) and same_bits(emb2, emb), what + ": emb of the case's own call differs"
    if c["pe_out"]:
        assert guards_intact(fpe2) and same_bits(pe2, pe)
    if c["h_out"]:
        assert guards_intact(fh2) and same_bits(h2, h)


# ----------------------------------------------------------------------------- rho_multi_embed
def _me_tables(space, tables):
    """(space, key_off, pointer array) on the device for value lists `space` and device tables `tables`."""
    off = np.cumsum([0] + [len(s) for s in space]).astype(np.int32)
    ptrs = torch.tensor([t.data_ptr() for t in tables], dtype=torch.int64, device=DEV)
    return torch.cat(space).to(F32).to(DEV), torch.from_numpy(off).to(DEV), ptrs


def _me_forward(hip, y, space, tables, dim, want_idx=True, want_err=True, nkeys=None):
    """(out, idx or None, err or None) on the CPU; guards asserted."""
    nkeys = len(space) if nkeys is None else nkeys
    B = y.shape[0]
    tabs = [dev(t) for t in tables]
    sp, off, ptrs = _me_tables(space, tabs)
    fo, out = guarded((B, dim), F32)
    fi, idx = guarded_i32((B, nkeys)) if want_idx else (None, None)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if want_err else None
    p = hip.ptr
    yd = dev(y)
    hip.check(hip.lib().rho_multi_embed(p(yd), 1 if y.dim() == 1 else y.shape[1], p(sp), p(off), p(ptrs), nkeys, B, dim, p(out), p(idx),
                                        p(err), hip.stream()), "rho_multi_embed")
    torch.cuda.synchronize()
    assert guards_intact(fo) and (fi is None or guards_intact_i32(fi))
    return out.cpu(), None if idx is None else idx.cpu(), None if err is None else int(err.item())


@pytest.mark.parametrize("c", E.ME_CASES, ids=_ids)
def test_multi_embed_forward(hip, c):
    """Real-valued tables: the gather and the ordered float32 adds e_0; += e_i are exact by construction, so bit-equal."""
    o = E.me_operands(c, integer=False)
    idx_ref = E.me_lookup(o["y"], o["space"])
    out, idx, err = _me_forward(hip, o["y"], o["space"], o["tables"], c["dim"])
    assert err == 0 and torch.equal(idx, idx_ref)
    assert_bit_equal(out, E.me_forward_ref(idx_ref, o["tables"], c["dim"]), f"multi_embed {c['name']}")


ME_EDGE_SPACE = [torch.tensor([1.0, 2.0, 2.0, 3.0]), torch.tensor([-0.0, 5.0]), torch.tensor([0.5])]


def _edge_tables(dim):
    return [det_normal((len(s), dim), f"me_edge{i}") for i, s in enumerate(ME_EDGE_SPACE)]


def test_multi_embed_first_match_zero_nan_unknown(hip):
    """Duplicate values: the first match; -0.0 matches 0.0 and back; a NaN label or one unknown in key i sets err_flag to 2 and
    idx = -1 for that key only while the others are summed; a sample that matches nowhere is the zero row."""
    dim = 257
    y = torch.tensor([[2.0, 0.0, 0.5], [3.0, -0.0, 0.25], [float("nan"), 5.0, 0.5], [7.0, 7.0, 7.0], [1.0, 5.0, 0.5]])
    want_idx = [[1, 0, 0], [3, 0, -1], [-1, 1, 0], [-1, -1, -1], [0, 1, 0]]
    tabs = _edge_tables(dim)
    assert E.me_lookup(y, ME_EDGE_SPACE).tolist() == want_idx
    out, idx, err = _me_forward(hip, y, ME_EDGE_SPACE, tabs, dim)
    assert idx.tolist() == want_idx and err == 2
    assert_bit_equal(out, E.me_forward_ref(torch.tensor(want_idx), tabs, dim), "multi_embed edges")
    assert bool((out[3] == 0).all())
    # no unknown label: the flag stays 0
    out, idx, err = _me_forward(hip, y[[0, 4]], ME_EDGE_SPACE, tabs, dim)
    assert err == 0 and idx.tolist() == [want_idx[0], want_idx[4]]


def test_multi_embed_one_label_for_all_keys(hip):
    """y_stride == 1 with several keys: every key looks the sample's one label up in its own list."""
    dim = 300
    space = [torch.tensor([0.0, 1.0, 2.0]), torch.tensor([2.0, 1.0]), torch.tensor([5.0, 0.0, 2.0, 2.0])]
    y = torch.tensor([2.0, 1.0, 0.0, 5.0, 2.0, 9.0, 1.0])
    tabs = [det_normal((len(s), dim), f"me_1d{i}") for i, s in enumerate(space)]
    want = E.me_lookup(y, space)
    assert want.tolist() == [[2, 0, 2], [1, 1, -1], [0, -1, 1], [-1, -1, 0], [2, 0, 2], [-1, -1, -1], [1, 1, -1]]
    out, idx, err = _me_forward(hip, y, space, tabs, dim)
    assert torch.equal(idx, want) and err == 2
    assert_bit_equal(out, E.me_forward_ref(want, tabs, dim), "multi_embed 1-D labels")


@pytest.mark.parametrize("want_idx,want_err", [(False, True), (True, False), (False, False)])
def test_multi_embed_optional_outputs(hip, want_idx, want_err):
    """idx_out and err_flag each NULL, with an unknown label in the batch."""
    dim = 256
    y = torch.tensor([[2.0, 0.0, 0.5], [3.0, 5.0, 0.25], [1.0, 5.0, 0.5]])
    tabs = _edge_tables(dim)
    ref_idx = E.me_lookup(y, ME_EDGE_SPACE)
    out, idx, err = _me_forward(hip, y, ME_EDGE_SPACE, tabs, dim, want_idx=want_idx, want_err=want_err)
    assert_bit_equal(out, E.me_forward_ref(ref_idx, tabs, dim), "multi_embed optional outputs")
    assert idx is None or torch.equal(idx, ref_idx)
    assert err is None or err == 2


def test_multi_embed_refuses_17_keys(hip):
    """nkeys above the kernel's 16 category slots: RHO_E_ARG from the forward and the backward, nothing written."""
    p = hip.ptr
    sp, off, _ = _me_tables([torch.tensor([0.0, 1.0])] * 17, [])
    y, demb = torch.zeros(2, 17, device=DEV), torch.ones(2, 8, device=DEV)
    idx = torch.zeros(2, 17, dtype=torch.int32, device=DEV)
    table = torch.ones(2, 8, device=DEV)
    for fn in ("fwd", "bwd"):
        flat, buf = guarded((2, 8), F32)
        with pytest.raises(hip.RhoHipError):
            if fn == "fwd":
                ptrs = torch.tensor([table.data_ptr()] * 17, dtype=torch.int64, device=DEV)
                hip.check(hip.lib().rho_multi_embed(p(y), 17, p(sp), p(off), p(ptrs), 17, 2, 8, p(buf), None, None, hip.stream()),
                          "rho_multi_embed")
            else:
                ptrs = torch.tensor([buf.data_ptr()] * 17, dtype=torch.int64, device=DEV)
                hip.check(hip.lib().rho_multi_embed_bwd(p(demb), p(idx), p(ptrs), 17, 2, 8, hip.stream()), "rho_multi_embed_bwd")
        torch.cuda.synchronize()
        assert guards_intact(flat) and bool(torch.isnan(buf).all())


# ----------------------------------------------------------------------------- rho_multi_embed_bwd
def _me_backward(hip, o, c):
    """One launch onto guarded copies of the prefilled tables: the tables on the CPU."""
    bufs = [guarded_copy(t, F32) for t in o["tables"]]
    ptrs = torch.tensor([v.data_ptr() for _, v in bufs], dtype=torch.int64, device=DEV)
    demb, idx = dev(o["demb"]), dev(o["idx"])
    hip.check(hip.lib().rho_multi_embed_bwd(hip.ptr(demb), hip.ptr(idx), hip.ptr(ptrs), c["nkeys"], c["B"], c["dim"], hip.stream()),
              "rho_multi_embed_bwd")
    torch.cuda.synchronize()
    for i, (flat, _) in enumerate(bufs):
        assert guards_intact(flat), f"table {i}: guard band written"
    return [v.cpu() for _, v in bufs]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("c", E.ME_CASES, ids=_ids)
def test_multi_embed_backward_integer(hip, det_mode, c, det):
    """Integer demb added onto integer tables: bit-equal in both modes, whole tables compared, so rows that no label names - and the
    rows of dropped samples (idx = -1) - are bit-unchanged; 64 samples on one row is the contended case."""
    det_mode(det)
    o = E.me_operands(c, integer=True)
    _, exact, _ = E.me_backward_ref(o["idx"], o["demb"], o["tables"])
    got = _me_backward(hip, o, c)
    for i in range(c["nkeys"]):
        check_f32_exact(exact[i], f"{c['name']} key {i}")
        assert_bit_equal(got[i], exact[i], f"multi_embed_bwd {c['name']} {'ordered' if det else 'atomic'} key {i}")


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
@pytest.mark.parametrize("c", [c for c in E.ME_CASES if c["B"] > 1], ids=_ids)
def test_multi_embed_backward_real(hip, det_mode, c, det):
    """Real demb: the ordered kernel is bit-equal to the float32 running sum in batch order; the atomic one is within
    B * 2^-24 * (sum of the terms' magnitudes) of the float64 sum."""
    det_mode(det)
    o = E.me_operands(c, integer=True)
    o["demb"] = E.me_operands(c, integer=False)["demb"]
    ordered, exact, mag = E.me_backward_ref(o["idx"], o["demb"], o["tables"])
    got = _me_backward(hip, o, c)
    for i in range(c["nkeys"]):
        what = f"multi_embed_bwd real {c['name']} key {i}"
        if det:
            assert same_bits(got[i], ordered[i]), what + ": not the float32 running sum in batch order"
        else:
            assert_within_abs(got[i], exact[i], c["B"] * E.U * mag[i], what)
