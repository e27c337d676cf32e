"""-m gpu: the two table-driven launches every weight passes through each training step, bit for bit against the CPU references of
weight_table_cases.py (integer operands, outputs inside NaN-prefilled guarded buffers, test_weight_table_cases_host.py proves the
references):

  rho_prep_batch            (k_prep_batch, csrc/weight_tables.hip) through ops.PrepTable: every layout kind in ONE table of 49 ops
                            (the bisection finds first, middle and last ops), the LDS transpose path at 3 / 9 / 27 / 32 taps with
                            ragged channel groups and row tables, the elementwise path at 1 and 36 taps, again with the per-op block
                            cap at 3 (several trips of both walks), as a one-op table, and the engine's own table against the eager
                            per-tensor refresh.
  rho_wgrad_finalize_batch  (k_wgrad_finalize_batch, csrc/weight_tables.hip) through ops.WfinTable over a synthetic arena: kinds
                            0 / 1 / 2, LDS and elementwise walks, row tables with holes, nblk = 1, accumulation onto prefilled gradients.

The per-tensor entry points of the same layouts (k_prep_one through ops.EagerPrep, k_wfin_one, k_wgrad_finalize_phase) run the same
device code on one op passed by value: they are judged by the same references, and each batched result is compared with theirs."""
import math

import pytest
import torch

import weight_table_cases as X
from exact_util import assert_bit_equal, guarded, guarded_copy, guards_intact
from gpu_util import DEV
from helpers import UNET_CASES, case_inputs, det_state_dict, golden_template, load_golden

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "f32"]


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _report(failures):
    assert not failures, f"{len(failures)} ops differ:\n" + "\n".join(failures)


def _collect(failures, fn, *a):
    try:
        fn(*a)
    except AssertionError as e:
        failures.append(str(e))


# ============================================================================================ rho_prep_batch
def _prep_into(sink, names, dtype):
    """The ops ``names`` into ``sink`` (an ops.PrepTable, or ops.EagerPrep: the per-tensor entry points, launched at once), each
    output inside a guarded buffer -> {name: (flat, view)}."""
    return X.prep_into(sink, names, dtype, guarded, DEV)


def _launch(ops, names, dtype):
    table = ops.PrepTable(DEV)
    outs = _prep_into(table, names, dtype)
    table.launch()
    torch.cuda.synchronize()
    return table, {n: (flat, out, out.float().cpu()) for n, (flat, out) in outs.items()}


ALL_PREP = [c["name"] for c in X.PREP_CASES]
PER_TENSOR_PREP = [c["name"] for c in X.PREP_CASES if c["kind"] != "vec"]       # (the general gather has no per-tensor entry point)


@pytest.fixture(scope="module")
def per_tensor_runs(ops):
    """Every layout with a per-tensor entry point through it (rho_prep_conv_weight / _dgrad / _phase / _sel on k_prep_one)."""
    res = {}
    for dt in DTYPES:
        outs = _prep_into(ops.EagerPrep(), PER_TENSOR_PREP, dt)
        torch.cuda.synchronize()
        res[dt] = {n: (flat, out, out.float().cpu()) for n, (flat, out) in outs.items()}
    return res


@pytest.fixture(scope="module")
def prep_runs(ops):
    """The whole case table in one launch per output dtype, under the default block cap."""
    return {dt: _launch(ops, ALL_PREP, dt) for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_batch_every_layout_bit_equal_to_the_reference(prep_runs, dtype):
    table, res = prep_runs[dtype]
    assert len(table.ops) == len(ALL_PREP) >= 20
    blk = 0
    for op, name in zip(table.ops, ALL_PREP):                            # the geometry the host twin reasons about is the table's
        g = X.prep_geometry(X.prep_io(name, dtype))
        assert (op.blk0, op.nblk, op.total) == (blk, g["nblk"], g["total"]), name
        blk += op.nblk
    failures = []
    for name in ALL_PREP:
        flat, _, got = res[name]
        _collect(failures, assert_bit_equal, got, X.prep_io(name, dtype)["ref"], f"{name} [{dtype}]")
        if not guards_intact(flat):
            failures.append(f"{name} [{dtype}]: a store outside the output")
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_batch_equals_the_per_tensor_entry_points(prep_runs, per_tensor_runs, dtype):
    _, res = prep_runs[dtype]
    failures, compared = [], 0
    for name in ALL_PREP:
        if name not in per_tensor_runs[dtype]:
            continue
        compared += 1
        _, single, got = per_tensor_runs[dtype][name]
        assert single.dtype == res[name][1].dtype
        _collect(failures, assert_bit_equal, res[name][2], got, f"{name} [{dtype}] vs its per-tensor launch")
    assert compared == sum(c["kind"] != "vec" for c in X.PREP_CASES)
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_tensor_prep_bit_equal_to_the_reference(per_tensor_runs, dtype):
    """rho_prep_conv_weight / _dgrad / _phase / _sel (k_prep_one) on every case with such an entry point, judged by the CPU
    reference itself (the batched launch shares their code, so agreeing with it proves nothing): both walks, ragged 64-groups on
    either axis, a second trip of the LDS walk at 3 taps (fwd_t3: 64 rows x 2 groups = 128 units on the 72 / 60 blocks of one
    output element per thread) and blocks with no unit at 27, and the row table with fewer rows than the parameter (qkv /
    holes).  Outputs through ``out=`` views of guarded buffers."""
    res = per_tensor_runs[dtype]
    assert len(res) == len(PER_TENSOR_PREP) >= 40
    for name, more_units in (("fwd_t3", True), ("fwd_t27", False)):       # the launch's blocks: ceil(total / 256), at most 2048
        g = X.prep_geometry(X.prep_io(name, dtype))
        assert g["lds"] and (g["units"] > min(-(-g["total"] // 256), 2048)) == more_units, name
    failures = []
    for name in PER_TENSOR_PREP:
        flat, _, got = res[name]
        _collect(failures, assert_bit_equal, got, X.prep_io(name, dtype)["ref"], f"{name} [{dtype}] per-tensor")
        if not guards_intact(flat):
            failures.append(f"{name} [{dtype}] per-tensor: a store outside the output")
    _report(failures)


def test_prep_functions_allocate_the_prepared_shape(ops):
    """The stand-alone functions without ``out``: the shape rules give the case table's shapes, the values the reference's."""
    td = torch.bfloat16
    for name, call in (("fwd_t9", lambda w, c: ops.prep_conv_weight(w, td)), ("dgrad_t9", lambda w, c: ops.prep_conv_weight_dgrad(w, td)),
                       ("phase_333_12_dgrad", lambda w, c: ops.prep_conv_weight_phase(w, td, c["ph"], dgrad=True)),
                       ("sel_01", lambda w, c: ops.prep_conv_weight_sel(w, td, c["sel"]))):
        io = X.prep_io(name, "bf16")
        got = call(io["w"].to(DEV), io["case"])
        assert got.dtype == td
        assert_bit_equal(got.float().cpu(), io["ref"], f"{name} through the function")


@pytest.mark.parametrize("dtype", DTYPES)
def test_prep_batch_with_three_blocks_per_op_walks_several_trips_to_the_same_bits(ops, prep_runs, dtype, monkeypatch):
    monkeypatch.setenv("RHO_PREP_MAX_BLOCKS", "3")
    table, res = _launch(ops, ALL_PREP, dtype)
    assert max(op.nblk for op in table.ops) == 3 and table._blocks <= 3 * len(ALL_PREP)
    failures = []
    for name in ALL_PREP:
        flat, _, got = res[name]
        _collect(failures, assert_bit_equal, got, prep_runs[dtype][1][name][2], f"{name} [{dtype}] capped vs uncapped")
        _collect(failures, assert_bit_equal, got, X.prep_io(name, dtype)["ref"], f"{name} [{dtype}] capped")
        if not guards_intact(flat):
            failures.append(f"{name} [{dtype}]: a store outside the output")
    _report(failures)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [X.PREP_ONE_OP, "dgrad_t3_wide", "vec_short_n"])
def test_prep_batch_one_op_table(ops, name, dtype):
    table, res = _launch(ops, [name], dtype)
    assert len(table.ops) == 1 and table.ops[0].blk0 == 0
    flat, _, got = res[name]
    assert_bit_equal(got, X.prep_io(name, dtype)["ref"], f"{name} [{dtype}] alone")
    assert guards_intact(flat)


def test_prep_case_gathers_are_the_engine_classes_own(ops):
    """The index tables of the two head re-readings in the case table are the ones the engine's classes build."""
    from torch import nn
    from rho_diffusion_amd.engine.weights import _HeadAsGemm, _HeadDgradW
    hd = _HeadDgradW(nn.Parameter(X.prep_io("vec_head_dgrad", "bf16")["w"].to(DEV)), torch.bfloat16)
    assert torch.equal(hd._perm.cpu(), X.head_dgrad_perm(32))
    hg = _HeadAsGemm(nn.Parameter(X.prep_io("vec_head_as_gemm", "bf16")["w"].to(DEV)), nn.Parameter(torch.zeros(1, device=DEV)), torch.bfloat16)
    t = ops.PrepTable(DEV)
    assert hg.prep_into(t)
    assert torch.equal(hg._perm.cpu(), X.head_as_gemm_perm(32, hg.w.shape[2]))
    torch.cuda.synchronize()
    assert_bit_equal(hd.w.float().cpu(), X.prep_io("vec_head_dgrad", "bf16")["ref"], "_HeadDgradW eager refresh")
    assert_bit_equal(hg.w.float().cpu(), X.prep_io("vec_head_as_gemm", "bf16")["ref"], "_HeadAsGemm eager refresh")


@pytest.mark.parametrize("case", ["tiny3d", "tiny2d"])
def test_engine_prep_table_equals_the_eager_refresh(ops, case):
    """The table UNetEngine.refresh_weights launches after every optimizer step against each object's eager per-tensor refresh(),
    every layout of a bf16 training plan (tiny2d: attention with its qkv row table, a downsample and an upsample; tiny3d: the
    one-channel ends), and the forward layouts against the CPU reference."""
    from rho_diffusion_amd.engine.weights import _ConvW
    from rho_diffusion_amd.models import UNet
    g = load_golden("g4_unet.npz")
    kw, _, ykind = UNET_CASES[case]
    assert ykind is None
    model = UNet(**dict(kw), compute_dtype=torch.bfloat16)
    model.load_state_dict(det_state_dict(golden_template(g, case), case))
    model = model.to(DEV).train()
    _, x, t, _ = case_inputs(case)
    model(x.to(DEV), t.to(DEV))                                           # builds the training plan: every layout exists now
    eng = model.engine()
    assert eng._last_train_plan is not None
    eng.refresh_weights(force=True)
    torch.cuda.synchronize()
    assert not eng._prep_eager                                            # every object went through the table
    objs = eng._convs + eng._aux_weights
    bufs, kinds = [], set()
    for i, cw in enumerate(objs):
        if isinstance(cw, _ConvW):
            for kind, buf, _ in cw.layouts():
                bufs.append((f"{type(cw).__name__}#{i} {tuple(cw.weight.shape)} {kind}", buf))
                kinds.add(kind)
        else:
            bufs.append((f"{type(cw).__name__}#{i}", cw.w))
    assert {"fwd", "bias", "dgrad"} <= kinds, kinds
    batched = [b.clone() for _, b in bufs]
    film_w, film_b = eng.film_w.clone(), eng.film_b.clone()
    for _, b in bufs:
        b.fill_(float("nan"))
    for cw in objs:
        cw.refresh()
    torch.cuda.synchronize()
    failures = []
    for (what, b), want in zip(bufs, batched):
        _collect(failures, assert_bit_equal, want.float().cpu(), b.float().cpu(), f"{case} {what}: table vs eager refresh")
    for i, cw in enumerate(objs):                                         # the arbiter: the forward layout by plain indexing
        if type(cw) is _ConvW:
            rs = cw.row_src.cpu() if cw.row_src is not None else None
            ref = X.ref_fwd(cw.weight.detach().cpu(), cw.kernel, cw.coutp, cw.cinp, rs).to(torch.bfloat16).float()
            _collect(failures, assert_bit_equal, batched[[n for n, _ in bufs].index(f"_ConvW#{i} {tuple(cw.weight.shape)} fwd")].float().cpu(), ref,
                     f"{case} _ConvW#{i} fwd: table vs reference")
    lins = [blk.emb_layers[1] for blk in eng._film_blocks]
    _collect(failures, assert_bit_equal, film_w.cpu(), torch.cat([l.weight.detach() for l in lins]).cpu(), f"{case} film_w")
    _collect(failures, assert_bit_equal, film_b.cpu(), torch.cat([l.bias.detach() for l in lins]).cpu(), f"{case} film_b")
    eng.refresh_weights(force=True)
    _report(failures)


# ============================================================================================ rho_wgrad_finalize_batch
ALL_WFIN = tuple(c["name"] for c in X.WFIN_CASES)


def _wfin_launch(ops, names):
    """One WfinTable over the ops ``names`` on a guarded copy of the synthetic arena -> per op (flat, grad view), the arena after."""
    from rho_diffusion_amd import hip
    io = X.wfin_io(tuple(names))
    aflat, arena = guarded_copy(io["arena"], torch.float32)
    table, grads, keep = ops.WfinTable(DEV), [], []
    for op in io["ops"]:
        c = op["case"]
        rs = op["rs"].to(DEV) if op["rs"] is not None else None
        keep.append(rs)
        grads.append(guarded_copy(op["grad0"], torch.float32))
        table.add(kind=c["kind"], off=op["off"] + c.get("off_extra", 0), rs=(rs.data_ptr() if rs is not None else None), cout=c["cout"],
                  cin=c["cin"], coutp=c["coutp"], cinb=c["cinb"], k=c["k"], up_h=c.get("up", (0, 0))[0], up_w=c.get("up", (0, 0))[1],
                  stride=X.wfin_stride(c), nblk=c.get("nblk"))
    table.build(arena.data_ptr(), [g.data_ptr() for _, g in grads])
    hip.check(table.launch(), "rho_wgrad_finalize_batch")
    torch.cuda.synchronize()
    return io, table, grads, (aflat, arena), keep


def _wfin_check(io, grads, arena, what):
    failures = []
    for op, (flat, gview) in zip(io["ops"], grads):
        _collect(failures, assert_bit_equal, gview.cpu(), op["ref"], f"{op['case']['name']} {what}")
        if not guards_intact(flat):
            failures.append(f"{op['case']['name']} {what}: a store outside the gradient")
    _collect(failures, assert_bit_equal, arena[1].cpu(), io["arena"], "the arena is read only")
    assert guards_intact(arena[0])
    _report(failures)


def test_wfin_batch_every_kind_bit_equal_to_the_reference(ops):
    io, table, grads, arena, _ = _wfin_launch(ops, ALL_WFIN)
    assert len(table.entries) >= 12
    recs = table.records(arena[1].data_ptr(), [g.data_ptr() for _, g in grads])
    for r, op in zip(recs, io["ops"]):
        c = op["case"]
        assert r.nblk == (c.get("nblk") or X.wfin_nblk(r.total)), c["name"]
    _wfin_check(io, grads, arena, "in the full table")


@pytest.mark.parametrize("name", [X.WFIN_ONE_OP, "k1_333_11", "k2_c64"])
def test_wfin_batch_one_op_table(ops, name):
    io, table, grads, arena, _ = _wfin_launch(ops, (name,))
    assert len(table.entries) == 1
    _wfin_check(io, grads, arena, "alone")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_per_tensor_wgrad_finalize_bit_equal_to_the_reference(ops, accumulate):
    """rho_wgrad_finalize (k_wfin_one) on every kind-0 case, judged by ref_wfin: accumulate = 1 adds the buffer to the prefilled
    gradient; accumulate = 0 stores it - the reference run on a zero gradient where the op writes, the prefill kept on the rows a row
    table with holes skips."""
    io = X.wfin_io(ALL_WFIN)
    arena = io["arena"].to(DEV)
    failures, n = [], 0
    for op in io["ops"]:
        c = op["case"]
        if c["kind"] != 0:
            continue
        n += 1
        taps = math.prod(c["k"])
        rs = op["rs"].to(DEV) if op["rs"] is not None else None
        flat, g = guarded_copy(op["grad0"], torch.float32)
        base = arena[op["off"] + c.get("off_extra", 0):]
        ops.wgrad_finalize(base[:taps * c["coutp"] * c["cinb"]].view(taps, c["coutp"], c["cinb"]), g, rs, accumulate=bool(accumulate))
        torch.cuda.synchronize()
        want = op["ref"]
        if not accumulate:
            region = io["arena"][op["off"]:op["off"] + X.wfin_region_floats(c)]
            written = X.ref_wfin(c, region, torch.zeros_like(op["grad0"]), op["rs"])
            rows = torch.zeros(c["cout"], dtype=torch.bool)
            for r in range(c["cout"]):
                d = X._src_row(op["rs"], r, c["cout"])
                if d >= 0:
                    rows[d] = True
            assert bool(rows.all()) == (c.get("rs") != "holes"), c["name"]
            want = torch.where(rows.view(-1, *[1] * (op["grad0"].dim() - 1)), written, op["grad0"])
        _collect(failures, assert_bit_equal, g.cpu(), want, f"{c['name']} accumulate={accumulate}")
        if not guards_intact(flat):
            failures.append(f"{c['name']} accumulate={accumulate}: a store outside the gradient")
    assert n == sum(c["kind"] == 0 for c in X.WFIN_CASES) >= 12
    _report(failures)


def test_wfin_batch_equals_the_per_tensor_finalize(ops):
    from rho_diffusion_amd import hip
    io, _, grads, arena, keep = _wfin_launch(ops, ALL_WFIN)
    L, failures, compared = hip.lib(), [], 0
    for op, (_, gview), rs in zip(io["ops"], grads, keep):
        c = op["case"]
        if c["kind"] == 2:
            continue                                                      # (no per-tensor form)
        compared += 1
        flat, g = guarded_copy(op["grad0"], torch.float32)
        base = arena[1][op["off"] + c.get("off_extra", 0):]
        if c["kind"] == 0:
            taps = math.prod(c["k"])
            ops.wgrad_finalize(base[:taps * c["coutp"] * c["cinb"]].view(taps, c["coutp"], c["cinb"]), g, rs, accumulate=True)
        else:
            for p, (a, b) in enumerate(X.wfin_phases(c["up"])):
                dw = base[p * X.wfin_stride(c):]
                hip.check(L.rho_wgrad_finalize_phase(dw.data_ptr(), g.data_ptr(), c["cout"], c["cin"], *c["k"], a, b, c["coutp"], c["cinb"], 1,
                                                     hip.stream()), "rho_wgrad_finalize_phase")
        torch.cuda.synchronize()
        _collect(failures, assert_bit_equal, gview.cpu(), g.cpu(), f"{c['name']}: batched vs per-tensor finalize")
        assert guards_intact(flat)
    assert compared == sum(c["kind"] != 2 for c in X.WFIN_CASES)
    _report(failures)
