"""CPU: what the per-tensor weight entry points refuse, and what ops.prep_op - the one builder of rho_prep_op records - writes
and refuses.  Every argument check returns before a launch, so no pointer here is ever read (they are made-up addresses); the calls
are made in ONE child process that sees no GPU, so that a check that stopped refusing gives an error code there and a failed
assertion here, on a machine with a GPU too, never a launch on those addresses."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import weight_table_cases as X

P = 0x10000             # a non-null "device pointer"
BF16, F32 = 1, 0

# One acceptable call per entry point (argument order of include/rho_hip.h) ...
GOOD = {
    "rho_prep_conv_weight": dict(w=P, out=P, dtype=BF16, cout=40, cin=72, taps=3, coutp=64, cinp=96, row_src=None, stream=None),
    "rho_prep_conv_weight_dgrad": dict(w=P, out=P, dtype=BF16, cout=40, cin=72, taps=3, rowsp=96, colsp=64, col_src=None, stream=None),
    "rho_prep_conv_weight_phase": dict(w=P, out=P, dtype=F32, cout=40, cin=72, kd=3, kh=3, kw=3, ph_h=1, ph_w=2, coutp=64, cinp=80, dgrad=0,
                                       stream=None),
    "rho_prep_conv_weight_sel": dict(w=P, out=P, dtype=BF16, cout=40, cin=72, kd=3, kh=3, kw=3, kh2=2, kw2=1, sel_h=0x20, sel_w=0x1, flip_d=0,
                                     coutp=64, cinp=96, dgrad=0, stream=None),
    "rho_wgrad_finalize": dict(dw=P, grad=P, cout=40, cin=72, taps=3, coutp=64, cin_buf=80, row_src=None, accumulate=1, stream=None),
    "rho_wgrad_finalize_phase": dict(dw=P, grad=P, cout=40, cin=72, kd=3, kh=3, kw=3, ph_h=1, ph_w=2, coutp=64, cin_buf=96, accumulate=1,
                                     stream=None),
}
_NONPOS = lambda *fields: [{f: v} for f in fields for v in (0, -1)]                                  # noqa: E731
_PHASE = [dict(ph_h=-1), dict(ph_h=3), dict(ph_w=-1), dict(ph_w=3), dict(ph_h=0, ph_w=0),
          dict(kh=2), dict(kh=4, ph_w=0), dict(kw=2), dict(kw=1, ph_h=0)]                              # a phased axis must have 3 taps
# ... and every change to it that the entry point answers with RHO_E_ARG (the conditions of the checks, one class per line)
BAD = {
    "rho_prep_conv_weight": [dict(w=None), dict(out=None)] + _NONPOS("cout", "cin", "taps")
    + [dict(cinp=71), dict(coutp=39), dict(coutp=0), dict(dtype=2), dict(dtype=-1), dict(taps=2 ** 31)],        # (taps: an int32 in the op)
    "rho_prep_conv_weight_dgrad": [dict(w=None), dict(out=None)] + _NONPOS("cout", "cin", "taps")
    + [dict(rowsp=71), dict(colsp=39), dict(colsp=39, col_src=P), dict(dtype=2), dict(taps=2 ** 31)],
    "rho_prep_conv_weight_phase": [dict(w=None), dict(out=None)] + _NONPOS("cout", "cin", "kd", "kh", "kw")
    + [dict(cinp=71), dict(coutp=39), dict(cinp=71, dgrad=1), dict(coutp=39, dgrad=1), dict(dtype=2)] + _PHASE,
    "rho_prep_conv_weight_sel": [dict(w=None), dict(out=None)] + _NONPOS("cout", "cin", "kd", "kh", "kw", "kh2", "kw2")
    + [dict(kh2=5, sel_h=0x21020), dict(kw2=5, sel_w=0x21020), dict(cinp=71), dict(coutp=39), dict(coutp=39, dgrad=1),
       dict(sel_h=0x30), dict(sel_h=0x3), dict(sel_w=0x3), dict(kw2=2, sel_w=0x31), dict(kh=2), dict(dtype=2)],
    "rho_wgrad_finalize": [dict(dw=None), dict(grad=None)] + _NONPOS("cout", "cin", "taps") + [dict(coutp=39), dict(coutp=39, row_src=P),
                                                                                                 dict(cin_buf=71), dict(taps=2 ** 31)],
    "rho_wgrad_finalize_phase": [dict(dw=None), dict(grad=None)] + _NONPOS("cout", "cin", "kd", "kh", "kw")
    + [dict(coutp=39), dict(cin_buf=71)] + _PHASE,
}
BAD_CALLS = [(fn, ch) for fn, changes in BAD.items() for ch in changes]


CHILD = """
import json, sys
from rho_diffusion_amd import hip
L = hip.load()
print(json.dumps([getattr(L, fn)(*args) for fn, args in json.load(sys.stdin)]))
"""


@pytest.fixture(scope="module")
def status():
    """{(entry point, index of the change): status code} of every bad call, from the child process without a GPU."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    calls = [(fn, list(dict(GOOD[fn], **ch).values())) for fn, ch in BAD_CALLS]
    r = subprocess.run([sys.executable, "-c", CHILD], input=json.dumps(calls), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(zip(range(len(BAD_CALLS)), json.loads(r.stdout.strip().splitlines()[-1])))


@pytest.mark.parametrize("i", range(len(BAD_CALLS)), ids=[f"{fn[4:]}-{'-'.join(f'{k}={v}' for k, v in ch.items())}" for fn, ch in BAD_CALLS])
def test_per_tensor_entry_points_refuse_bad_arguments(status, i):
    from rho_diffusion_amd import hip
    fn, change = BAD_CALLS[i]
    assert set(change) <= set(GOOD[fn]) and len(GOOD[fn]) == len(hip.SIGNATURES[fn][1])
    assert status[i] == -1                                                       # RHO_E_ARG


def test_bad_argument_cases_cover_every_entry_point_and_class():
    assert set(BAD) == set(GOOD) and len(GOOD) == 6
    for fn, changes in BAD.items():
        fields = {f for ch in changes for f in ch}
        assert {"cout", "cin"} <= fields and ({"w", "out"} <= fields or {"dw", "grad"} <= fields), fn
        assert ("dtype" in fields) == fn.startswith("rho_prep"), fn
        assert ("ph_h" in fields) == fn.endswith("_phase"), fn
    assert {"kh2", "kw2", "sel_h", "sel_w"} <= {f for ch in BAD["rho_prep_conv_weight_sel"] for f in ch}


# ============================================================================================ ops.prep_op
def _recording_sink():
    """A sink that keeps the records (what PrepTable does before it assigns the blocks)."""
    from rho_diffusion_amd.engine import ops

    class Records(ops.PrepSink):
        def __init__(self):
            self.ops = []

        def _push(self, op, w, out, perm):
            self.ops.append(op)
    return Records()


BUILDER_CASES = ["fwd_t1", "fwd_t27", "fwd_t32", "fwd_t36k", "fwd_qkv_t3", "dgrad_t3_wide", "dgrad_holes_t3", "phase_333_12", "phase_133_02_dgrad",
                 "sel_10", "sel_11_dgrad", "vec_bias_pad", "vec_short_n", "vec_head_as_gemm"]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_prep_op_records_are_what_prep_geometry_predicts(dtype):
    sink = _recording_sink()
    outs = X.prep_into(sink, BUILDER_CASES, dtype, lambda shape, td: (None, torch.empty(shape, dtype=td)))
    assert len(sink.ops) == len(BUILDER_CASES)
    for op, name in zip(sink.ops, BUILDER_CASES):
        io = X.prep_io(name, dtype)
        c, g, out = io["case"], X.prep_geometry(io), outs[name][1]
        assert (op.kind, op.total, op.out, op.blk0, op.nblk) == (X.KIND_CODE[c["kind"]], g["total"], out.data_ptr(), 0, 0), name
        assert op.dtype == {"bf16": 1, "f32": 0}[io["out_dtype"]], name
        taps = op.kd * op.kh * op.kw
        assert g["lds"] == (op.kind in (0, 1) and 1 < taps <= 32), name
        if c["kind"] == "vec":
            assert (op.cout, op.cin, op.d1, op.d2) == (io["n"] or io["w"].numel(), io["w"].numel(), g["total"], 1), name
            continue
        assert (op.cout, op.cin, op.d1, op.d2) == tuple(c["wshape"][:2]) + tuple(io["out_shape"][1:]), name
        assert (op.kd, op.kh, op.kw) == tuple(io["k"]) and taps == math.prod(io["k"]), name
        if g["lds"]:
            assert g["units"] == op.d1 * -(-op.d2 // 64), name
        assert (op.perm is not None) == (io["perm"] is not None), name
        if c["kind"] == "phase":
            assert (op.ph_h, op.ph_w, op.dgrad) == tuple(c["ph"]) + (int(c["dgrad"]),), name
        if c["kind"] == "sel":
            assert [(op.sel_h >> 4 * r) & 15 for r in range(op.kh2)] == list(c["sel"][0]), name
            assert [(op.sel_w >> 4 * r) & 15 for r in range(op.kw2)] == list(c["sel"][1]), name
            assert (op.flip_d, op.dgrad) == (int(c["flip_d"]), int(c["dgrad"])), name


def test_prepared_shape_is_the_case_tables_padding():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    for dtype in ("bf16", "f32"):
        for c in X.PREP_CASES:
            if c["kind"] == "vec":
                continue
            io = X.prep_io(c["name"], dtype)
            got = ops.prepared_shape(X.KIND_CODE[c["kind"]], c["wshape"], X.TORCH_DTYPE[dtype], c.get("dgrad", False), k=c.get("k"),
                                     phase_hw=c.get("ph", (0, 0)), sel_hw=c.get("sel", (None, None)))
            assert got == tuple(io["out_shape"]), c["name"]
    assert ops.kernel3((4, 5)) == (1, 1, 1) and ops.kernel3(torch.empty(4, 5, 3)) == (1, 1, 3) and ops.kernel3((4, 5, 2, 3, 7)) == (2, 3, 7)
    assert ops.sel_code((2, 0)) == 0x02 and ops.sel_code((0, 1, 2)) == 0x210 and hip.PREP_VEC == 4


def test_prep_op_refuses_extents_the_tensors_do_not_hold():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    E = hip.RhoHipError
    w = torch.zeros(40, 72, 3, 3)
    out = torch.zeros(9, 64, 96, dtype=torch.bfloat16)
    assert ops.prep_op(hip.PREP_FWD, w, out).total == out.numel()
    for kind in (hip.PREP_FWD, hip.PREP_DGRAD, hip.PREP_PHASE, hip.PREP_SEL):
        kw = {hip.PREP_PHASE: dict(phase_hw=(1, 1)), hip.PREP_SEL: dict(sel_hw=((1,), (0, 2)))}.get(kind, {})
        taps2 = {hip.PREP_PHASE: 4, hip.PREP_SEL: 2}.get(kind, 9)
        d = (96, 64) if kind == hip.PREP_DGRAD else (64, 96)
        good = torch.zeros(taps2, *d, dtype=torch.bfloat16)
        ops.prep_op(kind, w, good, **kw)
        with pytest.raises(E, match=rf"kind {kind}.*the source holds {w.numel()} .*\(40, 72, 3, 3\).*\({taps2}, "):        # cout * cin * taps > w.numel()
            ops.prep_op(kind, w, good, cout=41, **kw)
        with pytest.raises(E, match="taps"):                                        # taps' * d1 * d2 != out.numel()
            ops.prep_op(kind, w, torch.zeros(taps2 + 1, *d, dtype=torch.bfloat16), **kw)
        with pytest.raises(E, match="contiguous"):
            ops.prep_op(kind, w, torch.zeros(taps2, d[0], 2 * d[1], dtype=torch.bfloat16)[:, :, ::2], **kw)
        with pytest.raises(E, match="does not hold"):                               # a padded extent below the real one
            ops.prep_op(kind, w, torch.zeros(taps2, d[0], 32, dtype=torch.bfloat16), **kw)
    src = torch.zeros(50)
    ops.prep_op(hip.PREP_VEC, src, torch.zeros(64), n=64, perm=torch.zeros(64, dtype=torch.int32))
    with pytest.raises(E, match="holds 50"):                                        # src.numel() < cin
        ops.prep_op(hip.PREP_VEC, src, torch.zeros(64), cin=51)
    with pytest.raises(E, match="out holds 64"):                                    # n > out.numel()
        ops.prep_op(hip.PREP_VEC, src, torch.zeros(64), n=65, perm=torch.zeros(80, dtype=torch.int32))
    with pytest.raises(E, match="contiguous"):
        ops.prep_op(hip.PREP_VEC, src, torch.zeros(128)[::2])
    with pytest.raises(E, match="index table"):                                     # a table shorter than what is looked up
        ops.prep_op(hip.PREP_VEC, src, torch.zeros(64), n=64, perm=torch.zeros(50, dtype=torch.int32))
    with pytest.raises(E, match="index table"):
        ops.prep_op(hip.PREP_FWD, w, out, perm=torch.zeros(40, dtype=torch.int32))


def test_prep_op_refuses_the_head_parameter_read_as_32_rows():
    """A [1, C, 3, 3, 3] parameter offered as 32 rows x C of a 1x1x1 conv (the geometry of _HeadAsGemm: rows = taps, padded to 32)
    would be indexed up to 32 * C in a tensor that holds 27 * C."""
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    C_ = 32
    w = torch.zeros(1, C_, 3, 3, 3)
    for kind, out in ((hip.PREP_FWD, torch.zeros(1, 32, C_, dtype=torch.bfloat16)), (hip.PREP_DGRAD, torch.zeros(1, C_, 32, dtype=torch.bfloat16))):
        with pytest.raises(hip.RhoHipError, match=rf"kind {kind}.*{32 * C_} elements.*{27 * C_}.*\(1, {C_}, 3, 3, 3\).*\(1, 32, 32\)"):
            ops.prep_op(kind, w, out, cout=32, cin=C_, k=(1, 1, 1))
        ops.prep_op(kind, w, out, cout=27, cin=C_, k=(1, 1, 1))                      # (what it does hold)
