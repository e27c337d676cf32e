"""CPU twin of test_gpu_exact_layernorm.py and test_gpu_exact_v1_tail.py: proves, for every case of ln_cases.py and (second half of
the file) of v1_cases.py, what the GPU tests take for granted.

  - the geometry twin (G, NV, rpb, blocks per sample, sweeps) against a literal table read off ln_geom / ln_bps of vit.hip, and that
    every case reaches the branch it names, in every dtype it runs in;
  - the operands are exact in bf16, the references are on fp32 grids, and torch's float32 evaluation of the kernel's operation
    sequence with the kernel's block structure (ln_bwd_model32) equals the fp64 formulas wherever the GPU test demands bit equality;
    where it demands a bound, the float32 model is inside it;
  - the share of bf16 elements the tie rule lets pass on either neighbour is at most 1 % per tensor;
  - the model notices wrong code: each mutation (second sweep dropped, a slot's partial row skipped, the m2 term omitted, a ragged
    vector read as live; for the v1 GroupNorm: the fp32 run carry not flushed) fails the cases it must, and those are named."""
import pytest
import torch

import ln_cases as LN
from exact_util import TIE_SHARE_MAX, check_bf16_exact, check_f32_exact, check_f32_grid, f32_ulp, tie_margin, tie_share
from ln_cases import BF16, F32

_ids = [LN.case_id(c, dt) for c, dt in LN.LN_PARAMS]
_cache = {}


def _bwd(c):
    if c["name"] not in _cache:
        o = LN.ln_bwd_operands(c)
        _cache[c["name"]] = (o, LN.ln_bwd_reference(c, o))
    return _cache[c["name"]]


# (E, dtype) -> (G, NV, rpb), by hand from ln_geom: nvec = E / PE; G = the power of two in [4, 64] reaching nvec; NV = the power of
# two reaching ceil(nvec / G); rpb = 256 / G
GEOM_TABLE = {
    (32, F32): (8, 1, 32), (32, BF16): (4, 1, 64),
    (96, F32): (32, 1, 8), (96, BF16): (16, 1, 16),
    (160, F32): (64, 1, 4), (160, BF16): (32, 1, 8),
    (256, F32): (64, 1, 4), (256, BF16): (32, 1, 8),
    (1024, F32): (64, 4, 4), (1024, BF16): (64, 2, 4),
    (1056, F32): (64, 8, 4), (1056, BF16): (64, 4, 4),
    (2048, F32): (64, 8, 4), (2048, BF16): (64, 4, 4),
}
# case -> (nb, bps, sweeps) for float32, by hand from ln_bps: want = ceil(rps / rpb), cap = max(1, 1024 / nb)
LAUNCH_TABLE = {
    "e32_add": (3, 3, 1), "e32_plain_acc": (1, 3, 1), "e96_idle": (2, 2, 1), "e160_idle": (1, 3, 1), "e256_full": (3, 3, 1),
    "e1056_ragged": (2, 2, 1), "e1056_ragged_plain": (1, 2, 1), "e2048_max": (2, 2, 1), "e2048_max_plain": (1, 2, 1),
    "e256_ragged_rows": (2, 6, 1), "e32_one_row": (1, 1, 1), "e2048_one_row": (1, 1, 1), "e1024_sweeps": (512, 2, 3),
    "e32_sweeps": (1024, 1, 3),
}


@pytest.mark.parametrize("c,dtype", LN.LN_PARAMS, ids=_ids)
def test_geometry_twin_and_branch(c, dtype):
    L = LN.ln_layout(c, dtype)
    assert (L["G"], L["NV"], L["rpb"]) == GEOM_TABLE[(c["E"], dtype)], (c["name"], L)
    assert L["G"] * L["NV"] * L["PE"] >= c["E"] and L["rpb"] * c["E"] <= 8192, "a row must fit the lanes, a block's rows the LDS"
    if dtype == F32:
        assert (L["nb"], L["bps"], L["sweeps"]) == LAUNCH_TABLE[c["name"]], (c["name"], L)
    assert L["bps"] * L["nb"] <= 1024 or L["bps"] == 1
    assert LN.BRANCHES[c["branch"]](c, L), f"{LN.case_id(c, dtype)} does not reach its branch {c['branch']}: {L}"
    assert c["rows"] * c["E"] * 4 <= 50 * 2 ** 20, "a tensor of more than 50 MB"


def test_every_branch_and_mode_has_a_case():
    seen = {c["branch"] for c in LN.LN_CASES}
    assert seen == set(LN.BRANCHES), set(LN.BRANCHES) - seen
    for dt in (F32, BF16):
        cs = [c for c in LN.LN_CASES if dt in c["dtypes"]]
        for key in ("add", "acc_dx", "acc_params"):
            assert {bool(c[key]) for c in cs} == {False, True}, (key, dt)
        assert any(c["add"] and not c["dadd"] for c in cs), "dadd absent while add is present"
        assert any(c["add"] and c["rps"] > 1 for c in cs)
        assert any(LN.ln_layout(c, dt)["sweeps"] >= 3 for c in cs), dt
    assert {32, 256, 2048} <= set(LN.EXACT_DX_WIDTHS)
    assert all((e & (e - 1)) == 0 for e in LN.EXACT_DX_WIDTHS), "bit equality of dx rests on fl(1 / E) being exact"


@pytest.mark.parametrize("c,dtype", LN.LN_PARAMS, ids=_ids)
def test_backward_model_equals_fp64_where_bit_equality_is_demanded(c, dtype):
    o, r = _bwd(c)
    E = c["E"]
    for k in ("x", "dy", "gamma", "mean", "pre_dx", "pre_dgamma", "pre_dbeta") + (("add",) if c["add"] else ()):
        check_bf16_exact(o[k], f"{c['name']} {k}")
    assert set(o["rstd"].tolist()) <= {0.5, 1.0, 2.0}
    check_f32_grid(r["xhat"], 0.5, "xhat")
    check_f32_grid(r["dgamma"], 0.5, "dgamma")
    check_f32_exact(r["dbeta"], "dbeta")
    # the magnitude sums bound every partial sum in any order
    check_f32_grid((o["dy"].double() * r["xhat"]).abs().sum(0), 0.5, "sum |dy xhat| + prefill")
    m = LN.ln_bwd_model32(c, o, dtype)
    what = LN.case_id(c, dtype)
    assert torch.equal(m["dgamma"].double(), r["dgamma"]), what + ": dgamma"
    assert torch.equal(m["dbeta"].double(), r["dbeta"]), what + ": dbeta"
    # every (b, k) partial row the finalize reads adds up to the plain column sums
    assert torch.equal(m["part"][:, :, 1].double().sum((0, 1)), o["dy"].double().sum(0))
    if LN.dx_is_exact(c):
        check_f32_grid(r["m1"], 1.0 / E, "m1")
        check_f32_grid(r["m2"], 0.5 / E, "m2")
        check_f32_grid(r["xhat"] * r["m2"], 0.25 / E, "xhat m2")
        check_f32_grid(r["dx_mag"], 0.125 / E, "|g| + |m1| + |xhat m2|, scaled")
        check_f32_grid(r["dx"], 0.125 / E, "dx")
        assert torch.equal(m["m1"].double(), r["m1"]) and torch.equal(m["m2"].double(), r["m2"]), what + ": m1 / m2"
        assert torch.equal(m["dx"].double(), r["dx"]), what + ": dx"
        if c["add"]:
            check_f32_grid(r["dadd_mag"], 0.125 / E, "sum of the dx magnitudes")
            assert torch.equal(m["dadd"].double(), r["dadd"]), what + ": dadd"
    else:
        ulps = LN.DX_ULPS + (1 if c["acc_dx"] else 0)
        mag = r["dx_mag"] + (o["pre_dx"].double().abs() if c["acc_dx"] else 0.0)
        err = (m["dx"].double() - r["dx"]).abs() / f32_ulp(mag)
        assert float(err.max()) <= ulps, f"{what}: the float32 model is {float(err.max())} ulps off, outside the derived {ulps}"
        assert float(err.max()) > 0, f"{what}: fl(1 / E) is inexact here, the model should differ from fp64 somewhere"


def _mutation_failures(mutation):
    bad = []
    for c in LN.LN_CASES:
        o, r = _bwd(c)
        m = LN.ln_bwd_model32(c, o, F32, mutation)
        keys = ["dgamma", "dbeta"] + (["dx"] if LN.dx_is_exact(c) else []) + (["dadd"] if c["add"] and LN.dx_is_exact(c) else [])
        if any(not torch.equal(m[k].double(), r[k]) for k in keys):
            bad.append(c["name"])
    return bad


def test_mutations_of_the_backward_model_are_noticed():
    sweeps = [c["name"] for c in LN.LN_CASES if LN.ln_layout(c, F32)["sweeps"] >= 2]
    assert sweeps, "no case sweeps twice"
    bad = _mutation_failures("second_sweep_dropped")
    assert sorted(bad) == sorted(sweeps), f"second sweep dropped: noticed by {bad}, must be noticed by exactly {sweeps}"
    multi = [c["name"] for c in LN.LN_CASES if LN.ln_layout(c, F32)["rps"] > 1]
    bad = _mutation_failures("slot_skipped")
    assert sorted(bad) == sorted(multi), f"a slot's partial row skipped: noticed by {bad}, must be noticed by {multi}"
    exact = [c["name"] for c in LN.LN_CASES if LN.dx_is_exact(c)]
    bad = _mutation_failures("m2_omitted")
    assert sorted(bad) == sorted(exact), f"m2 term omitted: noticed by {bad}, must be noticed by every exact-dx case {exact}"
    assert _mutation_failures(None) == []


@pytest.mark.parametrize("c", [c for c in LN.LN_CASES if not LN.dx_is_exact(c)], ids=lambda c: c["name"])
def test_m2_omitted_is_outside_the_bound_of_the_inexact_widths(c):
    o, r = _bwd(c)
    m = LN.ln_bwd_model32(c, o, F32, "m2_omitted")
    mag = r["dx_mag"] + (o["pre_dx"].double().abs() if c["acc_dx"] else 0.0)
    err = (m["dx"].double() - r["dx"]).abs() / f32_ulp(mag)
    assert float(err.max()) > 1000 * LN.DX_ULPS, c["name"]


# ---- forward -----------------------------------------------------------------------------------------------------------------------
FWD_CASES = [c for c in LN.LN_CASES if c["rows"] * c["E"] <= 2 ** 21]      # the multi-sweep shapes exist for the backward's row loop


@pytest.mark.parametrize("c", FWD_CASES, ids=lambda c: c["name"])
def test_forward_operands_have_integer_means_and_exact_variance_sums(c):
    o = LN.ln_fwd_operands(c)
    r = LN.ln_fwd_reference(c, o)
    for k in ("x", "gamma", "beta") + (("add",) if c["add"] else ()):
        check_bf16_exact(o[k], f"{c['name']} {k}")
    assert torch.equal(r["mean"], o["k"].double()), "row means must be the integers k"
    check_f32_exact(r["sq"], "sum of squared deviations")
    if c["E"] * c["rows"] > 32:
        assert float(r["var"].min()) >= 1.0, "RSTD_ULPS neglects eps's own rounding only for var >= 1"
    share = tie_share(r["y"], tie_margin(LN.Y_ULPS, r["y_mag"]))
    assert share <= TIE_SHARE_MAX, f"{c['name']}: {share:.3%} of y within the tie margin"


def test_ragged_vector_read_as_live_is_noticed():
    must = [c for c in FWD_CASES if c["rows"] > 1 and c["branch"] in ("ragged", "idle_lanes")]
    assert must
    for dt in (F32, BF16):
        bad = []
        for c in FWD_CASES:
            o = LN.ln_fwd_operands(c)
            r, m = LN.ln_fwd_reference(c, o), LN.ln_fwd_reference(c, o, dt, "ragged_read_as_live")
            if not torch.equal(r["mean"], m["mean"]):
                bad.append(c["name"])
        assert set(x["name"] for x in must) <= set(bad), f"ragged vector read as live: noticed by {bad}, must include {[x['name'] for x in must]}"
        full = [c["name"] for c in FWD_CASES if LN.ln_geom(c["E"], dt)["G"] * LN.ln_geom(c["E"], dt)["NV"] == LN.ln_geom(c["E"], dt)["nvec"]]
        assert not set(full) & set(bad), "a row that fills its lanes has nothing to misread"


# ---- the legacy-UNet tail (v1_cases.py) --------------------------------------------------------------------------------------------
import v1_cases as V1  # noqa: E402

_v1ids = lambda c: c["name"]  # noqa: E731


def test_v1_cases_reach_their_branches():
    by = {c["name"]: c for c in V1.V1_CASES}
    assert {c["cpg"] for c in V1.V1_CASES} >= {1, 3, 12, 32, 260}
    assert by["s1"]["S"] == 1 and by["cpg3"]["cpg"] & (by["cpg3"]["cpg"] - 1)
    carry = [c["name"] for c in V1.V1_CASES if V1.per_thread(c) > 64]
    assert carry == ["cpg32_carry"] and by["cpg32_carry"]["m"] > 16384 and by["cpg32_carry"]["m"] // 256 >= 65, "every thread must carry a run"
    assert by["cpg260"]["cpg"] > 256 and V1.lds_bytes(by["cpg260"]) == 512 * 8 + 2 * 260 * 4 <= 64 * 1024
    assert {V1.dx_is_exact(c) for c in V1.V1_CASES} == {False, True}


@pytest.mark.parametrize("c", V1.V1_CASES, ids=_v1ids)
def test_v1_forward_operands_and_run_sums(c):
    o = V1.v1_fwd_operands(c)
    r = V1.v1_fwd_reference(c, o)
    for k in ("x", "gamma", "beta"):
        check_bf16_exact(o[k], f"{c['name']} {k}")
    assert torch.equal(r["mean"], o["k"].double()), "group means must be the integers k"
    check_f32_exact(r["sumsq"], "sum of squares: every fp32 run of x * x is exact")
    assert float(r["var"].min()) >= 0.5, "V1_RSTD_ULPS neglects eps's own rounding only for var >= 0.5"
    su, sq = V1.v1_fwd_sums_model(c, o)
    xg = V1._group_view(o["x"].double(), c)
    assert torch.equal(su, xg.sum(1)) and torch.equal(sq, (xg * xg).sum(1)), c["name"] + ": the run / carry model must give the exact sums"
    share = tie_share(r["y"], tie_margin(V1.V1_Y_ULPS, r["y_mag"]))
    assert share <= TIE_SHARE_MAX, f"{c['name']}: {share:.3%} of y within the tie margin"


def test_v1_carry_not_flushed_is_noticed():
    bad = []
    for c in V1.V1_CASES:
        o = V1.v1_fwd_operands(c)
        su, sq = V1.v1_fwd_sums_model(c, o, "carry_not_flushed")
        xg = V1._group_view(o["x"].double(), c)
        if not (torch.equal(su, xg.sum(1)) and torch.equal(sq, (xg * xg).sum(1))):
            bad.append(c["name"])
    assert bad == ["cpg32_carry"], f"carry not flushed: noticed by {bad}, must be noticed by cpg32_carry (the only case above 16384 per group)"


@pytest.mark.parametrize("c", V1.V1_CASES, ids=_v1ids)
def test_v1_backward_model_equals_fp64_where_bit_equality_is_demanded(c):
    o = V1.v1_bwd_operands(c)
    r = V1.v1_bwd_reference(c, o)
    for k in ("x", "dy", "gamma", "beta", "mean", "pre_dgamma", "pre_dbeta"):
        check_bf16_exact(o[k], f"{c['name']} {k}")
    assert set(o["rstd"].flatten().tolist()) <= {0.5, 1.0, 2.0}
    check_f32_grid(r["dgamma_mag"], 0.5, "sum |dy xhat| + |prefill|: every order of the float atomics is exact")
    check_f32_grid(r["dgamma"], 0.5, "dgamma")
    check_f32_exact(r["dbeta"], "dbeta")
    m = V1.v1_bwd_reference(c, o, F32)
    if V1.dx_is_exact(c):
        check_f32_grid(r["m1"], 1.0 / c["m"], "m1")
        check_f32_grid(r["m2"], 0.5 / c["m"], "m2")
        check_f32_grid(r["dx_mag"], 0.125 / c["m"], "|g| + |m1| + |xhat m2|, scaled")
        assert torch.equal(m["dx"], r["dx"]), c["name"] + ": dx"
    else:
        err = (m["dx"] - r["dx"]).abs() / f32_ulp(r["dx_mag"])
        assert 0 < float(err.max()) <= V1.V1_DX_ULPS, f"{c['name']}: the float32 model is {float(err.max())} ulps off (derived {V1.V1_DX_ULPS})"
    o2 = V1.act_add_operands()
    assert float((o2["x"].abs().max() + o2["r"].abs().max() + o2["nc"].abs().max())) <= 256
