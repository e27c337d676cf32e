"""CPU: the cases of tests/attn_cases.py before any kernel sees them.

  * the inputs are what the GPU test needs them to be (conditions on the fp64 reference, never on kernel output);
  * a plain-torch model of the bf16 kernels' rounding points stays inside the per-element bounds on every case;
  * the bounds discriminate: each of seven mutations of that model leaves them in at least one element on every case it applies to,
    and the fp32 bounds reject an fp32 walk whose P and dS are rounded to bf16;
  * rho_attention_variant answers as EXPECT_ATTN says, in a fresh process without the switches and in one with both set (the
    library latches them on first use), and refuses what the launches refuse.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):      # (run as a script by the variant test below)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_cases as A  # noqa: E402

IDS = [A.case_id(c) for c in A.CASES]
DT = {"bf16": A.BF16, "f32": A.F32}


@pytest.mark.parametrize("dname", ["bf16", "f32"])
@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_inputs_meet_the_conditions(case, dname):
    """Peaked, not one-hot, with a staircase.  Per (batch, head) the median effective key count 1 / sum p^2 lies in [3, 16].  In
    ascending (even) heads every query's running maximum rises on at least 2 key tiles after the first, so l and O are rescaled
    with 0 < alpha < 1 tile after tile - for the tile length of each forward kernel the case runs (k_attn_bf16, k_attn_f32m,
    k_attn_f32), and where the sequence has two tiles after the first in which a whole 32-key level of the staircase begins:
    T = 49 has none, and T = 130 ends in a tile of two keys, which cannot both beat the 32 keys one level below for every query
    and leave the softmax three effective keys; there the count is the number of such tiles.  In descending (odd) heads at least
    one whole 32-query wave sees no rise after the first tile: the rescale-skip branch of k_attn_bf16 and k_attn_f32m, for their
    tile lengths (k_attn_f32 has no such branch)."""
    B, T, H, ch = case
    dtype = DT[dname]
    skip_kts, valu_kt = A.forward_kts(ch)
    st = A.input_stats(case, dtype)
    print(f"{A.case_id(case)} {dname}: median effective keys per (b, h) {[round(v, 1) for v in st['neff'].flatten().tolist()]}")
    assert bool((st["neff"] >= 3).all()) and bool((st["neff"] <= 16).all()), st["neff"]
    for KT in sorted(set(skip_kts) | {valu_kt}):
        st = A.input_stats(case, dtype, KT)
        need = min(2, st["level_tiles"])
        asc = st["rises"][:, 0::2]
        print(f"   KT {KT}: ascending heads, rises per query min {int(asc.min())} (need {need})")
        assert int(asc.min()) >= need, KT
        if H > 1 and KT in skip_kts:
            des = st["rises"][:, 1::2]
            quiet = sum(bool((des[b, h, i:i + 32] == 0).all()) for b in range(B) for h in range(des.shape[1]) for i in range(0, T - 31, 32))
            print(f"   KT {KT}: descending heads, {quiet} whole waves without a rise after the first tile")
            assert quiet >= 1, KT
    r, b = A.reference(case, dtype), A.bounds(case, dtype)
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(r[n]).all())
        assert bool(torch.isfinite(b[n]).all()) and float(b[n].min()) > 0, n
    for n in ("out", "dq", "dk", "dv"):
        cap = float((b["f32_" + n] / b["mag_" + n]).max()) * 1024
        print(f"   fp32 bound / magnitude term of {n}: {cap:.3f} * 2^-10")
        assert cap <= 1.0, (n, cap)
        assert tuple(b[n].shape) == (B, H, T, ch)
    assert float(b["lse"].max()) < 1e-3


@pytest.mark.parametrize("dname", ["bf16", "f32"])
@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_rounding_model_stays_inside_the_bounds(case, dname):
    """(The largest error / bound ratios seen here in bf16: 0.61 on out, 0.42 on dQ, 0.34 on dK, 0.56 on dV, 0.06 on lse.  The fp32
    walk, torch's fp32 on the CPU, sits far inside the worst-case fp32 bounds.)"""
    got = A.model(case, dtype=DT[dname])
    ra = A.ratios(got, case, DT[dname])
    print(A.case_id(case), dname, "model error / bound:", {k: round(v, 3) for k, v in ra.items()})
    assert set(ra) == {"out", "lse", "dq", "dk", "dv"}
    for n, v in ra.items():
        assert v <= 1.0, (n, v)


@pytest.mark.parametrize("dname", ["bf16", "f32"])
@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_every_mutation_breaks_a_bound(mut, dname):
    cases = [c for c in A.CASES if A.mutation_applies(mut, c)]
    assert len(cases) >= 5
    for case in cases:
        ra = A.ratios(A.model(case, mut, dtype=DT[dname]), case, DT[dname])
        print(mut, dname, A.case_id(case), {k: round(v, 2) for k, v in ra.items()})
        assert max(ra.values()) > 1.0, (mut, case, ra)


@pytest.mark.parametrize("case", A.CASES, ids=IDS)
def test_fp32_bounds_reject_lowered_precision(case):
    """The fp32 bounds are worst cases - sums of n fp32 terms get n 2^-24, the difference dP - delta a (ch + 4) 2^-24 term of its
    own - and the fp32 walk sits at a few hundredths of them.  They still tell fp32 from less: the same walk with P and dS
    rounded to bf16 (what k_attn_bf16 does, and what an fp32 kernel must not) leaves them on every case."""
    ra = A.ratios(A.model(case, dtype=A.F32, round_p=True), case, A.F32)
    print(A.case_id(case), "fp32 operands, P and dS rounded to bf16: error / fp32 bound", {k: round(v, 2) for k, v in ra.items()})
    assert min(ra[n] for n in ("out", "dq", "dk", "dv")) > 1.0, ra


def test_no_mutation_is_the_model_itself():
    """The mutations change the model's output (a mutation that did nothing would prove nothing)."""
    case = A.E2E_CASE
    base = A.model(case)
    for mut in A.MUTATIONS:
        assert A.mutation_applies(mut, case)
        got = A.model(case, mut)
        assert any(not torch.equal(got[n], base[n]) for n in base), mut


# ----------------------------------------------------------------------------- the variant query
def _query_all():
    import ctypes as C
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    hip.load()
    out = {}
    for dname, dt in DT.items():
        for ch in (16, 32, 64, 128, 256):
            for bwd in (False, True):
                out[f"{dname},{ch},{int(bwd)}"] = ops.attention_variant(dt, ch, backward=bwd)
    buf = C.create_string_buffer(128)
    L = hip.lib()
    out["rc"] = [L.rho_attention_variant(hip.RHO_BF16, 48, 0, buf, 128), L.rho_attention_variant(hip.RHO_F32, 8, 1, buf, 128),
                 L.rho_attention_variant(77, 64, 0, buf, 128), L.rho_attention_variant(77, 48, 1, buf, 128),
                 L.rho_attention_variant(hip.RHO_BF16, 64, 0, buf, 8), L.rho_attention_variant(hip.RHO_BF16, 64, 0, None, 128)]
    return out


@pytest.mark.parametrize("switched", [False, True], ids=["default", "switched"])
def test_variant_query_in_a_fresh_process(switched):
    env = {k: v for k, v in os.environ.items() if k not in A.SWITCHES}
    if switched:
        env.update(A.SWITCHES)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--variants"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout)
    E_ARG, E_SHAPE = -1, -3
    assert got.pop("rc") == [E_SHAPE, E_SHAPE, E_ARG, E_ARG, E_ARG, E_ARG]
    want = {f"{d},{ch},{int(b)}": n for (sw, d, ch, b), n in A.EXPECT_ATTN.items() if sw == switched}
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}


def test_the_table_names_every_kernel_of_the_family():
    """Three forward and eight backward kernels + k_attn_delta, each for five head widths where the dispatcher has it."""
    names = A.kernel_names(A.EXPECT_ATTN.values())
    fam = {n.split("<")[0] for n in names}
    assert fam == {"k_attn_bf16", "k_attn_f32m", "k_attn_f32", "k_attn_delta", "k_attn_dq", "k_attn_dkv", "k_attn_dkv_fused",
                   "k_attn_dq_f32m", "k_attn_dkv_f32m", "k_attn_dq_f32", "k_attn_dkv_f32"}
    # 3 x 5 forward; delta x 2; dq 5 + dkv 10 + fused 1; f32m pair 2 x 4 (ch = 256 has none); VALU pair 2 x 5
    assert len(names) == 15 + 2 + 16 + 8 + 10, sorted(names)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--variants"]
    json.dump(_query_all(), sys.stdout)
