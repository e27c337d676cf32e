"""CPU checks of tests/embed_cases.py: the float64 references against torch autograd and the oracle, the representability of every
integer case (a condition on the inputs, never on a kernel's output), and the coverage of the case tables - every listed value of
every axis, every pair of the shape axes, and the boundary pairs the kernels can break at."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import embed_cases as E
from exact_util import check_f32_exact
from oracle import ref_torch as R

TORCH_ACT = {0: lambda u: u, 1: F.silu, 2: F.relu, 3: F.gelu, 4: torch.tanh, 5: torch.sigmoid, 6: F.elu}


# ----------------------------------------------------------------------------- references
@pytest.mark.parametrize("code", E.ACTS)
def test_activations_and_derivatives_match_torch(code):
    u = torch.cat([torch.linspace(-9.0, 9.0, 1441, dtype=torch.float64), torch.tensor([0.0, -0.0, 1e-8, -1e-8], dtype=torch.float64)])
    u = u[u != 0] if code == 2 else u                    # ReLU' at 0: the kernels and torch both take 0, checked below
    ur = u.clone().requires_grad_(True)
    y = TORCH_ACT[code](ur)
    (g,) = torch.autograd.grad(y.sum(), ur)
    assert torch.allclose(E.act64(u, code), y.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(E.dact64(u, code), g, rtol=1e-12, atol=1e-15)
    # the term magnitudes dominate the values and are equal to them away from the cancelling regions
    assert bool((E.act_mag64(u, code) >= E.act64(u, code).abs() * (1 - 1e-15)).all())
    assert bool((E.dact_mag64(u, code) >= E.dact64(u, code).abs() * (1 - 1e-15)).all())
    assert float(E.dact64(u, code).abs().max()) <= E.LIP
    if code == 2:
        z = torch.zeros(2, dtype=torch.float64)
        assert E.act64(z, 2).tolist() == [0.0, 0.0] and E.dact64(z, 2).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("c", [c for c in E.LINEAR_CASES if c["K"] <= 257], ids=lambda c: c["name"])
def test_linear_reference_matches_torch(c):
    o = E.linear_operands(c)
    out, bound = E.linear_ref(o["x"], o["w"], o["bias"], o["add"], c["act_in"], c["act_out"], {k: (1, 1) for k in E.ACTS})
    r = F.linear(TORCH_ACT[c["act_in"]](o["x"].double()), o["w"].double(), None if o["bias"] is None else o["bias"].double())
    if o["add"] is not None:
        r = r + o["add"].double()
    assert torch.allclose(out, TORCH_ACT[c["act_out"]](r), rtol=1e-12, atol=1e-13)
    assert tuple(bound.shape) == tuple(out.shape) and bool((bound >= 0).all()) and bool(torch.isfinite(bound).all())
    if c["kind"] == "real":                              # a bound of a few ulps of the terms, not a tolerance
        assert float(bound.max()) < 1e-4


@pytest.mark.parametrize("c", E.LINEAR_BWD_CASES, ids=lambda c: c["name"])
def test_linear_bwd_reference_matches_autograd(c):
    o = E.linear_bwd_operands(c)
    x = o["x"].double().requires_grad_(True)
    w = o["w"].double().requires_grad_(True)
    b = torch.zeros(c["O"], dtype=torch.float64, requires_grad=True)
    y = F.linear(TORCH_ACT[c["act_in"]](x), w, b)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), o["dout"].double())
    r = E.linear_bwd_ref(o["dout"], o["x"], o["w"], c["act_in"], act_ulps={k: (1, 1) for k in E.ACTS})
    for name, want in (("dw", dw), ("db", db), ("dx", dx)):
        assert torch.allclose(r[name][0], want, rtol=1e-12, atol=1e-12), name
        assert tuple(r[name][1].shape) == tuple(want.shape)
    p = o["pre"]
    r2 = E.linear_bwd_ref(o["dout"], o["x"], o["w"], c["act_in"], p["dw"], p["db"], p["dx"], {k: (1, 1) for k in E.ACTS})
    for name in ("dw", "db", "dx"):
        assert torch.equal(r2[name][0], r[name][0] + p[name].double())
        assert bool((r2[name][1] >= r[name][1]).all())


def test_sinusoid_reference_matches_oracle():
    t = torch.tensor(list(E.TE_T) + [17, 1999])
    for dim in E.TE_DIM:
        om = E.te_omega(dim)
        assert om.dtype == torch.float32 and om.numel() == dim // 2
        pe = E.te_sinusoid64(t, om)
        assert tuple(pe.shape) == (len(t), dim)
        # the oracle evaluates sin / cos in float32 on the host: within its own rounding of the float64 value
        assert float((pe - R.sinusoidal_embedding(t, dim).double()).abs().max()) < 2e-7


def test_timestep_chain_reference_matches_torch():
    c = next(c for c in E.TE_CASES if c["dim"] == 130 and c["edim"] == 70)
    o = E.te_operands(c)
    pe = E.te_sinusoid64(o["t"], o["omega"]).float()
    for act in E.ACTS:
        emb, bound = E.te_chain_ref(pe, o, act, o["cond"], {k: (1, 1) for k in E.ACTS})
        h = F.linear(pe.double(), o["w0"].double(), o["b0"].double())
        want = F.linear(TORCH_ACT[act](h), o["w2"].double(), o["b2"].double()) + o["cond"].double()
        assert torch.allclose(emb, want, rtol=1e-12, atol=1e-13)
        assert float(bound.max()) < 1e-4 and bool((bound > 0).all())


@pytest.mark.parametrize("c", [c for c in E.ME_CASES if not c["dropped"]], ids=lambda c: c["name"])
def test_multi_embed_reference_matches_oracle_and_autograd(c):
    o = E.me_operands(c, integer=False)
    assert torch.equal(E.me_lookup(o["y"], o["space"]), o["idx"])
    keys = [f"k{i}" for i in range(c["nkeys"])]
    space = {k: o["space"][i].tolist() for i, k in enumerate(keys)}
    sd = {f"cond_fn.embedding_layers.{k}.weight": o["tables"][i] for i, k in enumerate(keys)}
    want = R.multi_embeddings(o["y"], space, sd)
    assert torch.equal(E.me_forward_ref(o["idx"], o["tables"], c["dim"]), want)
    # backward: nn.Embedding autograd in float64 on integer operands is exact
    oi = E.me_operands(c, integer=True)
    tabs = [torch.zeros_like(t, dtype=torch.float64, requires_grad=True) for t in oi["tables"]]
    emb = sum(F.embedding(oi["idx"][:, i].long(), tabs[i]) for i in range(c["nkeys"]))
    grads = torch.autograd.grad(emb, tabs, oi["demb"].double())
    ordered, exact, mag = E.me_backward_ref(oi["idx"], oi["demb"], oi["tables"])
    for i in range(c["nkeys"]):
        assert torch.equal(exact[i], oi["tables"][i].double() + grads[i])
        assert torch.equal(ordered[i].double(), exact[i])             # integers: the float32 running sum is exact
        assert bool((mag[i] >= exact[i].abs()).all())


def test_multi_embed_lookup_edges():
    space = [torch.tensor([1.0, 2.0, 2.0, 3.0]), torch.tensor([-0.0, 5.0]), torch.tensor([0.5])]
    y = torch.tensor([[2.0, 0.0, 0.5], [3.0, -0.0, 0.25], [float("nan"), 5.0, 0.5], [7.0, 7.0, 7.0]])
    assert E.me_lookup(y, space).tolist() == [[1, 0, 0], [3, 0, -1], [-1, 1, 0], [-1, -1, -1]]
    assert E.me_lookup(torch.tensor([0.5, 2.0]), space).tolist() == [[-1, -1, 0], [1, -1, -1]]
    tabs = [torch.full((len(s), 3), float(i + 1)) for i, s in enumerate(space)]
    out = E.me_forward_ref(E.me_lookup(y, space), tabs, 3)
    assert out.tolist() == [[6.0] * 3, [3.0] * 3, [5.0] * 3, [0.0] * 3]


# ----------------------------------------------------------------------------- representability of the integer cases
@pytest.mark.parametrize("c", [c for c in E.LINEAR_CASES if c["kind"] == "int"], ids=lambda c: c["name"])
def test_linear_int_cases_are_exact(c):
    assert c["act_in"] in E.INT_ACTS and c["act_out"] in E.INT_ACTS
    o = E.linear_operands(c)
    assert float(o["x"].abs().max()) <= 8 and float(o["w"].abs().max()) <= 8
    for k in ("bias", "add"):
        assert o[k] is None or float(o[k].abs().max()) <= 64
    out, _ = E.linear_ref(o["x"], o["w"], o["bias"], o["add"], c["act_in"], c["act_out"])
    check_f32_exact(out, c["name"])
    # every partial sum is bounded by the sum of magnitudes
    S = E.act64(o["x"], c["act_in"]).abs() @ o["w"].double().abs().T + 128
    check_f32_exact(S, c["name"] + " (sum of magnitudes)")
    pre, _ = E.linear_ref(o["x"], o["w"], o["bias"], o["add"], c["act_in"], 0)
    assert float(pre.abs().max()) > 0


@pytest.mark.parametrize("c", [c for c in E.LINEAR_BWD_CASES if c["kind"] == "int"], ids=lambda c: c["name"])
def test_linear_bwd_int_cases_are_exact(c):
    assert c["act_in"] in E.INT_ACTS
    o = E.linear_bwd_operands(c)
    assert float(o["x"].abs().max()) <= 8 and float(o["w"].abs().max()) <= 8 and float(o["dout"].abs().max()) <= 64
    p = o["pre"]
    r = E.linear_bwd_ref(o["dout"], o["x"], o["w"], c["act_in"], p["dw"], p["db"], p["dx"])
    for name in ("dw", "db", "dx"):
        check_f32_exact(r[name][0], f"{c['name']} {name}")
        check_f32_exact(p[name], f"{c['name']} prefill of {name}")
    check_f32_exact(o["dout"].double().abs() @ o["w"].double().abs() + 64, c["name"] + " (sum of magnitudes of dx)")
    check_f32_exact(o["dout"].double().abs().T @ o["x"].double().abs() + 64, c["name"] + " (sum of magnitudes of dw)")


@pytest.mark.parametrize("c", E.ME_CASES, ids=lambda c: c["name"])
def test_multi_embed_bwd_int_cases_are_exact(c):
    o = E.me_operands(c, integer=True)
    ordered, exact, mag = E.me_backward_ref(o["idx"], o["demb"], o["tables"])
    for i in range(c["nkeys"]):
        check_f32_exact(exact[i], f"{c['name']} key {i}")
        check_f32_exact(mag[i], f"{c['name']} key {i} (sum of magnitudes)")
        assert len(set(o["space"][i].tolist())) == c["lens"][i]         # distinct values: one match per label
    for b in c["dropped"]:
        assert o["idx"][b].tolist() == [-1] * c["nkeys"]


# ----------------------------------------------------------------------------- coverage
def _values(cases, key):
    return {c[key] for c in cases}


def _pairs(cases, k1, k2):
    return {(c[k1], c[k2]) for c in cases}


def test_linear_cases_cover_their_axes():
    C = E.LINEAR_CASES
    assert 35 <= len(C) <= 50 and len({c["name"] for c in C}) == len(C)
    assert _values(C, "K") == set(E.LIN_K) and _values(C, "O") == set(E.LIN_O) and _values(C, "B") == set(E.LIN_B)
    assert _pairs(C, "K", "O") == set(itertools.product(E.LIN_K, E.LIN_O))
    assert _pairs(C, "K", "B") == set(itertools.product(E.LIN_K, E.LIN_B))
    assert _pairs(C, "O", "B") == set(itertools.product(E.LIN_O, E.LIN_B))
    for key in ("bias", "add"):
        assert _values(C, key) == {True, False}
        assert _pairs(C, key, "kind") == set(itertools.product((True, False), ("int", "real")))
    assert {(c["bias"], c["add"]) for c in C} == set(itertools.product((True, False), repeat=2))
    real = [c for c in C if c["kind"] == "real"]
    assert _values(real, "act_in") == set(E.ACTS) and _values(real, "act_out") == set(E.ACTS)
    integer = [c for c in C if c["kind"] == "int"]
    assert {(c["act_in"], c["act_out"]) for c in integer} == set(itertools.product(E.INT_ACTS, repeat=2))
    # both kinds at every K and every O; the template boundaries with a partial last workgroup, bit-exact
    assert _pairs(C, "K", "kind") == set(itertools.product(E.LIN_K, ("int", "real")))
    assert _pairs(C, "O", "kind") == set(itertools.product(E.LIN_O, ("int", "real")))
    for K, O in ((257, 5), (257, 3), (1, 1), (2048, 130), (1025, 3), (1025, 5), (65, 3), (63, 5), (256, 130), (1024, 130)):
        assert any(c["K"] == K and c["O"] == O and c["kind"] == "int" for c in C), (K, O)
    for K in (1, 63, 257, 1025, 2048):
        assert any(c["K"] == K and c["B"] == 1 for c in C) and any(c["K"] == K and c["O"] % 4 for c in C)


def test_linear_bwd_cases_cover_their_axes():
    C = E.LINEAR_BWD_CASES
    assert 25 <= len(C) <= 50 and len({c["name"] for c in C}) == len(C)
    assert {(c["K"], c["O"], c["B"]) for c in C} == set(itertools.product(E.BWD_K, E.BWD_O, E.BWD_B))
    for c in C:
        assert c["stride"] in (0, c["O"] + 7)
    strided = [c for c in C if c["stride"]]
    assert _values(strided, "O") == set(E.BWD_O) and _values(strided, "K") == set(E.BWD_K) and _values(strided, "B") == set(E.BWD_B)
    assert {c["O"] for c in C if not c["stride"]} == set(E.BWD_O)
    assert _pairs(strided, "O", "kind") >= {(65, "int"), (130, "int"), (63, "int"), (64, "int")}
    assert _values(C, "absent") == set(E.BWD_ABSENT)
    for a in E.BWD_ABSENT:
        sub = [c for c in C if c["absent"] == a]
        assert _values(sub, "kind") == {"int", "real"}, a
        assert any(c["stride"] for c in sub) and any(not c["stride"] for c in sub), a
    assert {(c["acc_params"], c["acc_dx"]) for c in C} == set(itertools.product((True, False), repeat=2))
    assert {(c["acc_params"], c["acc_dx"]) for c in C if c["kind"] == "int"} == set(itertools.product((True, False), repeat=2))
    assert _values([c for c in C if c["kind"] == "real"], "act_in") == set(E.ACTS)
    assert _values([c for c in C if c["kind"] == "int"], "act_in") == set(E.INT_ACTS)
    # the atomic slices: one full, one short by one, one over by one, three slices - with dx present, integer, accumulated and not
    for O in (63, 64, 65, 130):
        sub = [c for c in C if c["O"] == O and c["kind"] == "int" and c["absent"] != "dx"]
        assert sub, O
    assert any(c["acc_dx"] and c["absent"] != "dx" and c["O"] >= 65 and c["kind"] == "int" for c in C)
    assert any(not c["acc_dx"] and c["absent"] != "dx" and c["O"] >= 65 and c["kind"] == "int" for c in C)
    assert any(c["absent"] == "dw" and c["acc_params"] for c in C) and any(c["absent"] == "dw" and not c["acc_params"] for c in C)


def test_timestep_cases_cover_their_axes():
    C = E.TE_CASES
    assert 30 <= len(C) <= 45 and len({c["name"] for c in C}) == len(C)
    assert _pairs(C, "dim", "edim") == set(itertools.product(E.TE_DIM, E.TE_EDIM))
    assert _pairs(C, "dim", "B") == set(itertools.product(E.TE_DIM, E.TE_B))
    assert _pairs(C, "edim", "B") == set(itertools.product(E.TE_EDIM, E.TE_B))
    assert {t for c in C for t in c["t"]} == set(E.TE_T)
    for key in ("t_scalar", "cond", "pe_out", "h_out"):
        assert _values(C, key) == {True, False}, key
    assert _pairs(C, "dim", "act") == set(itertools.product(E.TE_DIM, E.ACTS))
    assert _values([c for c in C if c["t_scalar"]], "act") == set(E.ACTS)          # t_scalar_dev together with the MLP
    assert {(c["pe_out"], c["h_out"]) for c in C} == set(itertools.product((True, False), repeat=2))
    for c in C:
        assert c["dim"] % 2 == 0 and (c["dim"] + c["edim"]) * 4 <= 65536 and len(c["t"]) == c["B"]
    assert any(c["edim"] % 4 and c["edim"] > 64 for c in C) and any(c["dim"] % 64 and c["dim"] > 64 for c in C)


def test_multi_embed_cases_cover_their_axes():
    C = E.ME_CASES
    assert 15 <= len(C) <= 45 and len({c["name"] for c in C}) == len(C)
    assert _pairs(C, "nkeys", "dim") == set(itertools.product(E.ME_NKEYS, E.ME_DIM))
    assert _pairs(C, "nkeys", "B") == set(itertools.product(E.ME_NKEYS, E.ME_B))
    assert _pairs(C, "dim", "B") == set(itertools.product(E.ME_DIM, E.ME_B))
    lens = {n for c in C for n in c["lens"]}
    assert lens >= set(E.ME_LIST_LEN) and min(lens) == 1 and max(lens) == 71
    assert any(c["B"] == 64 and set(c["lens"]) == {1} for c in C)                  # every sample on one row
    assert any(c["dropped"] and len(c["dropped"]) < c["B"] for c in C)
    for c in C:
        assert len(c["lens"]) == c["nkeys"] <= 16
        o = E.me_operands(c, integer=True)
        # a repeated row somewhere unless the batch is 1: the scatter has something to collide on
        if c["B"] == 64:
            assert any(len(set(o["idx"][:, i].tolist())) < c["B"] for i in range(c["nkeys"]))


def test_code_inputs_span_the_real_cases():
    x = E.code_inputs()
    assert tuple(x.shape) == (16, 64) and float(x.min()) == -6.0 and float(x.max()) == 6.0
    worst = max(float(E.linear_operands(c)["x"].abs().max()) for c in E.LINEAR_CASES if c["kind"] == "real")
    assert worst <= 6.0
    assert math.isfinite(float(np.float32(worst)))
