"""CPU only: the float64 twin of the VisionTransformer restatement (tests/vit_ref64.py) and the case table of the whole-ViT sweep
(tests/vit_sweep_cases.py).

- the twin at float32 IS ``vit_ref``: ``torch.equal`` on the prediction, the loss, every parameter gradient and the input gradient, on
  the four recorded cases and the six new ones;
- ``vit_ref`` reproduces what the reference's own module gives on the new cases (tests/golden/g25_vit_sweep.npz), with the assertions
  of test_vit_host.py::test_vit_ref_is_pinned_to_the_reference, and the project's module has the recorded state_dict layout;
- every case runs finite through both precisions, every gradient tensor is live, and the float32 restatement lies within 1e-5 of the
  float64 twin in both norms (max norm of a time-transform weight: 1e-4, the float32 sinusoid of t = 999) - so that K = 4 times that
  distance is a tight bar for the engine;
- a gradient with ONE element moved by 1e-4 of the tensor's largest passes the rule of
  test_gpu_vit.py::test_backward_fp32_every_gradient_tensor (rel_l2 <= 2e-3) and fails the sweep's bars."""
import numpy as np
import pytest
import torch

import vit_ref
import vit_ref64 as V64
import vit_sweep_cases as VC
from helpers import golden_template, grad_digest_of, load_golden, rel_l2


@pytest.mark.parametrize("case", list(VC.ALL_CASES))
def test_twin_equals_vit_ref_at_float32(case):
    kw, x, t, target, sd = VC.sweep_inputs(case)
    p_o, l_o, g_o = VC.case_refs(case)["f32"]
    p_t, l_t, g_t = V64.loss_and_grads(V64.build(kw, sd, torch.float32), x, t, target)
    assert p_t.dtype == torch.float32 and torch.equal(p_t, p_o)
    assert torch.equal(l_t, l_o)
    assert set(g_t) == set(g_o) and VC.INPUT in g_t and len(g_t) > 20
    for name in g_o:
        assert g_t[name].dtype == torch.float32 and torch.equal(g_t[name], g_o[name]), name
    assert float(p_o.abs().max()) > 0 and all(float(g.abs().max()) > 0 for g in g_o.values())


def test_twin_evaluates_the_sinusoids_in_float64():
    t = torch.tensor([3, 17, 41, 999, 0])
    for dim in (32, 64, 128, 256):
        s64 = V64.Sinusoid(dim, torch.float64)(t)
        i = np.arange(dim // 2, dtype=np.float64)
        a = t.numpy().astype(np.float64)[:, None] / np.power(10000.0, 2 * i / dim)[None, :]
        want = np.stack([np.sin(a), np.cos(a)], -1).reshape(len(t), dim)
        assert s64.dtype == torch.float64 and float(np.abs(s64.numpy() - want).max()) < 1e-12
        assert torch.equal(V64.Sinusoid(dim, torch.float32)(t), vit_ref.Sinusoid(dim)(t))


@pytest.mark.parametrize("case", list(VC.SWEEP_CASES))
def test_vit_ref_is_pinned_to_the_reference_on_the_sweep_cases(case):
    """g25_vit_sweep.npz, recorded from the reference's own module: its constructor builds every case, with the state_dict layout of the
    restatement and of the project's module, and ``vit_ref`` reproduces its prediction, loss and gradient digests."""
    from rho_diffusion_amd.models.vit import VisionTransformer
    g = load_golden("g25_vit_sweep.npz")
    kw, x, t, target, sd = VC.sweep_inputs(case)
    assert {k: tuple(v.shape) for k, v in golden_template(g, case).items()} == {k: tuple(v.shape) for k, v in sd.items()}
    model = VisionTransformer(**kw, compute_dtype="fp32")
    assert [f"{k}|{','.join(str(s) for s in v.shape)}" for k, v in model.state_dict().items()] == [str(s) for s in g[f"{case}/keys"]]
    ref = vit_ref.build(kw, sd)
    pred = ref(x, t)
    loss = torch.nn.functional.mse_loss(pred, target)
    loss.backward()
    assert rel_l2(pred, torch.from_numpy(g[f"{case}/pred"])) < 1e-5
    assert abs(float(loss.detach()) - float(g[f"{case}/loss"])) < 1e-5 * float(g[f"{case}/loss"])
    n = 0
    for name, p in ref.named_parameters():
        d, rec = grad_digest_of(p.grad), g[f"{case}/grad/{name}"]
        assert abs(d[0] - rec[0]) <= 1e-4 * rec[0] + 1e-6, name
        assert np.max(np.abs(d[2:] - rec[2:])) <= 1e-4 * max(rec[0] / np.sqrt(p.numel()), 1e-7) * 10 + 1e-6, name
        n += 1
    assert n == len(g[f"{case}/keys"])


@pytest.mark.parametrize("case", list(VC.ALL_CASES))
def test_case_is_finite_live_and_tight(case):
    refs = VC.case_refs(case)
    (p64, l64, g64), (p32, l32, g32) = refs["f64"], refs["f32"]
    assert p64.dtype == torch.float64 and p32.dtype == torch.float32
    assert all(g.dtype == torch.float64 for g in g64.values())
    for run in (refs["f64"], refs["f32"]):
        assert bool(torch.isfinite(run[0]).all()) and bool(torch.isfinite(run[1]))
        assert all(bool(torch.isfinite(g).all()) for g in run[2].values())
    G, kinds = VC.classify(g64)                      # raises on a tensor between the two rules
    assert all(k == "live" for k in kinds.values()), [n for n, k in kinds.items() if k != "live"]
    worst = [0.0, None, 0.0, None]
    for name in ["<prediction>"] + list(kinds):
        a64, a32 = (p64, p32) if name == "<prediction>" else (g64[name], g32[name])
        e = VC.tensor_errors(a32, a64, a32)
        r2, rm = e["l2"] / e["n_l2"], e["max"] / e["n_max"]
        if r2 > worst[0]:
            worst[:2] = [r2, name]
        if rm > worst[2]:
            worst[2:] = [rm, name]
        # max norm: a float32 sinusoid of t = 999 carries an argument error of up to 999 * 2^-24 = 6e-5 into the one gradient element
        # that multiplies it (1.6e-5 on n1_token's time_transform weights); everything else stays below 1e-5 there as well
        assert r2 < 1e-5 and rm < (1e-4 if "time_transform" in name else 1e-5), (name, r2, rm)
    print(f"{case}: {len(kinds)} tensors; float32 restatement vs float64: rel-l2 <= {worst[0]:.2e} ({worst[1]}), "
          f"max / max|g| <= {worst[2]:.2e} ({worst[3]}); loss {float(l64):.6f}")


def _old_rule_accepts(got: torch.Tensor, ref: torch.Tensor) -> bool:
    """The per-tensor rule of test_gpu_vit.py::test_backward_fp32_every_gradient_tensor."""
    return rel_l2(got, ref) <= 2e-3


@pytest.mark.parametrize("case", list(VC.SWEEP_CASES))
def test_single_element_mutation_is_caught_by_the_new_bars_only(case):
    refs = VC.case_refs(case)
    g64, g32 = refs["f64"][2], refs["f32"][2]
    cands = [n for n in g64 if n.endswith("weight") and g64[n].numel() > 6]
    for name in (cands[0], cands[-1]):
        g = g32[name]
        assert VC.within_bars(VC.tensor_errors(g, g64[name], g)) and _old_rule_accepts(g, g)         # unmutated: both accept
        bad = g.clone().reshape(-1)
        idx = max(6, bad.numel() // 2)
        bad[idx] += 1e-4 * float(g.abs().max())
        bad = bad.reshape(g.shape)
        e = VC.tensor_errors(bad, g64[name], g)
        assert _old_rule_accepts(bad, g), name                             # the gap ...
        assert not VC.within_bars(e), VC.describe(case, "cpu", name, e)    # ... closed
        assert e["argmax"] == tuple(int(i) for i in np.unravel_index(idx, tuple(g.shape)))
