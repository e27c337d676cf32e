"""CPU only: the float64 twin of the UNetv2 oracle (tests/unet_ref64.py) and the case table of the whole-UNet sweep
(tests/unet_sweep_cases.py).

- the twin at float32 IS the oracle: ``torch.equal`` on the prediction and on every autograd gradient, on recorded golden cases;
- every sweep case runs finite through both, every gradient tensor is live or an exact-invariance zero (nothing in between, at
  most a third zeros), and the float32 oracle lies within 1e-5 of the float64 twin in both norms - so that K = 4 times that
  distance is a tight bar for the engine;
- a gradient with ONE element moved by 1e-4 of the tensor's largest passes the digest rule of
  test_gpu_training.py::test_unet_backward_fp32_vs_reference_golden (norm within 2e-3, six leading values) and fails the sweep's bars."""
import numpy as np
import pytest
import torch

import unet_ref64 as R64
import unet_sweep_cases as SC
from helpers import golden_template, grad_digest_of, load_golden
from oracle import ref_torch as R


@pytest.mark.parametrize("case", list(SC.TWIN_CASES))
def test_twin_equals_oracle_at_float32(case):
    cfg, x, t, y, ps, sd = SC.sweep_inputs(case)
    target = SC.target_of(case, x.shape)
    p_o, l_o, g_o = R64.loss_and_grads(R.unet_forward, sd, cfg, x, t, y, ps, target, torch.float32)
    p_t, l_t, g_t = R64.loss_and_grads(R64.unet_forward, sd, cfg, x, t, y, ps, target, torch.float32)
    assert p_t.dtype == torch.float32 and torch.equal(p_t, p_o)
    assert torch.equal(l_t, l_o)
    assert set(g_t) == set(g_o) and len(g_t) > 20
    for name in g_o:
        assert torch.equal(g_t[name], g_o[name]), name
    assert float(p_o.abs().max()) > 0 and sum(float(g.abs().max()) > 0 for g in g_o.values()) > 20


@pytest.mark.parametrize("case", list(SC.TWIN_CASES))
def test_template_matches_recorded_keys(case):
    """state_template re-derives the reference's state_dict layout: the same names and shapes as the key lists recorded from it."""
    g = load_golden("g15_updown.npz" if case == "updown2d_3lvl" else "g4_unet.npz")
    want = {k: tuple(v.shape) for k, v in golden_template(g, case).items()}
    got = {k: tuple(v.shape) for k, v in SC.state_template(SC.ALL_CASES[case][0]).items()}
    assert got == want


@pytest.mark.parametrize("case", list(SC.SWEEP_CASES))
def test_oracle_matches_reference_on_the_sweep_cases(case):
    """g24_unet_sweep.npz, recorded from the reference's own module: its constructor builds every case, with the state_dict layout
    ``state_template`` derives, and the float32 oracle reproduces its prediction, loss and gradient digests (the tolerances of
    test_oracle_golden.py, plus the six leading values)."""
    g = load_golden("g24_unet_sweep.npz")
    assert {k: tuple(v.shape) for k, v in golden_template(g, case).items()} == \
        {k: tuple(v.shape) for k, v in SC.state_template(SC.SWEEP_CASES[case][0]).items()}
    pred, loss, grads = SC.case_refs(case)["f32"]
    gold = torch.from_numpy(g[f"{case}/pred"])
    assert tuple(pred.shape) == tuple(gold.shape) and float((pred - gold).norm() / gold.norm()) < 1e-5
    assert abs(float(loss) - float(g[f"{case}/loss"])) < 1e-5
    n = 0
    for name, grad in grads.items():
        ref = g[f"{case}/grad/{name}"]
        d = grad_digest_of(grad)
        rms = ref[0] / np.sqrt(grad.numel())
        assert abs(d[0] - ref[0]) <= 1e-4 * ref[0] + 1e-6, name
        assert np.max(np.abs(d[2:] - ref[2:])) <= 1e-4 * max(rms, 1e-7) * 10 + 1e-6, name
        n += 1
    assert n == len([k for k in g.files if k.startswith(f"{case}/grad/")])


@pytest.mark.parametrize("case", list(SC.SWEEP_CASES))
def test_template_matches_module(case):
    """... and, for the new cases, as the project's own module tree (built on the CPU: no engine involved)."""
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    kw, _, ykind = SC.SWEEP_CASES[case]
    model = UNet(**dict(kw), compute_dtype="fp32")
    if ykind == "multi":
        model.cond_fn = MultiEmbeddings(parameter_space=SC.PARAM_SPACE, embedding_dim=4 * kw["model_channels"])
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in SC.state_template(kw).items()}
    assert got == want


@pytest.mark.parametrize("case", list(SC.SWEEP_CASES))
def test_case_is_finite_classified_and_tight(case):
    refs = SC.case_refs(case)
    (p64, l64, g64), (p32, l32, g32) = refs["f64"], refs["f32"]
    assert p64.dtype == torch.float64 and p32.dtype == torch.float32
    for run in (refs["f64"], refs["f32"]):
        assert bool(torch.isfinite(run[0]).all()) and bool(torch.isfinite(run[1]))
        assert all(bool(torch.isfinite(g).all()) for g in run[2].values())
    G, kinds = SC.classify(g64)                      # raises on a tensor between the two rules
    zeros = [n for n, k in kinds.items() if k == "zero"]
    assert 3 * len(zeros) <= len(kinds), (len(zeros), len(kinds))
    worst = [0.0, None, 0.0, None]
    for name, k in [("<prediction>", "live")] + list(kinds.items()):
        if k != "live":
            continue
        a64, a32 = (p64, p32) if name == "<prediction>" else (g64[name], g32[name])
        e = SC.tensor_errors(a32, a64, a32)
        r2, rm = e["l2"] / e["n_l2"], e["max"] / e["n_max"]
        if r2 > worst[0]:
            worst[:2] = [r2, name]
        if rm > worst[2]:
            worst[2:] = [rm, name]
        assert r2 < 1e-5 and rm < 1e-5, (name, r2, rm)
    print(f"{case}: {len(kinds)} tensors, {len(zeros)} exact zeros; float32 oracle vs float64: rel-l2 <= {worst[0]:.2e} ({worst[1]}), "
          f"max / max|g| <= {worst[2]:.2e} ({worst[3]}); loss {float(l64):.6f}")


def _digest_rule_accepts(got: torch.Tensor, ref: torch.Tensor) -> bool:
    """The per-tensor rule of test_gpu_training.py::test_unet_backward_fp32_vs_reference_golden, on digests [norm, sum, first six]."""
    d, r = grad_digest_of(got), grad_digest_of(ref)
    rms = r[0] / np.sqrt(ref.numel())
    if abs(d[0] - r[0]) > 2e-3 * r[0] + 1e-6:
        return False
    return not np.max(np.abs(d[2:] - r[2:])) > 2e-3 * max(rms, 1e-7) * 10 + 1e-6


@pytest.mark.parametrize("case", list(SC.SWEEP_CASES))
def test_single_element_mutation_is_caught_by_the_new_bars_only(case):
    refs = SC.case_refs(case)
    g64, g32 = refs["f64"][2], refs["f32"][2]
    _, kinds = SC.classify(g64)
    cands = [n for n in g64 if kinds[n] == "live" and n.endswith("weight") and g64[n].numel() > 6]
    for name in (cands[0], cands[-1]):
        g = g32[name]
        assert SC.within_bars(SC.tensor_errors(g, g64[name], g)) and _digest_rule_accepts(g, g)      # unmutated: both accept
        bad = g.clone().reshape(-1)
        idx = max(6, bad.numel() // 2)
        bad[idx] += 1e-4 * float(g.abs().max())
        bad = bad.reshape(g.shape)
        e = SC.tensor_errors(bad, g64[name], g)
        assert _digest_rule_accepts(bad, g), name                          # the gap ...
        assert not SC.within_bars(e), SC.describe(case, "cpu", name, e)    # ... closed
        assert e["argmax"] == tuple(int(i) for i in np.unravel_index(idx, tuple(g.shape)))
