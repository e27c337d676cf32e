"""-m gpu: forward + backward of the whole fp32 UNet engine against the float64 twin of the oracle (tests/unet_ref64.py), per tensor,
on the configurations of tests/unet_sweep_cases.py (the plan builders' branches no recorded golden reaches) and under both launch
paths of test_gpu_training.PATHS.

Every parameter gradient, the prediction and the loss are held against float64 in both norms; the float32 oracle only sizes the
bound (K = 4 times its own distance from float64, plus 16 float32 ulps of the tensor's size - the constants of
tests/test_gpu_sinkhorn.py) and is never the code under test.  A tensor whose float64 gradient is an exact-invariance zero must
stay below 1e-5 of the global gradient norm.  A failure names case, path, tensor, both norms and the index of the worst element.

MEASURED on an MI355X: worst err / (the float32 oracle's own error) over prediction, loss and every live gradient, per case, as
"l2 ratio | max-norm ratio", launch path phased / small_grid where they differ; head bias (below) left out:
    odd2d_b3          1.76 / 1.78 | 2.55 / 2.61      (output_blocks.3.0 conv bias / out_layers.0.bias of output_blocks.2.0)
    odd3d_b1          2.66 / 3.23 | 3.58 / 3.68      (GroupNorm weights of middle_block.2 and output_blocks.5.1)
    1d_b5_updown      1.46        | 2.03
    deep4_2d          1.43        | 1.72
    pool2d_add        1.77        | 2.60
    heads_up_new      1.43 / 1.35 | 2.24 / 1.64
    one_level         2.18        | 2.87
    cond3d_b4         1.93 / 2.30 | 2.26 / 2.79
    elu_updown3d_odd  2.87 (loss) | 4.35             (output_blocks.3.0.in_layers.0.weight, element 2; l2 ratio of that tensor 2.5)
Every tensor meets K = 4 plus the floor.  The 4.35 is inside the floor: a 32-element GroupNorm weight whose
float32-oracle error happens to be 0.5e-6 of max|g| at its worst element (its usual size is 2 - 3e-6, see the host test's
printout), against 2.3e-6 for the engine; bound 6.4e-8, error 4.8e-8.

THE HEAD BIAS (``out.2.bias``), K = 16.  Measured ratios: 4.75 (pool2d_add, both paths), 7.86 (deep4_2d, small_grid), at most 1.7
elsewhere.  d loss / d bias[c] = (2 / numel) * sum over (n, positions) of (pred - target): with a one-channel head it is ONE number,
the mean of a few hundred residuals of either sign - on pool2d_add 240 terms with sum |terms| = 116 * |sum|.  What reaches it is the
FORWARD's float32 error in ``pred`` (about 1e-6 of each element, for the engine as for the oracle: the prediction's own ratio is 1.2 -
1.6) carried through that cancellation; the backward kernel only adds up exact-to-an-ulp terms.  Engine and oracle therefore err by
two independent draws of the same size, and the ratio of two such draws for a single number has no moderate bound (for two
half-normals P(ratio > 4) = (2 / pi) atan(1 / 4) = 16 %): on pool2d_add the oracle's draw is 1.2e-6 of |g| and the engine's 5.5e-6,
which K = 4 plus the floor admits by less than one float32 ulp of g (error 8.964e-8, bound 9.106e-8) - and the channel sums are
accumulated by float32 atomics whose order may differ from run to run.  Following the rule of this suite for a tensor class whose
ratio exceeds K (the next power of two above twice the measured ratio: 2 * 7.86 -> 16), ``out.2.bias`` alone is held to K = 16; the
formula and the floor are unchanged, and every other tensor keeps K = 4.
"""
import pytest
import torch

import unet_sweep_cases as SC
from gpu_util import DEV
from test_gpu_training import PATHS

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(PATHS), ids=list(PATHS))
def launch_path(request, monkeypatch):
    for k, v in PATHS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def build_model(case: str, sd=None):
    """The project's UNet for a sweep case with the case's deterministic weights (or ``sd``), fp32 engine, on the device."""
    from rho_diffusion_amd.models import MultiEmbeddings, UNet
    kw, _, ykind = SC.ALL_CASES[case]
    model = UNet(**dict(kw), compute_dtype="fp32")
    if ykind == "multi":
        model.cond_fn = MultiEmbeddings(parameter_space=SC.PARAM_SPACE, embedding_dim=4 * kw["model_channels"])
    model.load_state_dict(sd if sd is not None else SC.sweep_inputs(case)[5])
    return model.to(DEV)


def train_step(model, x, t, y, target):
    """(prediction, loss, {name: gradient}) of one forward + backward in training mode; gradients are what the step ADDED to p.grad
    (the caller zeroes them)."""
    from rho_diffusion_amd.autograd import mse_loss
    model.train()
    pred = model(x.to(DEV), t.to(DEV), y.to(DEV) if y is not None else None)
    loss = mse_loss(pred, target.to(DEV))
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return pred.detach().clone(), loss.detach().clone(), grads


@pytest.mark.parametrize("case", list(SC.SWEEP_CASES))
def test_unet_fp32_per_tensor_vs_float64(case, launch_path):
    cfg, x, t, y, ps, sd = SC.sweep_inputs(case)
    refs = SC.case_refs(case)
    model = build_model(case)
    assert set(n for n, _ in model.named_parameters()) == set(refs["f64"][2])
    pred, loss, grads = train_step(model, x, t, y, SC.target_of(case, refs["f64"][0].shape))
    assert pred.dtype == torch.float32 and tuple(pred.shape) == tuple(refs["f64"][0].shape)
    assert bool(torch.isfinite(pred).all()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    SC.check_against_refs(case, launch_path, refs, pred, loss, grads)
