"""-m gpu: the state machine of UNetEngine - plans cached by key, prepared weights refreshed by a version sum, ``backward()`` bound
to the most recent training forward - on a tiny2d-sized fp32 model at two shapes, A = (2, 1, 16, 16) and B = (3, 1, 8, 24).

The reference is the float64 twin (tests/unet_ref64.py) run on whatever weights are current, at the bars of
tests/unet_sweep_cases.py (K = 4 times the float32 oracle's own distance from float64 + 16 ulps, per tensor, both norms).  The
library's deterministic switch is on for the whole module (restored afterwards): there results must also be bit-equal to those of a
freshly built model holding the same weights, which a stale buffer or a plan of another shape cannot be."""
import functools

import pytest
import torch

import unet_sweep_cases as SC
from detdata import det_normal, det_state_dict
from golden_cfg import UNET_CASES
from gpu_util import DEV
from helpers import rel_l2

pytestmark = pytest.mark.gpu

KW = dict(UNET_CASES["tiny2d"][0])
SHAPES = {"A": (2, 1, 16, 16), "B": (3, 1, 8, 24)}


@pytest.fixture(autouse=True)
def deterministic():
    from rho_diffusion_amd.engine import ops
    old = ops.set_deterministic(True)
    yield
    ops.set_deterministic(old)


@functools.lru_cache(maxsize=None)
def inputs(which: str):
    shape = SHAPES[which]
    x = det_normal(shape, f"lc{which}x")
    t = torch.tensor([(37 * i + 11) % 1000 for i in range(shape[0])])
    return x, t, det_normal(shape, f"lc{which}tgt")


@functools.lru_cache(maxsize=None)
def weights(salt: str = "lifecycle0"):
    return det_state_dict(SC.state_template(KW), salt)


@functools.lru_cache(maxsize=None)
def refs_of(which: str, salt: str = "lifecycle0"):
    """Forward + backward references at a shape for one of the deterministic weight sets, computed once."""
    x, t, target = inputs(which)
    return SC.reference_runs(KW, x, t, None, None, weights(salt), target)


def build(sd=None):
    from rho_diffusion_amd.models import UNet
    model = UNet(**KW, compute_dtype="fp32")
    model.load_state_dict(sd if sd is not None else weights())
    return model.to(DEV)


def current_weights(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def train_forward(model, which):
    from rho_diffusion_amd.autograd import mse_loss
    x, t, target = inputs(which)
    model.train()
    pred = model(x.to(DEV), t.to(DEV))
    return pred, mse_loss(pred, target.to(DEV))


def grads_of(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def train_step(model, which):
    """zero_grad, forward, backward -> (prediction, loss, gradients)."""
    model.zero_grad(set_to_none=False)
    pred, loss = train_forward(model, which)
    loss.backward()
    return pred.detach().clone(), loss.detach().clone(), grads_of(model)


def infer(model, which):
    x, t, _ = inputs(which)
    model.eval()
    with torch.no_grad():
        return model(x.to(DEV), t.to(DEV)).clone()


def same(a, b) -> bool:
    if isinstance(a, dict):
        return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    return torch.equal(a, b)


def check_pred_on_current_weights(model, which, pred, what):
    x, t, _ = inputs(which)
    SC.check_against_refs("lifecycle" + which, "fp32", SC.reference_preds(KW, x, t, None, None, current_weights(model)), pred, None, None, what)


# ----------------------------------------------------------------------------- plans
def test_plan_alternation_train_and_inference():
    model = build()
    a1 = train_step(model, "A")
    b1 = train_step(model, "B")
    a2 = train_step(model, "A")
    for which, r, what in (("A", a1, "first A"), ("B", b1, "B between"), ("A", a2, "second A")):
        SC.check_against_refs("lifecycle" + which, "fp32", refs_of(which), *r, what=what)
    assert all(same(u, v) for u, v in zip(a1, a2)), "the second pass over shape A differs from the first"
    ia, ib, ia2, ib2 = infer(model, "A"), infer(model, "B"), infer(model, "A"), infer(model, "B")
    for which, p in (("A", ia), ("B", ib), ("A", ia2), ("B", ib2)):
        SC.check_against_refs("lifecycle" + which, "fp32", refs_of(which), p, None, None, what="inference, interleaved")
    assert same(ia, ia2) and same(ib, ib2)
    b2 = train_step(model, "B")                          # a training plan again, after inference plans ran at both shapes
    assert all(same(u, v) for u, v in zip(b1, b2))
    fresh = build()
    fb = train_step(fresh, "B")                          # a model that has seen nothing else
    assert all(same(u, v) for u, v in zip(b1, fb)), "shape B after shape A differs from shape B on a fresh model"
    assert same(infer(build(), "A"), ia)


def test_inference_between_training_forward_and_backward():
    model = build()
    model.zero_grad(set_to_none=False)
    pred, loss = train_forward(model, "A")
    x_a, t_a, _ = inputs("A")
    x_b, t_b, _ = inputs("B")
    with torch.no_grad():                                 # sampling for a progress picture in the middle of a step
        pa = model(x_a.to(DEV), t_a.to(DEV)).clone()
        pb = model(x_b.to(DEV), t_b.to(DEV)).clone()
    loss.backward()
    got = (pred.detach().clone(), loss.detach().clone(), grads_of(model))
    SC.check_against_refs("lifecycleA", "fp32", refs_of("A"), *got, what="backward after two inference forwards")
    SC.check_against_refs("lifecycleA", "fp32", refs_of("A"), pa, None, None, what="inference A inside the step")
    SC.check_against_refs("lifecycleB", "fp32", refs_of("B"), pb, None, None, what="inference B inside the step")
    assert all(same(u, v) for u, v in zip(got, train_step(build(), "A")))


@pytest.mark.parametrize("how", ["one_after_the_other", "summed"])
@pytest.mark.parametrize("second", ["A", "B"], ids=["same_shape", "other_shape"])
def test_backward_of_an_older_training_forward_raises(second, how):
    """The engine keeps the activations of ONE training forward.  A backward that belongs to an older one must raise - before this
    rule it ran on the newer forward's activations (same shape) or on another plan (other shape) and returned wrong gradients."""
    from rho_diffusion_amd.hip import RhoHipError
    model = build()
    model.zero_grad(set_to_none=False)
    _, loss1 = train_forward(model, "A")
    pred2, loss2 = train_forward(model, second)
    if how == "summed":
        with pytest.raises(RhoHipError, match="most recent"):
            (loss1 + loss2).backward()
        return
    with pytest.raises(RhoHipError, match="most recent"):
        loss1.backward()
    assert all(float(p.grad.abs().max()) == 0.0 for p in model.parameters() if p.grad is not None)      # it raised before any launch
    loss2.backward()                                      # the most recent forward is still whole
    got = (pred2.detach().clone(), loss2.detach().clone(), grads_of(model))
    SC.check_against_refs("lifecycle" + second, "fp32", refs_of(second), *got, what="backward of the most recent forward")
    again = train_step(model, second)                     # and forward, backward, forward, backward goes on as before
    assert all(same(u, v) for u, v in zip(got, again))


# ----------------------------------------------------------------------------- weights
def _moved(model, which, before, what):
    after = infer(model, which)
    check_pred_on_current_weights(model, which, after, what)
    d = rel_l2(after, before)
    assert d > 1e-2, (what, d)
    return after


@pytest.mark.parametrize("kind", ["hip_adamw", "torch_sgd"])
def test_forward_after_an_optimizer_step(kind):
    from rho_diffusion_amd.optim import HipAdamW
    model = build()
    opt = HipAdamW(model.parameters(), lr=1e-4) if kind == "hip_adamw" else torch.optim.SGD(model.parameters(), lr=0.01)
    prev = {w: infer(model, w) for w in SHAPES}
    for step in range(2):                                 # the first step may move storage (the arena), the second only bumps versions
        opt.zero_grad()
        pred, loss = train_forward(model, "A")
        loss.backward()
        opt.step()
        for w in SHAPES:
            prev[w] = _moved(model, w, prev[w], f"{kind} step {step}, shape {w}")
    got = train_step(model, "A")                          # the training plan sees the new weights as well
    x, t, target = inputs("A")
    SC.check_against_refs("lifecycleA", "fp32", SC.reference_runs(KW, x, t, None, None, current_weights(model), target), *got,
                          what=f"training step after {kind}")


def test_forward_after_load_state_dict_and_in_place_writes():
    model = build()
    prev = {w: infer(model, w) for w in SHAPES}
    train_step(model, "A")
    model.load_state_dict(weights("lifecycle1"))
    for w in SHAPES:
        prev[w] = _moved(model, w, prev[w], f"load_state_dict, shape {w}")
    got = train_step(model, "A")
    SC.check_against_refs("lifecycleA", "fp32", refs_of("A", "lifecycle1"), *got, what="training step after load_state_dict")
    assert all(same(u, v) for u, v in zip(got, train_step(build(weights("lifecycle1")), "A")))
    # one conv weight through an in-place torch op: the version counter sees it
    name = "input_blocks.1.0.in_layers.2.weight"
    p = dict(model.named_parameters())[name]
    with torch.no_grad():
        p.copy_(weights("lifecycle2")[name].to(DEV))
    for w in SHAPES:
        prev[w] = _moved(model, w, prev[w], f"p.copy_ on {name}, shape {w}")
    # ... and through p.data, which no version counter sees: refresh_weights(force=True) is the documented way
    name = "input_blocks.1.0.out_layers.3.weight"
    p = dict(model.named_parameters())[name]
    p.data.copy_(weights("lifecycle2")[name].to(DEV))
    model.engine().refresh_weights(force=True)
    for w in SHAPES:
        prev[w] = _moved(model, w, prev[w], f"p.data write on {name} + refresh_weights(force=True), shape {w}")


def test_ema_forward_follows_every_update():
    """The shadow weights are written through raw pointers: every ``update()`` has to reach the shadow model's prepared conv weights,
    not only the first one after a forward (which moves the shadow into its arena, and a storage move is seen in any case)."""
    from rho_diffusion_amd.ema import ExponentialMovingAverage
    model = build().eval()
    ema = ExponentialMovingAverage(model, decay=0.9999)
    x, t, _ = inputs("A")
    xd, td = x.to(DEV), t.to(DEV)

    def ema_pred():
        with torch.no_grad():
            return ema(xd, td).clone()

    prev = ema_pred()
    SC.check_against_refs("lifecycleA", "fp32", refs_of("A"), prev, None, None, what="EMA before any update")
    for rnd, salt in enumerate(("lifecycle1", "lifecycle2", "lifecycle3")):
        model.load_state_dict(weights(salt))              # the live weights move ...
        ema.update()
        ema.update()                                      # ... and the shadow follows (the warm-up fraction is ~1e-3: almost all the way)
        now = ema_pred()
        shadow = current_weights(ema.ema_model)
        SC.check_against_refs("lifecycleA", "fp32", SC.reference_preds(KW, x, t, None, None, shadow), now, None, None,
                              what=f"EMA after update round {rnd}")
        d = rel_l2(now, prev)
        assert d > 1e-2, (rnd, d)
        prev = now
