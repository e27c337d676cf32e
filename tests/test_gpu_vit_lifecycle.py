"""-m gpu: the caches and launch-time lookups of models/vit.py - ``_Gemm.prepared`` keyed on (data_ptr, version, dtype), the positional
table keyed on the version counters and one data pointer, gradients written into whatever ``p.grad`` is at launch time, activations
kept per training forward - on a vit2d-sized fp32 model.

Every result is held against the float64 twin (tests/vit_ref64.py) run on the weights current at that moment, at the bars of
tests/vit_sweep_cases.py (K = 4 times the float32 restatement's own distance from float64 + 16 ulps, per tensor, both norms).  The
library's deterministic switch is on for the whole module (restored afterwards): there a result must also be bit-equal to that of a
freshly built model loaded with the same weights, which a stale layout, a stale positional table or another forward's activations
cannot be.

Three defects were found here and fixed in models/vit.py (each test named was seen failing on an MI355X against the sources before):
``test_frozen_parameters_get_no_gradient`` (block, pos_embedding, norms_and_output_bias: ``_grad_of`` allocated and wrote ``.grad`` of parameters with
requires_grad False); ``test_forward_and_backward_follow_a_weight_change[load_state_dict_assign]`` and ``[replace_parameter]`` (a
``_Gemm`` held its parameter OBJECT: once the module got another one it went on serving the old weights and the new parameter got no
gradient); ``[data_assign_pos_bias]`` (the positional table's key had the weight's data pointer and not the bias's)."""
import functools

import pytest
import torch

import vit_ref
import vit_sweep_cases as VC
from detdata import det_normal, det_state_dict
from gpu_util import DEV
from helpers import rel_l2
from vit_cfg import VIT_CASES

pytestmark = pytest.mark.gpu

CASE = "vit2d"
KW = dict(VIT_CASES[CASE][0])
F32_TOL = 1e-4                                  # test_gpu_vit.py
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def deterministic():
    from rho_diffusion_amd.engine import ops
    old = ops.set_deterministic(True)
    yield
    ops.set_deterministic(old)


@functools.lru_cache(maxsize=None)
def inputs(B: int, salt: str = "a"):
    shape = (B, KW["num_channels"], *KW["input_shapes"])
    return det_normal(shape, f"vlc{salt}{B}x"), torch.tensor(VC.TIMESTEPS[:B]), det_normal(shape, f"vlc{salt}{B}tgt")


@functools.lru_cache(maxsize=None)
def weights(salt: str = "vlc0"):
    return det_state_dict(VC.state_template(KW), salt)


@functools.lru_cache(maxsize=None)
def refs_of(B: int, salt: str = "vlc0", isalt: str = "a"):
    """Forward + backward references at a batch size for one of the deterministic weight sets, computed once."""
    x, t, target = inputs(B, isalt)
    return VC.reference_runs(KW, x, t, target, weights(salt))


def build(sd=None, dtype="fp32"):
    from rho_diffusion_amd.models.vit import VisionTransformer
    model = VisionTransformer(**KW, compute_dtype=dtype)
    model.load_state_dict(sd if sd is not None else weights())
    return model.to(DEV)


def current_weights(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def train_forward(model, B, isalt="a"):
    """(input on the device, prediction, loss) of a training-mode forward."""
    from rho_diffusion_amd.autograd import mse_loss
    x, t, target = inputs(B, isalt)
    model.train()
    xd = x.to(DEV).requires_grad_(True)
    pred = model(xd, t.to(DEV))
    return xd, pred, mse_loss(pred, target.to(DEV))


def grads_of(model, xd=None):
    g = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    if xd is not None:
        g[VC.INPUT] = xd.grad.detach().clone()
    return g


def train_step(model, B, isalt="a"):
    """zero_grad, forward, backward -> (prediction, loss, gradients)."""
    model.zero_grad(set_to_none=False)
    xd, pred, loss = train_forward(model, B, isalt)
    loss.backward()
    return pred.detach().clone(), loss.detach().clone(), grads_of(model, xd)


def infer(model, B, isalt="a"):
    x, t, _ = inputs(B, isalt)
    model.eval()
    with torch.no_grad():
        return model(x.to(DEV), t.to(DEV)).clone()


def same(a, b) -> bool:
    if isinstance(a, dict):
        return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    return torch.equal(a, b)


def same_step(r1, r2) -> bool:
    return all(same(u, v) for u, v in zip(r1, r2))


def settled_pred(model, B, pred, what):
    """An inference result on the weights the model holds NOW: within the bars of the float64 twin, and the bits of a fresh model."""
    x, t, _ = inputs(B)
    sd = current_weights(model)
    VC.check_against_refs(CASE, "fp32", VC.reference_preds(KW, x, t, sd), pred, None, None, what)
    assert same(pred, infer(build(sd), B)), f"{what}: differs from a freshly built model with the same weights"


def settled_step(model, B, got, what):
    x, t, target = inputs(B)
    sd = current_weights(model)
    VC.check_against_refs(CASE, "fp32", VC.reference_runs(KW, x, t, target, sd), *got, what=what)
    assert same_step(got, train_step(build(sd), B)), f"{what}: differs from a freshly built model with the same weights"


def fill_caches(model, B=3):
    """An inference forward (positional table, forward layouts) and a training step (both layouts of every _Gemm)."""
    before = infer(model, B)
    train_step(model, B)
    assert model._pos_cache is not None and all(g._key is not None for g in gemms(model))
    return before


def gemms(model):
    out = [model.patch_embedder._gemm, model._oproj, model._oconv]
    for blk in model.transformer_blocks:
        out += [blk._qkv, blk._proj, blk._lin1, blk._lin2]
    return out


# ----------------------------------------------------------------------------- weights
def test_eval_forward_after_hipadamw_steps():
    """The arena re-homes every parameter (data pointers move, version counters do not); a later step only bumps versions."""
    from rho_diffusion_amd.optim import HipAdamW
    model = build()
    prev = fill_caches(model)
    settled_pred(model, 3, prev, "before any step")
    ptr0 = model.pos_embedding[1].weight.data_ptr()
    opt = HipAdamW(model.parameters(), lr=1e-2)
    for step in range(2):
        ptr = model.pos_embedding[1].weight.data_ptr()
        opt.zero_grad()
        xd, pred, loss = train_forward(model, 3)
        loss.backward()
        opt.step()
        assert (model.pos_embedding[1].weight.data_ptr() != ptr0) and (step == 0 or model.pos_embedding[1].weight.data_ptr() == ptr)
        now = infer(model, 3)
        settled_pred(model, 3, now, f"HipAdamW step {step}")
        assert rel_l2(now, prev) > 1e-3, (step, rel_l2(now, prev))
        prev = now
    settled_step(model, 3, train_step(model, 3), "training step after two HipAdamW steps")


def _change(model, how):
    params = dict(model.named_parameters())
    other = weights("vlc1")
    if how == "load_state_dict":
        model.load_state_dict(other)
        return
    if how == "load_state_dict_assign":                      # every parameter becomes ANOTHER object
        model.load_state_dict({k: v.to(DEV) for k, v in other.items()}, assign=True)
        return
    name = {"copy_pos_bias": "pos_embedding.1.bias", "copy_in_proj": "transformer_blocks.1.attention_layer.in_proj_weight",
            "copy_time_weight": "transformer_blocks.0.time_transform.1.weight", "data_assign": "transformer_blocks.1.linear_block.0.weight",
            "data_assign_pos_bias": "pos_embedding.1.bias",
            "replace_parameter": "transformer_blocks.0.attention_layer.out_proj.weight"}[how]
    new = (other[name] + (1.0 if "pos_bias" in how else 0.0)).to(DEV)
    if how == "replace_parameter":
        model.transformer_blocks[0].attention_layer.out_proj.weight = torch.nn.Parameter(new.clone())
    elif how.startswith("data_assign"):
        params[name].data = new.clone()
    else:
        with torch.no_grad():
            params[name].copy_(new)


@pytest.mark.parametrize("how", ["load_state_dict", "copy_pos_bias", "copy_in_proj", "copy_time_weight", "data_assign",
                                 "data_assign_pos_bias", "load_state_dict_assign", "replace_parameter"])
def test_forward_and_backward_follow_a_weight_change(how):
    model = build()
    before = fill_caches(model)
    _change(model, how)
    after = infer(model, 3)
    settled_pred(model, 3, after, how)
    assert rel_l2(after, before) > 1e-3, (how, rel_l2(after, before))
    settled_step(model, 3, train_step(model, 3), f"training step after {how}")


def test_alternating_batch_sizes():
    model = build()
    runs = [(B, train_step(model, B)) for B in (2, 3, 2)]
    for B, r in runs:
        VC.check_against_refs(CASE, "fp32", refs_of(B), *r, what=f"training, batch {B}")
    assert same_step(runs[0][1], runs[2][1]), "the second pass at batch 2 differs from the first"
    assert same_step(runs[1][1], train_step(build(), 3)), "batch 3 after batch 2 differs from batch 3 on a fresh model"
    preds = [(B, infer(model, B)) for B in (2, 3, 2)]
    for B, p in preds:
        VC.check_against_refs(CASE, "fp32", refs_of(B), p, None, None, what=f"inference, batch {B}")
    assert same(preds[0][1], preds[2][1]) and same(preds[1][1], infer(build(), 3))


# ----------------------------------------------------------------------------- activations
def test_no_grad_forward_inside_a_training_step():
    model = build()
    model.zero_grad(set_to_none=False)
    xd, pred, loss = train_forward(model, 3)
    pa, pb = infer(model, 3), infer(model, 2)               # sampling for a progress picture in the middle of a step
    model.train()
    loss.backward()
    got = (pred.detach().clone(), loss.detach().clone(), grads_of(model, xd))
    VC.check_against_refs(CASE, "fp32", refs_of(3), *got, what="backward after two inference forwards")
    VC.check_against_refs(CASE, "fp32", refs_of(3), pa, None, None, what="inference inside the step, batch 3")
    VC.check_against_refs(CASE, "fp32", refs_of(2), pb, None, None, what="inference inside the step, batch 2")
    assert same_step(got, train_step(build(), 3))


@pytest.mark.parametrize("order", ["ab", "ba"])
@pytest.mark.parametrize("second", [3, 2], ids=["same_batch", "other_batch"])
def test_two_training_forwards_before_either_backward(second, order):
    """Each forward keeps its own activations: a backward contributes that forward's gradients whatever ran in between."""
    ga = train_step(build(), 3, "a")
    gb = train_step(build(), second, "b")
    VC.check_against_refs(CASE, "fp32", refs_of(3, isalt="a"), *ga, what="input a alone")
    VC.check_against_refs(CASE, "fp32", refs_of(second, isalt="b"), *gb, what="input b alone")
    model = build()
    model.zero_grad(set_to_none=False)
    xa, pred_a, loss_a = train_forward(model, 3, "a")
    xb, pred_b, loss_b = train_forward(model, second, "b")
    assert same(pred_a.detach(), ga[0]) and same(pred_b.detach(), gb[0])
    first_loss, alone = (loss_a, ga) if order == "ab" else (loss_b, gb)
    first_loss.backward()
    names = [n for n, _ in model.named_parameters()]
    after_first = grads_of(model)
    for n in names:                                         # added to zeros: the bits of the run that had this forward alone
        assert torch.equal(after_first[n], alone[2][n]), (order, n)
    (loss_b if order == "ab" else loss_a).backward()
    assert torch.equal(xa.grad, ga[2][VC.INPUT]) and torch.equal(xb.grad, gb[2][VC.INPUT])
    both = grads_of(model)
    for n in names:
        a64, b64 = ga[2][n].double(), gb[2][n].double()
        err = (both[n].double() - (a64 + b64)).abs()
        bound = 2 * U * (a64.abs() + b64.abs())
        assert bool((err <= bound).all()), (order, n, float((err - bound).max()))


def test_second_backward_through_the_same_forward_raises():
    model = build()
    model.zero_grad(set_to_none=False)
    xd, pred, loss = train_forward(model, 3)
    loss.backward(retain_graph=True)
    got = (pred.detach().clone(), loss.detach().clone(), grads_of(model, xd))
    with pytest.raises(RuntimeError, match="twice"):
        loss.backward()
    assert same(grads_of(model, xd), got[2])                  # it raised before any launch
    assert same_step(got, train_step(build(), 3))


def test_zeroing_modes_give_the_same_parameters():
    """p.grad None (a fresh tensor at the next launch, gathered into the arena by the step), p.grad zeroed in place, and the
    optimizer's own zero_grad: three steps each, the same bits."""
    from rho_diffusion_amd.optim import HipAdamW
    results = []
    for mode in ("none", "zeros", "optimizer"):
        model = build()
        opt = HipAdamW(model.parameters(), lr=1e-3)
        for step in range(3):
            if mode == "optimizer":
                opt.zero_grad()
            else:
                model.zero_grad(set_to_none=(mode == "none"))
            xd, pred, loss = train_forward(model, 3)
            loss.backward()
            opt.step()
        results.append((current_weights(model), infer(model, 3)))
        if mode == "none":
            settled_pred(model, 3, results[-1][1], "after three steps with set_to_none=True")
    for sd, pred in results[1:]:
        assert same(sd, results[0][0]) and same(pred, results[0][1])
    assert rel_l2(results[0][1], infer(build(), 3)) > 1e-4


# ----------------------------------------------------------------------------- copies
def test_ema_shadow_keeps_its_own_layouts():
    """The deep copy carries the live model's prepared layouts and positional table; each side has to follow its own weights only."""
    from rho_diffusion_amd.ema import ExponentialMovingAverage
    from rho_diffusion_amd.optim import HipAdamW
    model = build()
    live0 = fill_caches(model)
    ema = ExponentialMovingAverage(model, decay=0.9999)
    x, t, _ = inputs(3)
    xd, td = x.to(DEV), t.to(DEV)

    def shadow_pred(what):
        with torch.no_grad():
            p = ema(xd, td).clone()
        sd = current_weights(ema.ema_model)
        VC.check_against_refs(CASE, "fp32", VC.reference_preds(KW, x, t, sd), p, None, None, what)
        assert same(p, infer(build(sd), 3)), f"{what}: differs from a fresh model holding the shadow weights"
        return p

    s0 = shadow_pred("shadow before any update")
    assert same(s0, live0)
    opt = HipAdamW(model.parameters(), lr=1e-2)
    opt.zero_grad()
    _, _, loss = train_forward(model, 3)
    loss.backward()
    opt.step()
    assert same(shadow_pred("shadow after a live step, before update()"), s0)
    ema.update()
    s1 = shadow_pred("shadow after update()")
    assert rel_l2(s1, s0) > 1e-3
    live1 = infer(model, 3)
    settled_pred(model, 3, live1, "live model after update()")
    # a live weight changes: the shadow's output keeps its bits
    name = "transformer_blocks.0.linear_block.3.weight"
    with torch.no_grad():
        dict(model.named_parameters())[name].copy_(weights("vlc1")[name].to(DEV))
    live2 = infer(model, 3)
    settled_pred(model, 3, live2, "live model after a live write")
    assert not same(live2, live1) and same(shadow_pred("shadow after a live write"), s1)
    # a shadow weight changes: the live model's output keeps its bits
    with torch.no_grad():
        dict(ema.ema_model.named_parameters())["pos_embedding.1.bias"].add_(1.0)
        dict(ema.ema_model.named_parameters())[name].copy_(weights("vlc2")[name].to(DEV))
    s2 = shadow_pred("shadow after a shadow write")
    assert rel_l2(s2, s1) > 1e-3 and same(infer(model, 3), live2)


def test_standalone_patch_embedding_between_bf16_forwards():
    """``PatchEmbedding.forward`` runs the model's own ``_gemm`` in float32: the bf16 layouts it displaces have to come back."""
    model = build(dtype="bf16")
    x, t, target = inputs(3)
    p1 = infer(model, 3)
    with torch.no_grad():
        tok = model.patch_embedder(x.to(DEV)).clone()
    p2 = infer(model, 3)
    assert same(p1, p2)
    want = vit_ref.build(KW, weights()).patch_embedder.conv_shaper(x).flatten(2).transpose(1, 2)
    assert tok.dtype == torch.float32 and tuple(tok.shape) == tuple(want.shape)
    assert rel_l2(tok, want) < F32_TOL, rel_l2(tok, want)
    assert rel_l2(p1, refs_of(3)["f64"][0]) < 3e-2          # BF16_TOL of test_gpu_vit.py: the bf16 model itself is sane
    # ... and inside a training step, between the forward and its backward
    model.zero_grad(set_to_none=False)
    xd, pred, loss = train_forward(model, 3)
    with torch.no_grad():
        tok2 = model.patch_embedder(x.to(DEV)).clone()
    loss.backward()
    got = (pred.detach().clone(), loss.detach().clone(), grads_of(model, xd))
    assert same(tok2, tok) and same_step(got, train_step(build(dtype="bf16"), 3))


# ----------------------------------------------------------------------------- frozen parameters
@pytest.mark.parametrize("which", ["block", "pos_embedding", "norms_and_output_bias", "everything"])
def test_frozen_parameters_get_no_gradient(which):
    """A parameter with requires_grad False keeps ``.grad`` None (torch's contract; an optimizer built over all parameters would
    otherwise update it), and every other gradient keeps the bits of the unfrozen run."""
    full = train_step(build(), 3)
    model = build()
    prefix = {"block": ("transformer_blocks.0.",), "pos_embedding": ("pos_embedding.",),
              "norms_and_output_bias": ("transformer_blocks.1.norm_1.weight", "transformer_blocks.1.norm_2.bias", "output_conv.bias",
                                        "patch_embedder.conv_shaper.weight"),
              "everything": ("",)}[which]                      # only the input's gradient is left
    frozen = [n for n, p in model.named_parameters() if n.startswith(prefix)]
    assert frozen
    for n, p in model.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    model.zero_grad(set_to_none=True)
    xd, pred, loss = train_forward(model, 3)
    loss.backward()
    params = dict(model.named_parameters())
    for n in frozen:
        assert params[n].grad is None, n
    got = grads_of(model, xd)
    assert set(got) == set(full[2]) - set(frozen)
    assert same(pred.detach(), full[0]) and same(loss.detach(), full[1])
    for n, g in got.items():
        assert torch.equal(g, full[2][n]), n
