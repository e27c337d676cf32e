"""CPU: the host side of the fused optimizers (rho_diffusion_amd/optim.py) - the class map, the constructor signatures, the
keyword rule of configure_optimizers and the state_dict format before the first step.  No kernel runs here."""
import inspect

import pytest
import torch
from torch import nn

from rho_diffusion_amd import optim as O

FUSED = {"AdamW": O.HipAdamW, "Adam": O.HipAdam, "SGD": O.HipSGD, "RMSprop": O.HipRMSprop, "Adagrad": O.HipAdagrad,
         "Adamax": O.HipAdamax, "NAdam": O.HipNAdam, "RAdam": O.HipRAdam, "Adadelta": O.HipAdadelta}


def test_fused_optimizer_class_map():
    for name, cls in FUSED.items():
        assert O.fused_optimizer_class(getattr(torch.optim, name)) is cls
        assert issubclass(cls, torch.optim.Optimizer)
    for name in ("ASGD", "Rprop", "LBFGS", "SparseAdam"):
        assert O.fused_optimizer_class(getattr(torch.optim, name)) is None


@pytest.mark.parametrize("name", sorted(FUSED))
def test_signature_is_the_namesakes_plus_two_keywords(name):
    """Names, kinds (positional / keyword-only), order and defaults; the two extra keywords come last and default to None."""
    def params(cls):
        return [(n, p.kind, p.default) for n, p in inspect.signature(cls.__init__).parameters.items()]
    ours, theirs = params(FUSED[name]), params(getattr(torch.optim, name))
    assert [n for n, _, _ in ours[-2:]] == ["arena_order", "max_grad_norm"] and all(d is None for _, _, d in ours[-2:])
    assert [(n, d) for n, _, d in ours[:-2]] == [(n, d) for n, _, d in theirs]
    for (n, k, _), (_, kt, _) in zip(ours[:-2], theirs):
        assert k == kt, (n, k, kt)                      # what torch takes positionally stays positional


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fresh_state_dict_is_a_fresh_torch_optimizers(name):
    """Before the first step (no arena yet, CPU parameters): same group keys and values, same state (empty, except Adagrad's),
    and the dict loads into the torch class and back."""
    m = nn.Linear(3, 2)
    ours, theirs = FUSED[name](m.parameters()), getattr(torch.optim, name)(m.parameters())
    a, b = ours.state_dict(), theirs.state_dict()
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys()
        for key in a["state"][k]:
            assert torch.equal(a["state"][k][key], b["state"][k][key]), (k, key)
    theirs.load_state_dict(a)


def test_unsupported_options_say_why():
    m = nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match="differentiable"):
        O.HipAdam(m.parameters(), differentiable=True)
    with pytest.raises(ValueError, match="tensor lr"):
        O.HipSGD(m.parameters(), lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="Nesterov"):           # the namesake's own argument checks apply
        O.HipSGD(m.parameters(), nesterov=True)
    with pytest.raises(ValueError, match="max_grad_norm"):
        O.HipAdam(m.parameters(), max_grad_norm=-1.0)
    opt = O.HipAdam(m.parameters(), foreach=True, fused=False, capturable=True)          # accepted and ignored
    assert opt.param_groups[0]["foreach"] is None and opt.param_groups[0]["capturable"] is False
    emb = nn.Embedding(4, 2, sparse=True)
    emb(torch.tensor([1])).sum().backward()
    sgd = O.HipSGD(emb.parameters())
    with pytest.raises(RuntimeError, match="sparse"):
        sgd.step()


class _Pipe:
    """configure_optimizers of the pipeline base class over a tiny CPU module (nothing else of the pipeline is needed)."""

    def __init__(self, optimizer, opt_kwargs):
        from types import SimpleNamespace
        self.optimizer = optimizer
        self.hparams = SimpleNamespace(opt_kwargs=dict(opt_kwargs))
        self.net = nn.Linear(3, 2)

    def parameters(self):
        return self.net.parameters()

    def configure(self, world=1):
        from rho_diffusion_amd.diffusion.abstract_diffusion import AbstractDiffusionPipeline
        return AbstractDiffusionPipeline.configure_optimizers(self, world)["optimizer"]


def test_kwarg_rule_of_configure_optimizers():
    # SGD: the injected betas / eps / amsgrad go, the injected weight_decay stays
    opt = _Pipe(torch.optim.SGD, {"lr": 1e-2, "momentum": 0.9}).configure()
    g = opt.param_groups[0]
    assert type(opt) is O.HipSGD and g["momentum"] == 0.9 and g["weight_decay"] == 1e-2 and g["lr"] == 1e-2
    assert not {"betas", "eps", "amsgrad"} & set(g)
    # what the user supplied is passed on, so a key the optimizer does not take raises as torch would
    with pytest.raises(TypeError, match="betas"):
        _Pipe(torch.optim.SGD, {"betas": (0.9, 0.99)}).configure()
    with pytest.raises(TypeError):
        _Pipe(torch.optim.AdamW, {"no_such_option": 1}).configure()
    opt = _Pipe(torch.optim.Adam, {"amsgrad": True, "maximize": True}).configure()
    g = opt.param_groups[0]
    assert type(opt) is O.HipAdam and g["amsgrad"] is True and g["maximize"] is True
    assert g["lr"] == 1e-3 and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.999)      # the merged-in AdamW defaults
    # no fused counterpart: the torch class itself, with the same rule (LBFGS takes none of betas / eps / weight_decay / amsgrad)
    assert type(_Pipe(torch.optim.LBFGS, {}).configure()) is torch.optim.LBFGS
    # lr_schedule is the pipeline's own key, not the optimizer's
    assert type(_Pipe(torch.optim.RMSprop, {"lr_schedule": "cosine"}).configure()) is O.HipRMSprop


def test_default_path_builds_the_same_hip_adamw():
    """What tests/test_host_logic.py expects of the default path: HipAdamW, lr * sqrt(world), AdamW's weight_decay and betas, and
    the stored kwargs untouched."""
    pipe = _Pipe(torch.optim.AdamW, {"lr": 1e-4})
    opt = pipe.configure(world=4)
    g = opt.param_groups[0]
    assert type(opt) is O.HipAdamW
    assert g["lr"] == pytest.approx(2e-4) and g["weight_decay"] == 1e-2 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert g["amsgrad"] is False and g["maximize"] is False
    assert pipe.hparams.opt_kwargs == {"lr": 1e-4}
    assert len(g["params"]) == 2


def test_dptrainer_refuses_an_optimizer_without_an_arena():
    from rho_diffusion_amd import trainer

    class _Engine:
        def param_order(self):
            return []

    class _Backbone:
        def engine(self):
            return _Engine()

    pipe = _Pipe(torch.optim.LBFGS, {})
    pipe.backbone = _Backbone()
    with pytest.raises(ValueError, match="no fused counterpart"):
        trainer.DPTrainer(pipe)
