"""The registry's optimizers (reference: registry.py:177-193) whose update runs in fused HIP kernels over flat parameter /
gradient / state arenas: one launch per step instead of ~300 small ones.

``HipAdamW`` is the default (torch.optim.AdamW built at abstract_diffusion.py:103-119; defaults lr 1e-3, betas (0.9, 0.999),
eps 1e-8, weight_decay 1e-2; rho_adamw, 7 x 4 B per parameter of HBM traffic).  ``HipAdam``, ``HipSGD``, ``HipRMSprop``,
``HipAdagrad``, ``HipAdamax``, ``HipNAdam``, ``HipRAdam`` and ``HipAdadelta`` share its arena and take rho_optim_step, which follows
the single-tensor paths of torch 2.10's ``torch.optim``.  Every class has its namesake's constructor plus ``arena_order`` and
``max_grad_norm``; with the latter set, ``step()`` clips by the global L2 norm of all groups' gradients (the formula of
``torch.nn.utils.clip_grad_norm_``, diffusers.py:134 of the reference) without rewriting them or reading anything back.
``state_dict()`` / ``load_state_dict()`` speak torch's format: the dict of ``HipX`` loads into ``torch.optim.X`` and back."""
from __future__ import annotations

import ctypes

import torch

from .engine import ops


def _f32(x) -> float:
    """The float32 value the C ABI receives for a hyperparameter."""
    return ctypes.c_float(float(x)).value


class ArenaOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: parameters and gradients re-homed into one contiguous fp32 arena per param group, the
    gather of gradients produced outside it, clipping, the version bump and the state_dict in torch's format."""

    TORCH = None          # the torch.optim namesake: its defaults, its argument checks, its state_dict format
    KIND = None           # kind name of ops.optim_step

    def __init__(self, params, hyper: dict, arena_order=None, max_grad_norm=None):
        if hyper.get("differentiable"):
            raise RuntimeError(f"{type(self).__name__}: differentiable=True is not supported, the update runs in a HIP kernel outside autograd")
        if isinstance(hyper.get("lr"), torch.Tensor):
            raise ValueError(f"{type(self).__name__}: a tensor lr is not supported, the kernel takes lr by value; pass a float "
                             "(an lr_scheduler may still change param_groups[...]['lr'])")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0, got {max_grad_norm}")
        # foreach / fused / capturable choose between torch's implementations: accepted, and without meaning here
        hyper = {k: v for k, v in hyper.items() if k not in ("foreach", "fused", "capturable")}
        # the namesake checks the arguments (raising what torch would raise) and supplies the full set of group keys
        defaults = dict(self.TORCH([torch.zeros(1)], **hyper).defaults)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None        # 1-element device tensor: the norm before clipping, written by the last step()
        self._clip_ws = None
        self._arena = None
        self._arena_order = {id(p): i for i, p in enumerate(arena_order)} if arena_order is not None else None

    # ------------------------------------------------------------------ per kind
    def _slots(self, group):
        """[(torch state key, arena key) or None] x 3: the state arenas in rho_optim_step's slot order for this group's options."""
        raise NotImplementedError

    def _hp(self, group, a):
        """(flags, hyperparameters after lr / weight_decay / eps) for this step."""
        raise NotImplementedError

    def _init_value(self, group, key) -> float:
        return 0.0

    HAS_STEP = True       # the state carries torch's `step` entry
    EPS_KEY = "eps"

    # ------------------------------------------------------------------ arena
    def _build_arena(self):
        """Re-home every parameter into one contiguous fp32 arena (views keep the module API intact)."""
        self._arena = []
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.requires_grad]
            if self._arena_order is not None:
                ps.sort(key=lambda p: self._arena_order.get(id(p), 1 << 30))
            n = sum(p.numel() for p in ps)
            dev = ps[0].device
            flat = torch.empty(n, dtype=torch.float32, device=dev)
            grad = torch.zeros(n, dtype=torch.float32, device=dev)
            off = 0
            for p in ps:
                k = p.numel()
                flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + k].view_as(p)
                if p.grad is not None:                   # a backward ran before the arena existed: keep what it produced
                    self._refuse_sparse(p.grad)
                    grad[off:off + k].copy_(p.grad.reshape(-1))
                p.grad = grad[off:off + k].view_as(p)
                off += k
            a = dict(flat=flat, grad=grad, step=0, params=ps)
            for slot in self._slots(group):
                if slot is not None:
                    a[slot[1]] = torch.full_like(flat, self._init_value(group, slot[0]))
            self._arena.append(a)

    def build_arena(self):
        if self._arena is None:
            self._build_arena()
        return self._arena

    @property
    def flat_grads(self):
        return [a["grad"] for a in self.build_arena()]

    def zero_grad(self, set_to_none: bool = False):
        for a in self.build_arena():
            a["grad"].zero_()

    @staticmethod
    def _spans(a):
        off = 0
        for p in a["params"]:
            k = p.numel()
            yield p, off, k
            off += k

    def _refuse_sparse(self, g):
        if g.is_sparse:
            raise RuntimeError(f"{type(self).__name__} does not support sparse gradients: the update streams one dense arena")

    def _gather(self, a):
        # gradients produced outside the arena (first step / foreign autograd) are gathered once
        for p, off, k in self._spans(a):
            if p.grad is None:
                continue
            self._refuse_sparse(p.grad)
            if p.grad.data_ptr() != a["grad"][off:off + k].data_ptr():
                a["grad"][off:off + k].copy_(p.grad.reshape(-1))
                p.grad = a["grad"][off:off + k].view_as(p)

    def _clip_scale(self, arena):
        """Two launches per arena-set: per-workgroup sums of squares of every gradient arena side by side, then one workgroup that
        adds them in index order and writes {norm, coef}.  Returns the 1-element view of coef."""
        if self._clip_ws is None:
            blocks = [ops.sumsq_blocks(a["grad"].numel()) for a in arena]
            dev = arena[0]["grad"].device
            self._clip_ws = (blocks, torch.empty(sum(blocks), dtype=torch.float32, device=dev),
                             torch.zeros(2, dtype=torch.float32, device=dev))
        blocks, partials, out = self._clip_ws
        off = 0
        for a, k in zip(arena, blocks):
            ops.sumsq_partial(a["grad"], partials[off:off + k])
            off += k
        ops.clip_coef(partials, self.max_grad_norm, out)
        self.last_grad_norm = out[0:1]
        return out[1:2]

    def _update(self, group, a, gscale):
        states = []
        for slot in self._slots(group):
            if slot is None:
                states.append(None)
                continue
            if slot[1] not in a:                         # an option switched on after the arena was built
                a[slot[1]] = torch.full_like(a["flat"], self._init_value(group, slot[0]))
            states.append(a[slot[1]])
        flags, extra = self._hp(group, a)
        if group.get("maximize"):
            flags |= ops.OPT_MAXIMIZE
        hp = [group["lr"], group["weight_decay"], group.get(self.EPS_KEY, 0.0), *extra]
        ops.optim_step(self.KIND, a["flat"], a["grad"], states, hp, a["step"], flags, gscale)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        arena = self.build_arena()
        for a in arena:
            self._gather(a)
        gscale = self._clip_scale(arena) if self.max_grad_norm is not None else None
        for group, a in zip(self.param_groups, arena):
            if isinstance(group["lr"], torch.Tensor):
                raise ValueError(f"{type(self).__name__}: a tensor lr is not supported, the kernel takes lr by value")
            a["step"] += 1
            self._update(group, a, gscale)
        # parameters changed in place through the arena: bump their version counters (no kernel) so
        # dependants (the engine's prepared conv weights) refresh
        for a in arena:
            for p in a["params"]:
                torch.autograd.graph.increment_version(p)
        return loss

    # ------------------------------------------------------------------ state_dict in torch's format
    def _param_state(self, group, a, view):
        """torch's per-parameter state entry; ``view(arena key)`` is this parameter's window of a state arena.  None: no entry yet."""
        if a["step"] == 0:
            return None
        st = {"step": torch.tensor(float(a["step"]), dtype=torch.float32)} if self.HAS_STEP else {}
        for slot in self._slots(group):
            if slot is not None:
                st[slot[0]] = view(slot[1])
        return st

    def _fresh_state(self, group, p):
        """State of a parameter before the arena exists: what a new torch.optim namesake holds (nothing, for most)."""
        return None

    def _export_state(self):
        self.state.clear()
        if self._arena is None:
            for group in self.param_groups:
                for p in group["params"]:
                    st = self._fresh_state(group, p)
                    if st is not None:
                        self.state[p] = st
            return
        for group, a in zip(self.param_groups, self._arena):
            for p, off, k in self._spans(a):
                st = self._param_state(group, a, lambda key: a[key][off:off + k].view_as(p))
                if st is not None:
                    self.state[p] = st

    def state_dict(self):
        """torch's format, entries indexed in param_groups order; the tensors are windows of the state arenas."""
        self._export_state()
        return super().state_dict()

    def _load_step(self, group, a, states):
        steps = {int(st["step"]) for st in states if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"{type(self).__name__}: the parameters of one group carry different step counts {sorted(steps)}; "
                             "the arena keeps one per group")
        a["step"] = steps.pop() if steps else 0

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies a torch.optim (or Hip*) state_dict into the arenas; param_groups options are taken over as torch does."""
        super().load_state_dict(state_dict)               # casts to each parameter's device, fills self.state and param_groups
        arena = self.build_arena()
        for group, a in zip(self.param_groups, arena):
            loaded = [self.state[p] for p in a["params"] if p in self.state and self.state[p]]
            if loaded and len(loaded) != len(a["params"]):
                raise ValueError(f"{type(self).__name__}: state for {len(loaded)} of {len(a['params'])} parameters of a group; "
                                 "the arena needs all or none")
            self._load_step(group, a, loaded)
            self._load_extra(group, a, loaded)
            for slot in self._slots(group):
                if slot is None:
                    continue
                if slot[1] not in a:
                    a[slot[1]] = torch.empty_like(a["flat"])
                if not loaded:
                    a[slot[1]].fill_(self._init_value(group, slot[0]))
                    continue
                for p, off, k in self._spans(a):
                    src = self.state[p].get(slot[0])
                    if src is None:
                        a[slot[1]][off:off + k].fill_(self._init_value(group, slot[0]))
                    else:
                        a[slot[1]][off:off + k].copy_(src.reshape(-1))
        self._export_state()                              # self.state: windows of the arenas again, not the loaded copies

    def _load_extra(self, group, a, states):
        pass


class _AdamFamily(ArenaOptimizer):
    def _slots(self, group):
        return [("exp_avg", "m"), ("exp_avg_sq", "v"), ("max_exp_avg_sq", "max") if group.get("amsgrad") else None]

    def _hp(self, group, a):
        flags = ops.OPT_AMSGRAD if group.get("amsgrad") else 0
        if group.get("decoupled_weight_decay"):
            flags |= ops.OPT_DECOUPLED_WD
        return flags, group["betas"]


class HipAdamW(_AdamFamily):
    TORCH, KIND = torch.optim.AdamW, "AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, arena_order=None, max_grad_norm=None):
        """``arena_order``: optional parameter order for the flat arena (``UNetEngine.param_order()``), so
        that the gradients that become final together during backward are adjacent in memory."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _hp(self, group, a):
        flags, extra = super()._hp(group, a)
        return flags & ~ops.OPT_DECOUPLED_WD, extra        # the kind itself is decoupled

    def _update(self, group, a, gscale):
        if group["amsgrad"] or group["maximize"] or gscale is not None:
            return super()._update(group, a, gscale)
        b1, b2 = group["betas"]
        ops.adamw(a["flat"], a["grad"], a["m"], a["v"], group["lr"], b1, b2, group["eps"], group["weight_decay"], a["step"])


class HipAdam(_AdamFamily):
    TORCH, KIND = torch.optim.Adam, "Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                 arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      differentiable=differentiable, decoupled_weight_decay=decoupled_weight_decay),
                         arena_order, max_grad_norm)


class HipSGD(ArenaOptimizer):
    """The first step seeds the momentum buffer with the gradient (torch/optim/sgd.py: ``buf = clone(grad)``); torch's state has no
    step count, so a loaded momentum_buffer means "past the first step"."""
    TORCH, KIND, HAS_STEP, EPS_KEY = torch.optim.SGD, "SGD", False, None

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("momentum_buffer", "momentum_buffer") if group["momentum"] != 0 else None, None, None]

    def _hp(self, group, a):
        return (ops.OPT_NESTEROV if group["nesterov"] else 0), (group["momentum"], group["dampening"])

    def _param_state(self, group, a, view):
        if a["step"] == 0:
            return None
        return {"momentum_buffer": view("momentum_buffer") if group["momentum"] != 0 else None}

    def _load_step(self, group, a, states):
        a["step"] = 1 if any(st.get("momentum_buffer") is not None for st in states) else 0


class HipRMSprop(ArenaOptimizer):
    TORCH, KIND = torch.optim.RMSprop, "RMSprop"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False,
                 foreach=None, maximize=False, differentiable=False, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered,
                                      maximize=maximize, differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("square_avg", "square_avg"), ("grad_avg", "grad_avg") if group["centered"] else None,
                ("momentum_buffer", "momentum_buffer") if group["momentum"] > 0 else None]

    def _hp(self, group, a):
        return (ops.OPT_CENTERED if group["centered"] else 0), (group["alpha"], group["momentum"])


class HipAdagrad(ArenaOptimizer):
    """torch's Adagrad creates its state in the constructor (step 0, sum = initial_accumulator_value): so does the state_dict here."""
    TORCH, KIND = torch.optim.Adagrad, "Adagrad"

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10, foreach=None, *,
                 maximize=False, differentiable=False, fused=None, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                                      initial_accumulator_value=initial_accumulator_value, eps=eps, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("sum", "sum"), None, None]

    def _init_value(self, group, key):
        return float(group["initial_accumulator_value"])

    def _hp(self, group, a):
        return 0, (group["lr_decay"],)

    def _param_state(self, group, a, view):
        return {"step": torch.tensor(float(a["step"]), dtype=torch.float32), "sum": view("sum")}

    def _fresh_state(self, group, p):
        return {"step": torch.tensor(0.0, dtype=torch.float32),
                "sum": torch.full_like(p, float(group["initial_accumulator_value"]), memory_format=torch.preserve_format)}


class HipAdamax(ArenaOptimizer):
    TORCH, KIND = torch.optim.Adamax, "Adamax"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, foreach=None, *, maximize=False,
                 differentiable=False, capturable=False, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("exp_avg", "m"), ("exp_inf", "exp_inf"), None]

    def _hp(self, group, a):
        return 0, group["betas"]


class HipNAdam(ArenaOptimizer):
    """``mu_product`` is a float32 scalar in torch's state (one per parameter, all equal): kept per group on the host, advanced with
    torch's own float32 arithmetic, and handed to the kernel's launcher by value."""
    TORCH, KIND = torch.optim.NAdam, "NAdam"

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, momentum_decay=4e-3,
                 decoupled_weight_decay=False, *, foreach=None, maximize=False, capturable=False, differentiable=False,
                 arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum_decay=momentum_decay,
                                      decoupled_weight_decay=decoupled_weight_decay, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("exp_avg", "m"), ("exp_avg_sq", "v"), None]

    def _hp(self, group, a):
        b1, b2 = group["betas"]
        md = _f32(group["momentum_decay"])
        mu = _f32(b1) * (1.0 - 0.5 * (0.96 ** (a["step"] * md)))          # nadam.py: the kernel's launcher evaluates the same
        a.setdefault("mu_product", torch.ones((), dtype=torch.float32))
        a["mu_product"] *= mu
        return (ops.OPT_DECOUPLED_WD if group["decoupled_weight_decay"] else 0), (b1, b2, md, float(a["mu_product"]))

    def _param_state(self, group, a, view):
        st = super()._param_state(group, a, view)
        if st is not None:
            st["mu_product"] = a["mu_product"].clone()
        return st

    def _load_extra(self, group, a, states):
        mus = {float(st["mu_product"]) for st in states if "mu_product" in st}
        if len(mus) > 1:
            raise ValueError("HipNAdam: the parameters of one group carry different mu_product values; the arena keeps one per group")
        a["mu_product"] = torch.tensor(mus.pop() if mus else 1.0, dtype=torch.float32)


class HipRAdam(ArenaOptimizer):
    TORCH, KIND = torch.optim.RAdam, "RAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, decoupled_weight_decay=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=decoupled_weight_decay, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("exp_avg", "m"), ("exp_avg_sq", "v"), None]

    def _hp(self, group, a):
        return (ops.OPT_DECOUPLED_WD if group["decoupled_weight_decay"] else 0), group["betas"]


class HipAdadelta(ArenaOptimizer):
    TORCH, KIND = torch.optim.Adadelta, "Adadelta"

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, foreach=None, *, capturable=False, maximize=False,
                 differentiable=False, arena_order=None, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay, maximize=maximize,
                                      differentiable=differentiable), arena_order, max_grad_norm)

    def _slots(self, group):
        return [("square_avg", "square_avg"), ("acc_delta", "acc_delta"), None]

    def _hp(self, group, a):
        return 0, (group["rho"],)


_FUSED = {c.TORCH: c for c in (HipAdamW, HipAdam, HipSGD, HipRMSprop, HipAdagrad, HipAdamax, HipNAdam, HipRAdam, HipAdadelta)}


def fused_optimizer_class(torch_cls):
    """The fused class of a ``torch.optim`` class, or None (ASGD, Rprop, LBFGS and SparseAdam stay on torch.optim)."""
    return _FUSED.get(torch_cls)


def optimizer_kwargs(cls, user_kwargs: dict) -> dict:
    """The keyword arguments ``configure_optimizers`` / ``DPTrainer`` build ``cls`` with.  The reference merges the defaults of
    AdamW into whatever optimizer is named (abstract_diffusion.py:103-116); here a merged-in default that the user did not supply
    and that ``cls`` does not take is dropped, so that optimizer="SGD" can be built at all.  Everything the user supplied is passed
    on: an unknown key raises TypeError in the constructor, as torch would."""
    import inspect
    spec = inspect.getfullargspec(torch.optim.AdamW)
    names = [n for n in spec.args if n not in ("self", "params")]
    takes = set(inspect.signature(cls.__init__).parameters)
    kw = {k: v for k, v in zip(names, spec.defaults or ()) if k in takes and k not in user_kwargs}
    kw.update(user_kwargs)
    kw.pop("lr_schedule", None)
    return kw
