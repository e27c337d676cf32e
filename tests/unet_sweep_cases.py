"""Case table, reference runs and error bars of the whole-UNet sweep (tests/test_unet_sweep_host.py on the CPU,
tests/test_gpu_unet_sweep.py and tests/test_gpu_engine_lifecycle.py on the device).

Cases: value = (UNetv2 constructor kwargs, x shape, y kind) as in golden_cfg.UNET_CASES.  Each reaches a branch of the plan builders
that no recorded golden does (see the comments), at sizes where an engine forward + backward is a few dozen small launches.
Weights: ``det_state_dict`` over a template derived from ``oracle.ref_torch.unet_structure`` (the reference's key names and shapes),
salt = case name; x = det_normal(case + "x"), target = det_normal(case + "tgt"), t = (37 i + 11) % 1000, labels as case_inputs.

Bars (``tensor_errors`` / ``within_bars``): got against the float64 twin g64, the float32 oracle g32 only sizing the bound -
    ||got - g64||_2  <= K ||g32 - g64||_2  + 16 * 2^-24 ||g64||_2      and      max|got - g64| <= K max|g32 - g64| + 16 * 2^-24 max|g64|
with K = 4 and the 16-ulp floor of tests/test_gpu_sinkhorn.py (one tensor class, the head bias, has K = 16: ``K_CLASS``).  A tensor
is LIVE when ||g64|| >= 1e-5 G (G = the global float64 gradient norm; the rule of test_gpu_training.py) and an exact-invariance
ZERO when ||g64|| <= 1e-12 G: a bias in front of a GroupNorm whose groups hold one channel, the embedding projection of an additive
block in front of one.  ``classify`` refuses anything in between."""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np
import torch

import unet_ref64 as R64
from detdata import det_normal, det_state_dict
from golden_cfg import PARAM_SPACE, UNET_CASES, UPDOWN_CASES
from oracle import ref_torch as R

U = 2.0 ** -24
K = 4.0
FLOOR = 16.0 * U
LIVE, ZERO = 1e-5, 1e-12
# The one tensor class with a K of its own (the reason and the measured ratios: docstring of tests/test_gpu_unet_sweep.py)
K_CLASS = {"out.2.bias": 16.0}

SWEEP_CASES = {
    # in != out channels, 3 levels with a non-power-of-two multiplier (96 channels: 3 per GroupNorm group), heads from num_head_channels
    # (1 / 2 / 3 heads of 32), attention at two levels, batch 3, H = 12 -> 6 -> 3
    "odd2d_b3": (dict(in_channels=3, out_channels=6, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 3), attention_resolutions=[2, 4],
                      num_head_channels=32, use_scale_shift_norm=True, dims=2, data_shape=[12, 20]), (3, 3, 12, 20), None),
    # batch 1, odd depth, two channels in and out, attention at full resolution (T = 180), additive embedding, two ResBlocks per level
    "odd3d_b1": (dict(in_channels=2, out_channels=2, model_channels=32, num_res_blocks=2, channel_mult=(1, 2), attention_resolutions=[1],
                      num_heads=1, use_scale_shift_norm=False, dims=3, data_shape=[3, 6, 10]), (1, 2, 3, 6, 10), None),
    # 1-D, batch 5, ResBlock up / down, a level that keeps its width (mult 1, 1), L = 44 -> 22 -> 11 (attention with T = 11)
    "1d_b5_updown": (dict(in_channels=1, out_channels=1, model_channels=64, num_res_blocks=1, channel_mult=(1, 1, 2), attention_resolutions=[4],
                          num_heads=4, use_scale_shift_norm=True, resblock_updown=True, dims=1, data_shape=[44]), (5, 1, 44), None),
    # the constructor's default multipliers: four levels, 256 channels and T = 2 * 3 = 6 at the bottom, one head of 256 channels
    "deep4_2d": (dict(in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, attention_resolutions=[8],
                      use_scale_shift_norm=True, dims=2, data_shape=[16, 24]), (1, 1, 16, 24), None),
    # average pool / nearest without convolutions, additive embedding, attention in the middle block only (T = 15)
    "pool2d_add": (dict(in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 2), attention_resolutions=[],
                        num_heads=2, use_scale_shift_norm=False, conv_resample=False, dims=2, data_shape=[12, 20]), (1, 1, 12, 20), None),
    # another head count on the way up (2 heads of 64 down and in the middle, 4 heads of 32 up), new attention order
    "heads_up_new": (dict(in_channels=1, out_channels=1, model_channels=64, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions=[2],
                          num_heads=2, num_heads_upsample=4, use_scale_shift_norm=True, use_new_attention_order=True, dims=2,
                          data_shape=[8, 8]), (2, 1, 8, 8), None),
    # no resampling at all: one level, attention everywhere (T = 60), batch 4
    "one_level": (dict(in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, channel_mult=(1,), attention_resolutions=[1],
                       num_heads=2, use_scale_shift_norm=True, dims=2, data_shape=[6, 10]), (4, 1, 6, 10), None),
    # label embedding (MultiEmbeddings over PARAM_SPACE) in 3-D, batch 4, depth 2
    "cond3d_b4": (dict(in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions=[2],
                       num_heads=2, use_scale_shift_norm=True, dims=3, data_shape=[2, 4, 12], num_classes=12), (4, 1, 2, 4, 12), "multi"),
    # an activation that runs in the materialising passes, ResBlock up / down, odd depth, 3 x 5 positions per slice at the bottom
    "elu_updown3d_odd": (dict(in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_resolutions=[2],
                              num_heads=2, use_scale_shift_norm=True, resblock_updown=True, activation="ELU", dims=3,
                              data_shape=[3, 6, 10]), (1, 1, 3, 6, 10), None),
}

# the recorded cases on which the float64 twin has to equal the oracle bit for bit at float32
TWIN_CASES = {"tiny2d": UNET_CASES["tiny2d"], "tiny3d": UNET_CASES["tiny3d"], "reftest2d": UNET_CASES["reftest2d"],
              "updown2d_3lvl": UPDOWN_CASES["updown2d_3lvl"]}

ALL_CASES = dict(SWEEP_CASES, **TWIN_CASES)


# --------------------------------------------------------------------------- inputs
def state_template(kw: dict) -> Dict[str, torch.Tensor]:
    """name -> empty tensor of the shape the reference's ``state_dict`` has for these constructor kwargs, in its order: re-derived from
    ``unet_structure`` (the tests hold it against the project's own module and against the recorded key lists)."""
    dims, mc = kw.get("dims", 2), kw["model_channels"]
    e = 4 * mc
    ssn = bool(kw.get("use_scale_shift_norm", False))
    st = R.unet_structure(kw)
    t: Dict[str, Tuple[int, ...]] = {}

    def lin(p, cin, cout):
        t[p + "weight"], t[p + "bias"] = (cout, cin), (cout,)

    def conv(p, cin, cout, k=3):
        t[p + "weight"], t[p + "bias"] = (cout, cin) + (k,) * dims, (cout,)

    def norm(p, c):
        t[p + "weight"], t[p + "bias"] = (c,), (c,)

    def layers(ls):
        for layer in ls:
            kind, p = layer[0], layer[1]
            if kind == "conv":
                conv(p, kw["in_channels"], int(tuple(kw.get("channel_mult", (1, 2, 4, 8)))[0] * mc))
            elif kind in ("res", "res_up", "res_down"):
                cin, cout = layer[2], layer[3]
                norm(p + "in_layers.0.", cin)
                conv(p + "in_layers.2.", cin, cout)
                lin(p + "emb_layers.1.", e, 2 * cout if ssn else cout)
                norm(p + "out_layers.0.", cout)
                conv(p + "out_layers.3.", cout, cout)
                if cin != cout:
                    conv(p + "skip_connection.", cin, cout, 1)
            elif kind == "attn":
                c = layer[2]
                norm(p + "norm.", c)
                t[p + "qkv.weight"], t[p + "qkv.bias"] = (3 * c, c, 1), (3 * c,)
                t[p + "proj_out.weight"], t[p + "proj_out.bias"] = (c, c, 1), (c,)
            elif kind in ("down", "up"):
                conv(p, layer[2], layer[2])

    lin("time_embed.0.", mc, e)
    lin("time_embed.2.", e, e)
    if kw.get("num_classes") is not None:
        for key, vals in PARAM_SPACE.items():
            t[f"cond_fn.embedding_layers.{key}.weight"] = (len(vals), e)
    for ls in st["input"]:
        layers(ls)
    layers(st["middle"])
    for ls in st["output"]:
        layers(ls)
    norm("out.0.", st["final_ch"])
    conv("out.2.", int(tuple(kw.get("channel_mult", (1, 2, 4, 8)))[0] * mc), kw["out_channels"])
    return {k: torch.empty(s) for k, s in t.items()}


def sweep_inputs(case: str):
    """(cfg, x, t, y, parameter space or None, state dict) of a case, all float32 on the CPU."""
    kw, xshape, ykind = ALL_CASES[case]
    x = det_normal(xshape, case + "x")
    B = xshape[0]
    t = torch.tensor([(37 * i + 11) % 1000 for i in range(B)])
    y = None
    if ykind == "multi":
        keys = list(PARAM_SPACE.keys())
        y = torch.tensor([[PARAM_SPACE[k][(i + j) % len(PARAM_SPACE[k])] for j, k in enumerate(keys)] for i in range(B)], dtype=torch.float32)
    sd = det_state_dict(state_template(kw), case)
    return dict(kw), x, t, y, (PARAM_SPACE if ykind == "multi" else None), sd


def target_of(case: str, pred_shape) -> torch.Tensor:
    return det_normal(tuple(pred_shape), case + "tgt")


def reference_runs(cfg, x, t, y, ps, sd, target):
    """{"f64": (pred, loss, grads) of the float64 twin, "f32": the same of the float32 oracle} for any weights (the lifecycle tests)."""
    return {"f64": R64.loss_and_grads(R64.unet_forward, sd, cfg, x, t, y, ps, target, torch.float64),
            "f32": R64.loss_and_grads(R.unet_forward, sd, cfg, x, t, y, ps, target, torch.float32)}


def reference_preds(cfg, x, t, y, ps, sd):
    """The predictions alone, in the layout of ``reference_runs`` (loss and gradients None)."""
    with torch.no_grad():
        p64 = R64.unet_forward(sd, cfg, x, t, y, ps, dtype=torch.float64)
        p32 = R.unet_forward({k: v.float() for k, v in sd.items()}, cfg, x, t, y, ps)
    return {"f64": (p64, None, None), "f32": (p32, None, None)}


@functools.lru_cache(maxsize=None)
def case_refs(case: str):
    """The two reference runs of a case, computed once per process and shared (read-only) by every test that needs them."""
    cfg, x, t, y, ps, sd = sweep_inputs(case)
    kw = ALL_CASES[case][0]
    out_shape = (x.shape[0], kw["out_channels"]) + tuple(x.shape[2:])
    return reference_runs(cfg, x, t, y, ps, sd, target_of(case, out_shape))


# --------------------------------------------------------------------------- bars
def global_norm(grads: Dict[str, torch.Tensor]) -> float:
    return float(np.sqrt(sum(float(g.double().norm()) ** 2 for g in grads.values())))


def classify(g64: Dict[str, torch.Tensor]):
    """(G, {name: "live" | "zero"}); a tensor between the two rules is an error of the CASE (change its inputs, not the rule)."""
    G = global_norm(g64)
    kinds, gap = {}, []
    for name, g in g64.items():
        n = float(g.double().norm())
        if n >= LIVE * G:
            kinds[name] = "live"
        elif n <= ZERO * G:
            kinds[name] = "zero"
        else:
            gap.append((name, n / G))
    assert not gap, f"neither live nor an exact zero (||g64|| / G): {gap}"
    return G, kinds


def tensor_errors(got: torch.Tensor, g64: torch.Tensor, g32: torch.Tensor) -> dict:
    """Both norms of got - g64 and of g32 - g64, the bounds they give, and the index of the worst element."""
    g64 = g64.double().cpu()
    d = got.detach().double().cpu().reshape(g64.shape) - g64
    o = g32.double().cpu() - g64
    flat = int(d.abs().argmax())
    return dict(l2=float(d.norm()), max=float(d.abs().max()), o_l2=float(o.norm()), o_max=float(o.abs().max()),
                n_l2=float(g64.norm()), n_max=float(g64.abs().max()), argmax=tuple(int(i) for i in np.unravel_index(flat, tuple(g64.shape) or (1,))))


def bounds(e: dict, k: float = K) -> Tuple[float, float]:
    return k * e["o_l2"] + FLOOR * e["n_l2"], k * e["o_max"] + FLOOR * e["n_max"]


def within_bars(e: dict, k: float = K) -> bool:
    b2, bm = bounds(e, k)
    return e["l2"] <= b2 and e["max"] <= bm


def ratios(e: dict) -> Tuple[float, float]:
    """err / (the float32 oracle's own error), per norm; the oracle's error is floored at one ulp of the tensor's size so that a tensor
    the oracle gets exactly right prints a finite figure."""
    return e["l2"] / max(e["o_l2"], U * e["n_l2"], 1e-300), e["max"] / max(e["o_max"], U * e["n_max"], 1e-300)


def describe(case: str, path: str, name: str, e: dict, k: float = K) -> str:
    b2, bm = bounds(e, k)
    return (f"{case}[{path}] {name}: l2 err {e['l2']:.3e} (bound {b2:.3e}, oracle {e['o_l2']:.3e}, |g64| {e['n_l2']:.3e}); "
            f"max err {e['max']:.3e} at {e['argmax']} (bound {bm:.3e}, oracle {e['o_max']:.3e}, max|g64| {e['n_max']:.3e})")


def check_against_refs(case: str, path: str, refs: dict, pred, loss, grads: Dict[str, torch.Tensor], what: str = "") -> dict:
    """Hold an engine result (prediction, loss, {name: gradient}) against reference runs at the bars above.  Returns the worst ratios
    {"l2": (ratio, tensor), "max": (ratio, tensor, index)} over the tensors held to K (those of ``K_CLASS`` are printed apart); raises AssertionError listing every tensor over its bar."""
    p64, l64, g64 = refs["f64"]
    p32, l32, g32 = refs["f32"]
    G, kinds = classify(g64) if grads is not None else (None, None)
    bad = []
    worst = {"l2": (0.0, None), "max": (0.0, None, None)}

    def one(name, got, r64, r32):
        e = tensor_errors(got, r64, r32)
        r2, rm = ratios(e)
        k = K_CLASS.get(name, K)
        if k != K:
            print(f"    {case}[{path}] {name} (K = {k:g}): l2 ratio {r2:.3f}, max ratio {rm:.3f}")
        elif r2 > worst["l2"][0]:
            worst["l2"] = (r2, name)
        if k == K and rm > worst["max"][0]:
            worst["max"] = (rm, name, e["argmax"])
        if not within_bars(e, k):
            bad.append(describe(case, path, name, e, k) + (f" [K = {k:g} for this tensor class]" if k != K else ""))
        elif max(r2, rm) > K:
            print(f"    over {K:g} times the oracle's error, inside its bar: " + describe(case, path, name, e, k))

    if pred is not None:
        one("<prediction>", pred, p64, p32)
    if loss is not None:
        one("<loss>", torch.as_tensor(loss).reshape(()), l64.reshape(()), l32.reshape(()))
    if grads is not None:
        missing = sorted(set(g64) - set(grads))
        assert not missing, f"{case}[{path}] {what}: no gradient for {missing[:4]}"
        for name, r64 in g64.items():
            if kinds[name] == "zero":
                n = float(grads[name].double().norm())
                if not n <= 1e-5 * G:
                    bad.append(f"{case}[{path}] {name}: an exact-invariance zero has norm {n:.3e} > 1e-5 G = {1e-5 * G:.3e}")
            else:
                one(name, grads[name], r64, g32[name])
    print(f"{case}[{path}] {what}: worst l2 ratio {worst['l2'][0]:.3f} ({worst['l2'][1]}), worst max ratio {worst['max'][0]:.3f} "
          f"({worst['max'][1]} at {worst['max'][2]})")
    assert not bad, "\n".join([f"{len(bad)} over the bar (K = {K:g}):"] + bad[:8])
    return worst
