"""-m gpu: StructuralSimilarityIndexMeasure (metrics/ssim.py, csrc/ssim.hip) against the float64 restatement of tests/ssim_ref.py.

The per-voxel bound is computed in float64 from the kernel's written arithmetic (the header of csrc/ssim.hip), not from its output:

  roundings of one window sum.  A pass over k taps is one product and k - 1 fmaf: k roundings; the passes along W, H and D give
  k_w + k_h + k_d (a dimension the field does not have is the one-tap window {1.0}: exact).  Each factor of x = a a, b b, a b carries
  the rounding of its shift a = p - s (2 in all), and the product rounds once.  K = k_w + k_h + k_d + 3 bounds all five moments:
      |err W[x y]| <= K u W[|x y|] on the shifted data, u = 2^-24   (every partial sum of a pass is at most the pass of |.|).
  window sum.  The float32 taps sum to 1 + delta, not 1 (test_ssim_host.py: the shifted variance differs from the definition's by
  delta s (2 W[p] - s), the covariance by delta s (W[p] + W[t] - s), the mean by delta s): these gaps are part of the bound.
  index.  First-order partials through s_pp, s_tt, s_pt, mu = s + W[.], the two factors of numerator and denominator, their
  products and the quotient, plus the rounding of every operation written in ssim_index(); c1 = (k1 R)^2 and c2 in float32 from a
  float32 k and a float32 R (7 u each: conversions, two products, and the subtraction behind a measured R).

Reductions: |got - ref| <= mean(bound) + 2 u |ref| (the sums of S run in float64; one rounding to float32 at the end)."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import ssim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
TD, TH, TW = 16, 16, 32          # output planes / rows / columns per workgroup (SSIM_TD, SSIM_TH, SSIM_TW of csrc/ssim.hip)
VEC = 4                          # floats per 16-byte load: taken when W % 4 == 0 and both bases are 16-byte aligned
CAP = 15                         # rho_ssim_max_window()

G = dict(gaussian_kernel=True, sigma=1.5)                  # the default window: the compiled 11-tap forms
ANISO = dict(gaussian_kernel=True, sigma=(0.8, 1.5, 2.0))  # 7, 11, 15 taps: the runtime form


def uni(*k):
    return dict(gaussian_kernel=False, kernel_size=k if len(k) > 1 else k[0])


# name -> (shape, window keywords, data kind, data_range).  Output extents one below / at / one above the tile: size = tile + 10 - 1,
# + 10, + 11 for 11 taps (25, 26, 27 along D and H; 41, 42, 43 along W); W = 40 and 44 take the 16-byte loads, the others the scalar.
CASES = {
    # ---- 3-D, default window (form 11 x 11 x 11)
    "3d-one-window": ((1, 1, 11, 11, 11), G, "rand", 1.0),
    "3d-window+1": ((1, 1, 12, 12, 12), G, "rand", 1.0),
    "3d-below-tile": ((1, 1, TD + 9, TH + 9, TW + 9), G, "rand", 1.0),
    "3d-at-tile": ((1, 1, TD + 10, TH + 10, TW + 10), G, "rand", 1.0),
    "3d-above-tile": ((1, 1, TD + 11, TH + 11, TW + 11), G, "rand", 1.0),
    "3d-vec-two-tiles": ((3, 3, 12, 13, 11 * VEC), G, "rand", 1.0),
    "3d-vec-one-tile": ((1, 1, 12, 12, 10 * VEC), G, "rand", 1.0),
    "3d-aniso-field": ((1, 3, 11, 40, 13), G, "rand", 1.0),
    "3d-ring-wraps": ((3, 1, 35, 12, 12), G, "rand", 1.0),
    "3d-workload-plane": ((2, 1, 12, 64, 64), G, "rand", 1.0),
    "3d-offset": ((1, 1, 16, 16, 16), G, "offset", 1.0),
    # ---- 2-D (form 1 x 11 x 11)
    "2d-one-window": ((1, 1, 11, 11), G, "rand", 1.0),
    "2d-window+1": ((1, 1, 12, 12), G, "rand", 1.0),
    "2d-below-tile": ((3, 3, TH + 9, TW + 9), G, "rand", 1.0),
    "2d-at-tile": ((1, 1, TH + 10, TW + 10), G, "rand", 1.0),
    "2d-above-tile": ((1, 1, TH + 11, TW + 11), G, "rand", 1.0),
    "2d-vec": ((2, 1, 64, 64), G, "rand", 1.0),
    "2d-vec-odd-h": ((1, 3, 17, 11 * VEC), G, "rand", 1.0),
    "2d-offset": ((1, 1, 32, 32), G, "offset", 1.0),
    # ---- 1-D (form 1 x 1 x 11)
    "1d-one-window": ((1, 1, 11), G, "rand", 1.0),
    "1d-window+1": ((1, 1, 12), G, "rand", 1.0),
    "1d-below-tile": ((3, 3, TW + 9), G, "rand", 1.0),
    "1d-at-tile": ((1, 1, TW + 10), G, "rand", 1.0),
    "1d-above-tile": ((1, 1, TW + 11), G, "rand", 1.0),
    "1d-vec": ((2, 3, 100), G, "rand", 1.0),
    # ---- other windows (the runtime form)
    "3d-7x11x15": ((1, 2, 20, 20, 40), ANISO, "rand", 1.0),
    "3d-7x11x15-one-window": ((1, 1, 7, 11, 15), ANISO, "rand", 1.0),
    "3d-7x11x15-tiles": ((1, 1, TD + 6, TH + 11, TW + 15), ANISO, "rand", 1.0),
    "2d-uniform-3x7": ((2, 1, 20, 45), uni(3, 7), "rand", 1.0),
    "3d-uniform-3x7x3": ((1, 1, 20, 20, 35), uni(3, 7, 3), "rand", 1.0),
    "3d-window-1-in-d": ((1, 2, 5, 20, 36), uni(1, 7, 3), "rand", 1.0),
    "2d-window-1-in-w": ((1, 1, 20, 33), uni(7, 1), "rand", 1.0),
    "1d-uniform-3": ((2, 2, 37), uni(3), "rand", 1.0),
    "3d-cap-one-window": ((1, 1, CAP, CAP, CAP), uni(CAP), "rand", 1.0),
    "3d-cap-tiles": ((1, 1, CAP + 2, TH + CAP + 1, TW + CAP), uni(CAP), "rand", 1.0),       # 30 x 46 staged: the LDS tile's limits
    "2d-cap-vec": ((1, 1, 40, 64), uni(CAP), "offset", 1.0),
    # ---- data_range
    "2d-range-none": ((2, 2, 20, 24), G, "wide", None),
    "3d-range-pair": ((1, 2, 12, 14, 16), G, "wide", (0.0, 1.0)),
    "2d-range-float": ((1, 1, 20, 20), G, "wide", 2.5),
}
IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def data(name):
    shape, _, kind, _ = CASES[name]
    g = torch.Generator().manual_seed(IDS.index(name))
    if kind == "offset":                                  # small contrast on a large offset: what an unshifted float32 form loses
        return 0.9 + 0.1 * torch.rand(shape, generator=g), 0.9 + 0.1 * torch.rand(shape, generator=g)
    t = torch.rand(shape, generator=g)
    p = t + 0.1 * torch.randn(shape, generator=g)
    if kind == "wide":
        p, t = 2.0 * p - 0.5, 1.5 * t - 0.25
    return p, t


def wins_of(name):
    shape, kw, _, _ = CASES[name]
    return R.windows(len(shape) - 2, kw["gaussian_kernel"], kw.get("sigma", 1.5), kw.get("kernel_size", 11))


@functools.lru_cache(maxsize=None)
def ref(name):
    p, t = data(name)
    r = R.ssim(p.numpy(), t.numpy(), wins_of(name), CASES[name][3])
    r["bound"] = bound_of(r, wins_of(name))
    return r


def bound_of(r, wins):
    """The per-voxel bound of the module docstring, float64."""
    K = sum(len(w) for w in wins) + 3
    delta = abs(float(np.prod([w.astype(np.float64).sum() for w in wins])) - 1.0)
    s = np.abs(r["shift"])
    wa, wb, mu_p, mu_t = np.abs(r["w_a"]), np.abs(r["w_b"]), np.abs(r["mu_p"]), np.abs(r["mu_t"])
    e_a, e_b = K * U * r["w_abs_a"], K * U * r["w_abs_b"]
    e_aa, e_bb, e_ab = K * U * r["w_aa"], K * U * r["w_bb"], K * U * r["w_abs_ab"]
    e_mup, e_mut = e_a + U * mu_p + delta * s, e_b + U * mu_t + delta * s
    e_spp = e_aa + 2 * wa * e_a + U * wa ** 2 + U * np.abs(r["w_aa"] - wa ** 2) + delta * s * (2 * mu_p + s)
    e_stt = e_bb + 2 * wb * e_b + U * wb ** 2 + U * np.abs(r["w_bb"] - wb ** 2) + delta * s * (2 * mu_t + s)
    e_spt = e_ab + wa * e_b + wb * e_a + U * wa * wb + U * np.abs(r["w_ab"] - r["w_a"] * r["w_b"]) + delta * s * (mu_p + mu_t + s)
    c1, c2, e_c = r["c1"], r["c2"], 7 * U
    a1, a2 = 2 * r["mu_p"] * r["mu_t"] + c1, 2 * r["s_pt"] + c2
    b1, b2 = r["mu_p"] ** 2 + r["mu_t"] ** 2 + c1, r["s_pp"] + r["s_tt"] + c2
    e_a1 = 2 * (mu_t * e_mup + mu_p * e_mut) + U * 2 * mu_p * mu_t + U * np.abs(a1) + e_c * c1
    e_a2 = 2 * e_spt + U * np.abs(a2) + e_c * c2
    e_b1 = 2 * mu_p * e_mup + 2 * mu_t * e_mut + 2 * U * (mu_p ** 2 + mu_t ** 2) + U * b1 + e_c * c1
    e_b2 = e_spp + e_stt + U * (r["s_pp"] + r["s_tt"]) + U * b2 + e_c * c2
    num, den = a1 * a2, b1 * b2
    e_num = np.abs(a2) * e_a1 + np.abs(a1) * e_a2 + U * np.abs(num)
    e_den = b2 * e_b1 + b1 * e_b2 + U * den
    return e_num / den + np.abs(num) * e_den / den ** 2 + U * np.abs(num / den)


def metric(name, **kw):
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    return StructuralSimilarityIndexMeasure(data_range=CASES[name][3], **CASES[name][1], **kw)


def run(name, return_map=True, p=None, t=None):
    """(per_sample, out = {mean, sum}, map) from one call of ops.ssim with the metric's windows."""
    from rho_diffusion_amd.engine import ops
    m = metric(name)
    if p is None:
        p, t = (x.to(DEV) for x in data(name))
    return ops.ssim(p, t, m._device_windows(p.device, p.dim() - 2), m.range, m.clamp, m.k1, m.k2, return_map)


def check_against_ref(name, per_sample, out, smap):
    r = ref(name)
    got = smap.double().cpu().numpy()
    assert got.shape == r["map"].shape
    err = np.abs(got - r["map"])
    fp32 = np.abs(R.ssim(*(x.numpy() for x in data(name)), wins_of(name), CASES[name][3], fp32=True)["map"].astype(np.float64) - r["map"])
    print(f"{name}: map max err {err.max():.3e}, max bound {r['bound'].max():.3e}, max err/bound {(err / r['bound']).max():.3f}; "
          f"unshifted float32 form max err {fp32.max():.3e}")
    assert bool((err <= r["bound"]).all())
    mean_b = r["bound"].reshape(got.shape[0], -1).mean(axis=1)
    ps = per_sample.double().cpu().numpy()
    assert bool((np.abs(ps - r["per_sample"]) <= mean_b + 2 * U * np.abs(r["per_sample"])).all())
    assert abs(float(out[0]) - r["mean"]) <= mean_b.mean() + 2 * U * abs(r["mean"])
    assert abs(float(out[1]) - r["sum"]) <= mean_b.sum() + 2 * U * abs(r["sum"])
    # the map's own mean, in float64, is the per-sample value to one float32 ulp
    own = got.reshape(got.shape[0], -1).mean(axis=1)
    assert bool((np.abs(ps - own) <= np.spacing(np.abs(own).astype(np.float32)).astype(np.float64)).all())


# ----------------------------------------------------------------------------- map, reductions, determinism
@pytest.mark.parametrize("name", IDS)
def test_map_and_reductions_within_the_derived_bound(name):
    per_sample, out, smap = run(name)
    assert per_sample.dtype == out.dtype == smap.dtype == torch.float32 and per_sample.shape == (CASES[name][0][0],)
    check_against_ref(name, per_sample, out, smap)
    ps2, out2, map2 = run(name)                            # two calls: the same bits
    assert torch.equal(per_sample, ps2) and torch.equal(out, out2) and torch.equal(smap, map2)
    ps3, out3, none = run(name, return_map=False)          # with and without the map: the same bits
    assert none is None and torch.equal(per_sample, ps3) and torch.equal(out, out3)


@pytest.mark.parametrize("name", ["3d-vec-one-tile", "2d-vec", "1d-vec", "3d-7x11x15", "2d-cap-vec"])
def test_a_base_misaligned_by_one_float_gives_the_bits_of_the_aligned_call(name):
    """The same field, W % 4 == 0, once 16-byte aligned and once sliced one float into a larger buffer (the scalar loads)."""
    p, t = (x.to(DEV) for x in data(name))
    n = p.numel()
    bp, bt = torch.empty(n + 8, device=DEV), torch.empty(n + 8, device=DEV)
    assert bp.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0 and p.shape[-1] % VEC == 0
    p1, t1 = bp[1:n + 1].view(p.shape).copy_(p), bt[1:n + 1].view(t.shape).copy_(t)
    assert p1.data_ptr() % 16 == 4 and p1.is_contiguous()
    a, b = run(name), run(name, p=p1, t=t1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    check_against_ref(name, *b)


@pytest.mark.parametrize("name", ["3d-above-tile", "3d-vec-two-tiles", "2d-below-tile", "1d-vec", "3d-7x11x15", "3d-cap-tiles",
                                  "3d-window-1-in-d", "2d-range-none"])
def test_a_field_against_itself_is_exactly_one(name):
    from rho_diffusion_amd.engine import ops
    p = data(name)[0].to(DEV)
    m = metric(name)
    per_sample, out, smap = ops.ssim(p, p, m._device_windows(p.device, p.dim() - 2), m.range, m.clamp, m.k1, m.k2, True)
    assert bool((smap == 1.0).all()) and bool((per_sample == 1.0).all())
    assert float(out[0]) == 1.0 and float(out[1]) == float(p.shape[0])
    assert float(metric(name)(p, p)) == 1.0


# ----------------------------------------------------------------------------- the class
def test_reductions_shapes_and_the_map_of_the_class():
    name = "3d-vec-two-tiles"
    p, t = (x.to(DEV) for x in data(name))
    per_sample, out, smap = run(name)
    mean, vsum, none, none2 = (metric(name, reduction=r)(p, t) for r in ("elementwise_mean", "sum", "none", None))
    assert mean.dim() == 0 and vsum.dim() == 0 and none.shape == (3,) and mean.dtype == torch.float32 and mean.is_cuda
    assert torch.equal(mean, out[0]) and torch.equal(vsum, out[1]) and torch.equal(none, per_sample) and torch.equal(none2, per_sample)
    assert torch.equal(metric(name)(p, t), mean)                                     # the default
    v, m = metric(name, return_map=True)(p, t)
    assert torch.equal(v, mean) and torch.equal(m, smap) and m.shape == (3, 3, 2, 3, 34)
    # other dtypes and strides go through .float().contiguous()
    v2 = metric(name)(p.double().transpose(3, 4).contiguous().transpose(3, 4), t.double())
    assert torch.equal(v2, mean)


# ----------------------------------------------------------------------------- data_range
def test_data_range_none_is_the_float_mode_at_the_measured_extent():
    name = "2d-range-none"
    p, t = data(name)
    ext = max(float(p.max() - p.min()), float(t.max() - t.min()))       # float32 subtractions, as the range pass
    assert ext == float(p.max() - p.min()) > float(t.max() - t.min())   # preds is the wider one: target alone would be wrong
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    pd, td = p.to(DEV), t.to(DEV)
    assert float(ops.ssim_range(pd, td)) == ext and float(ops.ssim_range(td, pd)) == ext
    a = StructuralSimilarityIndexMeasure(data_range=None, reduction="none", return_map=True)(pd, td)
    b = StructuralSimilarityIndexMeasure(data_range=ext, reduction="none", return_map=True)(pd, td)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = StructuralSimilarityIndexMeasure(data_range=1.0, reduction="none")(pd, td)
    assert not torch.equal(a[0], c)


def test_a_data_range_pair_clamps_both_inputs():
    name = "3d-range-pair"
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    p, t = data(name)
    assert float(p.min()) < 0.0 and float(p.max()) > 1.0 and float(t.min()) < 0.0 and float(t.max()) > 1.0
    pd, td = p.to(DEV), t.to(DEV)
    a = StructuralSimilarityIndexMeasure(data_range=(0.0, 1.0), reduction="none", return_map=True)(pd, td)
    b = StructuralSimilarityIndexMeasure(data_range=1.0, reduction="none", return_map=True)(pd.clamp(0.0, 1.0), td.clamp(0.0, 1.0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    only_p = StructuralSimilarityIndexMeasure(data_range=1.0, reduction="none")(pd.clamp(0.0, 1.0), td)
    assert not torch.equal(a[0], only_p)


# ----------------------------------------------------------------------------- memory and the stream
@pytest.mark.parametrize("name", ["3d-above-tile", "2d-below-tile", "1d-vec", "3d-cap-tiles"])
def test_sentinels_around_the_outputs_are_untouched(name):
    from rho_diffusion_amd.engine import ops
    p, t = (x.to(DEV) for x in data(name))
    m = metric(name)
    B = p.shape[0]
    n_map = ref(name)["map"].size
    pad = 64
    bufs = [torch.full((n + 2 * pad,), -7.5, device=DEV) for n in (B, 2, n_map)]
    ps, out, smap = (b[pad:-pad] for b in bufs)
    ops.ssim(p, t, m._device_windows(p.device, p.dim() - 2), m.range, m.clamp, m.k1, m.k2, True, per_sample=ps, out=out,
             map=smap.view(ref(name)["map"].shape))
    for b in bufs:
        assert bool((b[:pad] == -7.5).all()) and bool((b[-pad:] == -7.5).all())
    ps0, out0, map0 = run(name)
    assert torch.equal(ps, ps0) and torch.equal(out, out0) and torch.equal(smap, map0.flatten())


@pytest.mark.parametrize("data_range", [1.0, None], ids=["float", "none"])
def test_a_call_neither_syncs_nor_breaks_a_graph_capture(data_range):
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    p, t = (x.to(DEV) for x in data("3d-vec-two-tiles"))
    m = StructuralSimilarityIndexMeasure(data_range=data_range, reduction="none", return_map=True)
    eager = [x.clone() for x in m(p, t)]                   # also uploads the windows, once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = m(p, t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again[0], eager[0]) and torch.equal(again[1], eager[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=side):
            out = m(p, t)
    except RuntimeError as exc:                            # not retried
        pytest.skip(f"graph capture refused: {exc}")
    out[0].zero_(), out[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ----------------------------------------------------------------------------- refusals of the library itself
@pytest.mark.parametrize("shape,ks,code", [((1, 1, 12, 10), (11, 11), "RHO_E_SHAPE"), ((1, 1, 10), (11,), "RHO_E_SHAPE"),
                                           ((1, 1, 4, 40, 40), (5, 5, 5), "RHO_E_SHAPE"),
                                           ((1, 1, 40, 40), (11, CAP + 2), "RHO_E_SHAPE"), ((1, 1, 40, 40), (10, 11), "RHO_E_SHAPE"),
                                           ((1, 1, 40, 40), (11, 0), "RHO_E_SHAPE")],
                         ids=["small-2d", "small-1d", "small-3d", "above-cap", "even", "empty-window"])
def test_rho_ssim_refuses_with_its_code_and_writes_nothing(shape, ks, code):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    p = torch.rand(shape, device=DEV)
    wins = [torch.full((max(k, 1),), 1.0 / max(k, 1), device=DEV)[:k] for k in ks]
    ps, out, smap = torch.full((1,), -7.5, device=DEV), torch.full((2,), -7.5, device=DEV), torch.full((4096,), -7.5, device=DEV)
    with pytest.raises(RhoHipError, match=code):
        ops.ssim(p, p, wins, 1.0, None, 0.01, 0.03, True, per_sample=ps, out=out, map=smap)
    torch.cuda.synchronize()
    assert bool((ps == -7.5).all()) and bool((out == -7.5).all()) and bool((smap == -7.5).all())


def test_rho_ssim_refuses_a_missing_range_and_a_short_workspace():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    p = torch.rand(1, 1, 12, 12, device=DEV)
    w = [torch.full((11,), 1.0 / 11, device=DEV)] * 2
    for bad in (0.0, -1.0):
        with pytest.raises(RhoHipError, match="RHO_E_ARG"):
            ops.ssim(p, p, w, bad)
    with pytest.raises(RhoHipError, match="RHO_E_ARG"):
        ops.ssim(p, p, w, 1.0, clamp=(1.0, 1.0))
    import ctypes as C
    sizes, ks, wp = (C.c_int64 * 2)(12, 12), (C.c_int64 * 2)(11, 11), (C.c_void_p * 2)(w[0].data_ptr(), w[1].data_ptr())
    out, ws = torch.full((3,), -7.5, device=DEV), torch.empty(4096, device=DEV)
    rc = hip.lib().rho_ssim(p.data_ptr(), p.data_ptr(), 1, 1, 2, sizes, wp, ks, 1.0, None, 0, 0.0, 0.0, 0.01, 0.03, out.data_ptr(),
                            out.data_ptr() + 4, None, ws.data_ptr(), 8, hip.stream())
    assert rc == -1
    rc = hip.lib().rho_ssim_range(p.data_ptr(), p.data_ptr(), p.numel(), out.data_ptr(), ws.data_ptr(), 1024, hip.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())


# ----------------------------------------------------------------------------- pipeline
def test_training_step_logs_train_ssim_and_leaves_the_loss_alone():
    from detdata import det_normal, det_state_dict, det_uniform
    from golden_cfg import UNET_CASES
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    from rho_diffusion_amd.models import UNet
    kw, xshape, _ = UNET_CASES["tiny2d"]
    x0 = det_uniform(xshape, "x0", 0.0, 1.0).to(DEV)
    eps = det_normal(xshape, "eps").to(DEV)
    tq = torch.tensor([3, 41])
    losses, logged = [], []
    for with_metric in (False, True):
        ddpm = DDPM(UNet, dict(kw, compute_dtype="fp32"), LinearSchedule(50, 1e-3, 0.02), nn.MSELoss, timesteps=50)
        ddpm.backbone.load_state_dict(det_state_dict(ddpm.backbone.state_dict(), "tiny2d"))
        ddpm = ddpm.to(DEV).train()
        if with_metric:
            ddpm.metrics["ssim"] = StructuralSimilarityIndexMeasure(data_range=1.0)
        ddpm.noise = lambda data: eps
        ddpm.random_timesteps = lambda bs: tq
        losses.append(ddpm.training_step(x0).detach().clone())
        logged.append(dict(ddpm._logged))
    assert torch.equal(losses[0], losses[1])
    assert "train_ssim" not in logged[0] and torch.equal(logged[1]["train_loss"].detach(), losses[1])
    xt, _ = ddpm.forward_process(x0, tq)
    wins = R.windows(2)
    r = R.ssim(xt.cpu().numpy(), x0.cpu().numpy(), wins, 1.0)
    bound = float(bound_of(r, wins).reshape(xshape[0], -1).mean(axis=1).mean()) + 2 * U * abs(r["mean"])
    got = logged[1]["train_ssim"]
    print(f"train_ssim {float(got)!r} vs {r['mean']!r}, bound {bound:.3e}")
    assert got.dim() == 0 and abs(float(got) - r["mean"]) <= bound
