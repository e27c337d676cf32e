"""CPU: the host side of StructuralSimilarityIndexMeasure (rho_diffusion_amd/metrics/ssim.py, csrc/ssim.hip) - the float64
restatement of tests/ssim_ref.py against a brute-force n-D window sum and against scipy, the window rule, known answers, the surface
(symbols declared, bound, exported; ABI version) and every refusal that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_SYMBOLS = ["rho_ssim_max_window", "rho_ssim_workspace_bytes", "rho_ssim_range", "rho_ssim"]


def _cls():
    from rho_diffusion_amd.metrics import StructuralSimilarityIndexMeasure
    return StructuralSimilarityIndexMeasure


def _err():
    from rho_diffusion_amd.hip import RhoHipError
    return RhoHipError


def _pair(shape, seed):
    g = np.random.default_rng(seed)
    t = g.random(shape)
    return t + 0.1 * g.standard_normal(shape), t


# ----------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("shape,sigma", [((2, 2, 9), (0.8,)), ((1, 2, 8, 6), (0.8, 0.5)), ((2, 1, 6, 8, 6), (0.5, 0.8, 0.5))],
                         ids=["1d", "2d", "3d"])
def test_restatement_against_brute_force_outer_product_window(shape, sigma):
    """Anisotropic windows (7 and 5 taps), every window position by explicit loops with the full n-D window."""
    p, t = _pair(shape, 1)
    wins = R.windows(len(shape) - 2, True, sigma)
    assert sorted({len(w) for w in wins}) in ([7], [5, 7])
    got = R.ssim(p, t, wins, data_range=1.0)
    want = R.brute_force(p, t, wins, 1.0)
    assert got["map"].shape == want.shape == shape[:2] + tuple(s - len(w) + 1 for s, w in zip(shape[2:], wins))
    assert float(np.abs(got["map"] - want).max()) <= 1e-12
    assert np.allclose(got["per_sample"], want.reshape(shape[0], -1).mean(1), rtol=0, atol=1e-12)
    assert abs(got["mean"] - want.reshape(shape[0], -1).mean(1).mean()) <= 1e-12 and abs(got["sum"] - shape[0] * got["mean"]) <= 1e-12


@pytest.mark.parametrize("shape", [(1, 1, 20), (1, 2, 14, 17), (1, 1, 12, 13, 15)], ids=["1d", "2d", "3d"])
def test_restatement_against_scipy_correlate1d_cropped_to_the_valid_region(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    p, t = _pair(shape, 2)
    nd = len(shape) - 2
    wins = R.windows(nd)

    def W(x):
        for d, g in enumerate(wins):
            x = ndimage.correlate1d(x, g.astype(np.float64), axis=2 + d, mode="reflect")
        crop = (slice(None), slice(None)) + tuple(slice(len(g) // 2, x.shape[2 + d] - len(g) // 2) for d, g in enumerate(wins))
        return x[crop]

    got = R.ssim(p, t, wins, data_range=1.0)
    assert float(np.abs(got["mu_p"] - W(p)).max()) <= 1e-13 and float(np.abs(got["mu_t"] - W(t)).max()) <= 1e-13
    assert float(np.abs(got["s_pt"] - (W(p * t) - W(p) * W(t))).max()) <= 1e-13
    assert float(np.abs(got["s_pp"] - np.maximum(W(p * p) - W(p) ** 2, 0)).max()) <= 1e-13


def test_shifted_moments_give_the_same_variances_up_to_the_window_sum():
    """With s the shift and 1 + delta the sum of the n-D window (float32 taps: delta is a few 1e-8, not 0), in exact arithmetic
    W[a a] - W[a]^2 = s_pp + delta s (2 W[p] - s) - delta^2 s^2, W[a b] - W[a] W[b] likewise with W[p] + W[t], and
    s + W[a] = mu_p - delta s.  The GPU test's bound carries these three terms."""
    p, t = _pair((2, 2, 13, 12), 3)
    wins = R.windows(2)
    delta = float(np.prod([w.astype(np.float64).sum() for w in wins])) - 1.0
    assert 0.0 < abs(delta) <= 4 * 2.0 ** -24
    r = R.ssim(p + 5.0, t + 5.0, wins, data_range=1.0)
    s = r["shift"]
    gap = delta * s * (2 * r["mu_p"] - s) - delta ** 2 * s ** 2
    assert float(np.abs(r["w_aa"] - r["w_a"] ** 2 - r["s_pp"] - gap).max()) <= 1e-12
    gap = delta * s * (r["mu_p"] + r["mu_t"] - s) - delta ** 2 * s ** 2
    assert float(np.abs(r["w_ab"] - r["w_a"] * r["w_b"] - r["s_pt"] - gap).max()) <= 1e-12
    assert bool((r["w_abs_ab"] >= np.abs(r["w_ab"])).all())
    assert float(np.abs(s + r["w_b"] - r["mu_t"] + delta * s).max()) <= 1e-12


# ----------------------------------------------------------------------------- the window rule
def test_window_rule():
    from rho_diffusion_amd.metrics.ssim import ssim_window
    m = _cls()()
    assert [len(w) for w in m.windows(3)] == [11, 11, 11] and [len(w) for w in m.windows(1)] == [11]
    # Gaussian: the size follows sigma, kernel_size is ignored
    assert [len(w) for w in _cls()(sigma=(0.8, 1.5, 2.0), kernel_size=3).windows(3)] == [7, 11, 15]
    assert len(ssim_window(True, 0.5, 11)) == 5
    for sigma in (0.5, 0.8, 1.5, 2.0):
        w = ssim_window(True, sigma, 11)
        assert w.dtype == np.float32 and np.array_equal(w, R.window(True, sigma, 11)) and np.array_equal(w, w[::-1])
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
        k = len(w)
        g = np.exp(-(((np.arange(k) - (k - 1) / 2) / sigma) ** 2) / 2)
        assert np.array_equal(w, (g / g.sum()).astype(np.float32))
    # uniform: 1 / k, kernel_size per dimension
    u = _cls()(gaussian_kernel=False, kernel_size=(3, 7)).windows(2)
    assert [len(w) for w in u] == [3, 7]
    assert np.array_equal(u[0], np.full(3, np.float32(1.0 / 3))) and np.array_equal(u[1], np.full(7, np.float32(1.0 / 7)))
    for w in u + [ssim_window(False, 1.5, 1), ssim_window(False, 1.5, 15)]:
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
    assert np.array_equal(ssim_window(False, 1.5, 1), np.ones(1, np.float32))


# ----------------------------------------------------------------------------- known answers
def test_a_field_against_itself_is_one():
    p, _ = _pair((2, 3, 12, 14), 4)
    r = R.ssim(p, p, R.windows(2), data_range=1.0)
    assert float(np.abs(r["map"] - 1.0).max()) <= 1e-15 and abs(r["mean"] - 1.0) <= 1e-15 and abs(r["sum"] - 2.0) <= 1e-15


def test_data_range_none_takes_the_larger_extent():
    p, t = _pair((1, 1, 16, 16), 5)
    p = 3.0 * p                                           # preds has the larger extent
    ext = max(p.max() - p.min(), t.max() - t.min())
    assert ext == p.max() - p.min() > t.max() - t.min()
    a, b = R.ssim(p, t, R.windows(2), data_range=None), R.ssim(p, t, R.windows(2), data_range=float(ext))
    assert a["R"] == ext and np.array_equal(a["map"], b["map"])
    c = R.ssim(t, p, R.windows(2), data_range=None)      # and the other way round
    assert c["R"] == ext


def test_clamp_is_applied_to_both_inputs():
    p, t = _pair((1, 2, 12, 12), 6)
    p, t = 2.0 * p - 0.5, 2.0 * t - 0.5
    assert p.min() < 0.0 < 1.0 < p.max() and t.min() < 0.0 < 1.0 < t.max()
    a = R.ssim(p, t, R.windows(2), data_range=(0.0, 1.0))
    b = R.ssim(np.clip(p, 0.0, 1.0), np.clip(t, 0.0, 1.0), R.windows(2), data_range=1.0)
    assert a["R"] == 1.0 and np.array_equal(a["map"], b["map"])
    only_p = R.ssim(np.clip(p, 0.0, 1.0), t, R.windows(2), data_range=1.0)
    assert not np.array_equal(a["map"], only_p["map"])


# ----------------------------------------------------------------------------- surface
def test_symbols_declared_bound_and_exported():
    from rho_diffusion_amd import hip
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    declared = set(re.findall(r"\b(rho_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    if not os.path.exists(hip.LIB_PATH):
        from rho_diffusion_amd.build import build
        build(verbose=False)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in SSIM_SYMBOLS:
        assert name in declared, name
        assert name in hip.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(hip.SIGNATURES["rho_ssim"][1]) == 21 and hip.SIGNATURES["rho_ssim"][1][8] == ctypes.c_float
    assert len(hip.SIGNATURES["rho_ssim_range"][1]) == 7
    for name in SSIM_SYMBOLS:                               # each declaration's comment cites the reference
        comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*[a-z0-9_ ]*\b" + name + r"\s*\(", header, flags=re.S)
        assert comment and "abstract_diffusion.py:31,79" in comment.group(1), name
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == hip.ABI_VERSION
    lib.rho_abi_version.restype = ctypes.c_int
    assert lib.rho_abi_version() == 10


def test_window_cap_and_workspace_query_without_a_gpu():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    lib = hip.load()
    cap = int(lib.rho_ssim_max_window())
    assert cap >= 15 and cap == ops.SSIM_MAX_WINDOW

    def ws(sizes, ks, batch=2, channels=3):
        n = len(sizes)
        return int(lib.rho_ssim_workspace_bytes(batch, channels, n, (ctypes.c_int64 * n)(*sizes), (ctypes.c_int64 * n)(*ks)))

    assert ws((64, 64, 64), (11, 11, 11)) >= 16384 and ws((11,), (11,)) >= 16384
    assert ws((10, 64), (11, 11)) == -1 and ws((64, 64), (11, cap + 2)) == -1 and ws((64, 64), (10, 11)) == -1
    assert ws((64, 64), (11, 11), batch=0) == -1


def test_exported_from_the_metrics_package_and_keywords():
    import inspect
    import rho_diffusion_amd.metrics as M
    assert "StructuralSimilarityIndexMeasure" in M.__all__ and M.StructuralSimilarityIndexMeasure is M.ssim.StructuralSimilarityIndexMeasure
    sig = inspect.signature(M.StructuralSimilarityIndexMeasure.__init__)
    want = dict(gaussian_kernel=True, sigma=1.5, kernel_size=11, reduction="elementwise_mean", data_range=None, k1=0.01, k2=0.03,
                return_map=False)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert isinstance(M.StructuralSimilarityIndexMeasure(), torch.nn.Module)
    assert not hasattr(M.StructuralSimilarityIndexMeasure, "update") and not hasattr(M.StructuralSimilarityIndexMeasure, "compute")


# ----------------------------------------------------------------------------- refusals, none of which needs a GPU
@pytest.mark.parametrize("kw", [dict(kernel_size=10), dict(kernel_size=0), dict(kernel_size=-3), dict(gaussian_kernel=False, kernel_size=4),
                                dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=(1.5, 0.0)), dict(sigma=4.5),
                                dict(gaussian_kernel=False, kernel_size=17), dict(reduction="mean"), dict(data_range=0.0),
                                dict(data_range=-1.0), dict(data_range=(1.0, 1.0)), dict(data_range=(1.0, 0.0)),
                                dict(sigma=(1.5, 1.5), kernel_size=(11, 11, 11))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_constructor_refusals(kw):
    with pytest.raises(_err()):
        _cls()(**kw)


@pytest.mark.parametrize("kw,pshape,tshape", [
    (dict(), (2, 1, 16, 16), (2, 1, 16, 17)),                      # shape mismatch
    (dict(), (16, 16), (16, 16)),                                  # rank 2
    (dict(), (1, 1, 12, 12, 12, 12), (1, 1, 12, 12, 12, 12)),      # rank 6
    (dict(sigma=(1.5, 1.5)), (1, 1, 12, 12, 12), (1, 1, 12, 12, 12)),                       # two sigmas, three dimensions
    (dict(gaussian_kernel=False, kernel_size=(3, 3, 3)), (1, 1, 12, 12), (1, 1, 12, 12)),   # three sizes, two dimensions
    (dict(), (1, 1, 12, 10), (1, 1, 12, 10)),                      # a size below its window
    (dict(), (1, 1, 10), (1, 1, 10)),
    (dict(sigma=(0.5, 2.0)), (1, 1, 20, 14), (1, 1, 20, 14)),
], ids=["mismatch", "rank2", "rank6", "sigma-len", "ksize-len", "small-2d", "small-1d", "small-aniso"])
def test_forward_refusals_come_before_the_gpu_check(kw, pshape, tshape):
    m = _cls()(**kw)
    with pytest.raises(_err()) as exc:
        m(torch.zeros(pshape), torch.zeros(tshape))
    assert "must live on the GPU" not in str(exc.value)


def test_cpu_tensors_of_a_valid_shape_are_refused_by_the_gpu_check():
    with pytest.raises(_err(), match="must live on the GPU"):
        _cls()()(torch.zeros(1, 1, 12, 12), torch.zeros(1, 1, 12, 12))
