"""-m gpu: rho_line_profile / SpectroscopyDataset on the device against the reference's items recorded in
tests/golden/g21_spectroscopy.npz and against a dense float64 restatement of spectroscopy.py:142-189 + :130 on the CPU (float32
differences and squares as the reference takes them, everything after in float64, every line at every grid point).

Bounds.  Rows are normalised to a maximum of 1, so the absolute error is relative to the peak.  The float32 evaluation differs from
the float64 one by the rounding of the per-item constant and of the product (|exponent| * 2^-23 relative on a term), the hardware
exponential (about 1 ulp) and the float32 sum; a float32 windowed restatement on the CPU gave 1.8e-7 .. 5.6e-7.  ABS_BOUND is four
times the worst value measured on an MI355X over the tests below (the figures are in DESIGN.md "Spectra on the device"), and
never above 5e-6.  The tail test is a condition, not a precision figure: a line skipped where it still matters gives a relative
error of 1.0."""
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV
from make_golden_g21 import CASES, SIM_WIDTH, build_fixture, sim_inputs, unit

pytestmark = pytest.mark.gpu

ABS_BOUND = 6.4e-7          # 4 x 1.6e-7, the worst row measured (the 3000-line item at width 1.3)
DEFAULT_GRID = np.linspace(1000, 32000, 50_000, dtype=np.float32)


def dense_profile(grid, centers, intensity, width, normalise=True, chunk=128):
    """spectroscopy.py:177-188 (+ :130): float32 (grid - c) ** 2 as the reference takes it, then float64; every line inside
    [grid.min(), grid.max()] at every grid point.  ``width``: a scalar or one per line."""
    grid = np.asarray(grid, dtype=np.float32)
    c, inten = np.asarray(centers, dtype=np.float32), np.asarray(intensity, dtype=np.float32)
    w = np.broadcast_to(np.asarray(width, dtype=np.float64), c.shape)
    mask = np.all([c <= grid.max(), grid.min() <= c], axis=0)
    c, inten, w = c[mask], inten[mask], w[mask]
    out = np.zeros(grid.shape, dtype=np.float64)
    for k in range(0, c.size, chunk):
        d2 = (grid[None, :] - c[k:k + chunk, None]) ** 2.0
        out += (inten[k:k + chunk, None] * np.exp(-d2 / (2 * w[k:k + chunk, None] ** 2.0))).sum(axis=0)
    if normalise:
        with np.errstate(invalid="ignore"):
            out = out / out.max() if out.size else out
    return out


def hashed_lines(n, salt, lo=1000.0, hi=32000.0, cluster=0):
    """n lines over [lo, hi] (a few percent outside it), log10 I in [-7, -2]; ``cluster`` of them near-degenerate around 20 000."""
    c = lo - 300.0 + (hi - lo + 600.0) * unit(n, salt)
    if cluster:
        c[:cluster] = 20000.0 + 0.004 * np.arange(cluster) + 0.5 * unit(cluster, salt + 50)
    logi = -7.0 + 5.0 * unit(n, salt + 100)
    return c.astype(np.float32), (10 ** logi.astype(np.float32))


def pack(items):
    """CSR tensors on the device of [(centers, intensity)] sorted by centre (stable)."""
    cs, is_, off = [], [], [0]
    for c, inten in items:
        o = np.argsort(c, kind="stable")
        cs.append(c[o])
        is_.append(inten[o])
        off.append(off[-1] + c.size)
    cat = lambda p: torch.from_numpy(np.concatenate(p).astype(np.float32)).to(DEV)          # noqa: E731
    return cat(cs), cat(is_), torch.tensor(off, dtype=torch.int64, device=DEV)


def check_row(got, ref, what):
    """got float32 [G] against the normalised float64 ref: the absolute bound, exactly 1.0 somewhere and nothing above it."""
    got = got.astype(np.float64)
    err = float(np.abs(got - ref).max())
    print(f"{what}: max abs error {err:.3e}")
    assert np.isfinite(got).all(), what
    assert got.max() == 1.0 and (got == 1.0).sum() >= 1, what
    assert err <= ABS_BOUND, f"{what}: max abs error {err:.3e}"
    return err


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(os.path.join(golden_dir, "g21_spectroscopy.npz"))


@pytest.fixture(scope="module")
def fixture_h5(tmp_path_factory):
    from rho_diffusion_amd import h5io
    p = tmp_path_factory.mktemp("spg") / "spectra.h5"
    h5io.write(p, build_fixture())
    return str(p)


@pytest.mark.parametrize("case", list(CASES))
def test_items_equal_the_reference(g21, fixture_h5, case):
    """ds[i] under the recorded seed: the reference's spectrum, max_int, members and key order; the all-out-of-range item is NaN."""
    import random
    from rho_diffusion_amd.data import SpectroscopyDataset
    kw, items, seed = CASES[case]
    ds = SpectroscopyDataset(fixture_h5, **kw)
    for i in items:
        random.seed(seed + i)
        data = ds[i]
        random.seed(seed + i)
        assert abs(random.gauss(1.0, 0.1)) == float(g21[f"{case}/{i}/width"])
        assert list(data.keys()) == list(g21[f"{case}/{i}/keys"])
        for k, v in data.items():
            ref = g21[f"{case}/{i}/{k}"]
            assert v.device.type == "cuda" and v.dtype == torch.float32 and tuple(v.shape) == ref.shape, (case, i, k)
            if k != "spectrum":
                assert np.array_equal(v.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (case, i, k)
        got, ref = data["spectrum"].cpu().numpy()[0], g21[f"{case}/{i}/spectrum"][0]
        if np.isnan(ref).any():
            assert i == 4 and np.isnan(ref).all() and np.isnan(got).all()
        else:
            check_row(got, ref.astype(np.float64), f"golden {case}/{i}")
    # the same rows through batch(index, widths)
    rows = [i for i in items if i != 4]
    widths = [float(g21[f"{case}/{i}/width"]) for i in rows]
    b = ds.batch(rows, widths=widths)
    assert b["spectrum"].shape == (len(rows), 1, ds.grid_size) and b["max_int"].shape == (len(rows), 1)
    for j, i in enumerate(rows):
        check_row(b["spectrum"][j, 0].cpu().numpy(), g21[f"{case}/{i}/spectrum"][0].astype(np.float64), f"golden batch {case}/{i}")
        assert float(b["max_int"][j, 0]) == float(g21[f"{case}/{i}/max_int"][0])
        assert np.array_equal(b["constants"][j].cpu().numpy(), g21[f"{case}/{i}/constants"])
    assert "zeta" not in b                                                  # only item 0 has it


def test_simulate_lineprofile_equals_the_reference(g21):
    """The unnormalised profile for a scalar width and for one width per line, relative to the reference's own maximum."""
    from rho_diffusion_amd.data import SpectroscopyDataset
    grid, c, inten, widths = sim_inputs()
    for name, w in (("scalar", SIM_WIDTH), ("per_line", widths)):
        ref = g21[f"sim/{name}"].astype(np.float64)
        for args in ((grid, c, inten, w), (torch.from_numpy(grid), torch.from_numpy(c).to(DEV), torch.from_numpy(inten), w)):
            got = SpectroscopyDataset.simulate_lineprofile(*args)
            assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == (grid.size,)
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / ref.max())
            print(f"simulate_lineprofile {name}: max abs error / max {err:.3e}")
            assert err <= ABS_BOUND, (name, err)
    # masked lines take their widths with them (the reference's broadcast fails here)
    c2 = np.concatenate([c, np.array([7000.0, 9500.0], dtype=np.float32)])
    i2 = np.concatenate([inten, np.array([1.0, 1.0], dtype=np.float32)])
    w2 = np.concatenate([widths, [50.0, 0.01]])
    got = SpectroscopyDataset.simulate_lineprofile(grid, c2, i2, w2).cpu().numpy().astype(np.float64)
    ref = g21["sim/per_line"].astype(np.float64)
    assert float(np.abs(got - ref).max() / ref.max()) <= ABS_BOUND
    # a decreasing grid is the same profile reversed
    rev = SpectroscopyDataset.simulate_lineprofile(grid[::-1].copy(), c, inten, widths).cpu().numpy()[::-1].astype(np.float64)
    assert float(np.abs(rev - ref).max() / ref.max()) <= ABS_BOUND


def test_batch_equals_the_dense_float64_restatement():
    """600 and 3000 lines on the default grid (the 3000 with a cluster of 150 near-degenerate lines), a short and an empty item in
    one batch, widths 0.73 / 1.0 / 1.13 / 1.3, repeated and unsorted indices."""
    from rho_diffusion_amd.engine import ops
    items = [hashed_lines(600, 1), hashed_lines(3000, 2, cluster=150), hashed_lines(0, 3), hashed_lines(37, 4)]
    centers, intensity, offsets = pack(items)
    grid = torch.from_numpy(DEFAULT_GRID).to(DEV)
    index = [1, 0, 3, 2, 1, 0, 3]
    widths = [1.0, 0.73, 1.13, 1.0, 1.3, 1.0, 1.3]
    got = ops.line_profile(grid, centers, intensity, offsets, torch.tensor(index, device=DEV),
                           torch.tensor(widths, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == (len(index), DEFAULT_GRID.size)
    worst = 0.0
    for b, (i, w) in enumerate(zip(index, widths)):
        c, inten = items[i]
        if c.size == 0:
            assert np.isnan(got[b]).all()
            continue
        ref = dense_profile(DEFAULT_GRID, c, inten, float(np.float32(w)))
        worst = max(worst, check_row(got[b], ref, f"dense item {i} ({c.size} lines) width {w}"))
    print(f"dense restatement: worst max abs error {worst:.3e}")
    # the unnormalised sums and per-line widths through the same entry
    lw = (0.7 + 0.6 * unit(int(offsets[-1]), 9)).astype(np.float32)
    o = np.argsort(items[0][0], kind="stable")
    raw = ops.line_profile(grid, centers, intensity, offsets, torch.tensor([0], device=DEV), torch.ones(1, device=DEV),
                           line_width=torch.from_numpy(lw).to(DEV), normalise=False)[0].cpu().numpy().astype(np.float64)
    ref = dense_profile(DEFAULT_GRID, items[0][0][o], items[0][1][o], lw[:600].astype(np.float64), normalise=False)
    err = float(np.abs(raw - ref).max() / ref.max())
    print(f"dense per-line widths: max abs error / max {err:.3e}")
    assert err <= ABS_BOUND


def tail_lines():
    """760 equal lines 40 MHz apart plus a slowly varying offset below 7.3 MHz (neighbours differ by at most 2 MHz: gap >= 38)."""
    k = np.arange(760)
    tri = np.abs(((k * 0.137) % 2.0) - 1.0)
    c = (1020.0 + 40.0 * k + 7.3 * tri).astype(np.float32)
    return c, np.full(c.shape, 1e-3, dtype=np.float32)


def tail_error(got, ref):
    """Largest relative error where the normalised float64 reference is >= 1e-25."""
    sel = ref >= 1e-25
    return float((np.abs(got.astype(np.float64)[sel] - ref[sel]) / ref[sel]).max()), int(sel.sum())


@pytest.mark.parametrize("width", [1.0, 1.3])
def test_tails_are_not_cut_short(width):
    """Every line contributes wherever the normalised reference is >= 1e-25 (down to 10.7 widths from a line): relative error <=
    1e-3 there.  A window cut at an exponent of -40 or -20 instead of -87 fails this with an error of 1.0."""
    from rho_diffusion_amd.engine import ops
    c, inten = tail_lines()
    assert np.diff(c).min() >= 37.0
    centers, intensity, offsets = pack([(c, inten)])
    got = ops.line_profile(torch.from_numpy(DEFAULT_GRID).to(DEV), centers, intensity, offsets, torch.zeros(1, dtype=torch.int64, device=DEV),
                           torch.tensor([width], dtype=torch.float32, device=DEV))[0].cpu().numpy()
    ref = dense_profile(DEFAULT_GRID, c, inten, float(np.float32(width)))
    err, n = tail_error(got, ref)
    print(f"tail width {width}: max relative error {err:.3e} over {n} points")
    assert n > 20_000
    assert err <= 1e-3, f"width {width}: max relative error {err:.3e} where the reference is >= 1e-25"


def test_batches_of_the_dataset(fixture_h5):
    """batch(B): shapes, an epoch of the permutation covers every item once, widths inside the distribution's support, max_int and
    the members gathered by the same rows."""
    from rho_diffusion_amd.data import SpectroscopyDataset
    ds = SpectroscopyDataset(fixture_h5, grid_size=4096, linewidth=(1.5, 0.05), seed=7)
    consts = np.stack([build_fixture()[f"{i}/constants"] for i in range(5)]).astype(np.float32)
    seen = []
    for B in (3, 2):
        b = ds.batch(B)
        assert list(b.keys()) == ["constants", "spectrum", "max_int", "width"]
        assert b["spectrum"].shape == (B, 1, 4096) and b["max_int"].shape == (B, 1) and b["constants"].shape == (B, 3)
        assert all(v.device.type == "cuda" and v.dtype == torch.float32 for v in b.values())
        rows = [int(np.flatnonzero((consts == r).all(axis=1))[0]) for r in b["constants"].cpu().numpy()]
        assert torch.equal(b["max_int"][:, 0].cpu(), ds.max_int[rows])
        w = b["width"].cpu()
        assert bool(((w > 1.5 - 6 * 0.05) & (w < 1.5 + 6 * 0.05)).all())          # Box-Muller on 32-bit uniforms stays within 6.7 sigma
        for j, r in enumerate(rows):
            s = b["spectrum"][j, 0].cpu().numpy()
            assert np.isnan(s).all() if r == 4 else (s.max() == 1.0 and s.min() >= 0.0)
        seen += rows
    ds.check_errors()
    assert sorted(seen) == [0, 1, 2, 3, 4]
    w1, w2 = ds.draw_widths(64), ds.draw_widths(64)
    assert not torch.equal(w1, w2) and abs(float(w1.mean()) - 1.5) < 0.05
    const = SpectroscopyDataset(fixture_h5, grid_size=4096, linewidth=0.8).batch(4)
    assert const["width"].tolist() == [np.float32(0.8)] * 4
    default = SpectroscopyDataset(fixture_h5, grid_size=4096).batch(5)["width"].cpu()
    assert bool(((default > 0.4) & (default < 1.6)).all()) and float(default.std()) > 0.01
    with pytest.raises(ValueError):
        ds.batch(6)


def test_out_of_range_index_raises_and_the_next_launch_succeeds(fixture_h5):
    from rho_diffusion_amd.data import SpectroscopyDataset
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    ds = SpectroscopyDataset(fixture_h5, grid_size=4096)
    grid = torch.from_numpy(ds.frequency_grid).to(DEV)
    for bad in ([0, 5], [-1]):
        with pytest.raises(RhoHipError, match="outside"):
            ops.line_profile(grid, ds.centers, ds.intensity, ds.offsets, torch.tensor(bad, device=DEV),
                             torch.ones(len(bad), device=DEV))
        with pytest.raises(RhoHipError, match="outside"):
            ds.batch(bad, widths=[1.0] * len(bad))
    with pytest.raises(IndexError):
        ds[5]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.line_profile(grid, ds.centers, ds.intensity, ds.offsets, torch.tensor([7], device=DEV), torch.ones(1, device=DEV), err_flag=flag)
    with pytest.raises(RhoHipError, match="outside"):
        ops.line_profile_check(flag)
    ops.line_profile_check(flag)                                            # the poll cleared it
    got = ds.batch([2, 0], widths=[1.0, 1.0])["spectrum"]
    assert float(got[0].max()) == 1.0 and float(got[1].max()) == 1.0


def test_training_step_on_spectra(fixture_h5):
    """The first real 1-D input of the engine: UNetv2(dims=1) DDPM.training_step on a grid-4096 batch; the loss is finite and an
    optimizer step runs."""
    from torch import nn
    from rho_diffusion_amd.data import SpectroscopyDataset
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    from rho_diffusion_amd.optim import HipAdamW
    ds = SpectroscopyDataset(fixture_h5, grid_size=4096)
    torch.manual_seed(21)
    kw = dict(dims=1, in_channels=1, out_channels=1, model_channels=32, num_res_blocks=1, data_shape=[4096],
              attention_resolutions=[], channel_mult=(1, 2, 2), use_scale_shift_norm=True, num_heads=4, activation="SiLU")
    ddpm = DDPM(UNet, kw, LinearSchedule(100), nn.MSELoss, timesteps=100).to(DEV)
    b = ds.batch([0, 1, 2, 3], widths=[1.0, 0.9, 1.1, 1.2])
    x = b["spectrum"]
    assert x.shape == (4, 1, 4096) and bool(torch.isfinite(x).all())
    opt = HipAdamW(ddpm.parameters(), lr=1e-4)
    for _ in range(2):
        opt.zero_grad()
        loss = ddpm.training_step({"data": x})
        loss.backward()
        opt.step()
        assert np.isfinite(float(loss.detach()))
