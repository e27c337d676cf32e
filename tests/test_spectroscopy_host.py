"""CPU: SpectroscopyDataset's host side against the real reference (tests/golden/g21_spectroscopy.npz, tests/golden/make_golden_g21.py):
registry entry, metadata (len, frequency_grid, max_int, the other members, key order, falsy bounds), the CSR packing of the lines,
the missing-file assertion, the CPU device, batch()'s width rule, the new C-ABI symbol."""
import os
import re

import numpy as np
import pytest
import torch

from rho_diffusion_amd import h5io
from make_golden_g21 import CASES, build_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_h5 = pytest.mark.skipif(not h5io.available(), reason="libhdf5 not found on this machine")


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(os.path.join(golden_dir, "g21_spectroscopy.npz"))


@pytest.fixture(scope="module")
def fixture_h5(tmp_path_factory):
    p = tmp_path_factory.mktemp("sp") / "spectra.h5"
    h5io.write(p, build_fixture())
    return str(p)


def test_registry_entry_and_exports():
    from rho_diffusion_amd import data, registry
    from rho_diffusion_amd.data import SpectroscopyDataset
    assert registry.get("datasets", "SpectroscopyDataset") is SpectroscopyDataset
    assert "SpectroscopyDataset" in data.__all__


def test_line_profile_symbol_in_header_and_binding():
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    assert re.search(r"\brho_line_profile\s*\(", header) and "rho_line_profile" in hip.SIGNATURES
    assert "spectroscopy.py:111-189" in header
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION
    assert callable(ops.line_profile) and callable(ops.line_profile_check)
    from rho_diffusion_amd import build
    assert "spectrum.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "spectrum.hip"))


@needs_h5
@pytest.mark.parametrize("case", list(CASES))
def test_metadata_follows_the_reference(g21, fixture_h5, case):
    from rho_diffusion_amd.data import SpectroscopyDataset
    kw, items, _ = CASES[case]
    ds = SpectroscopyDataset(fixture_h5, device="cpu", **kw)
    assert str(g21[f"{case}/len_error"]) == "TypeError"             # the reference's len(ds) raises; here it is the group count
    assert len(ds) == 5
    grid = ds.frequency_grid
    assert grid.dtype == np.float32 and np.array_equal(grid.view(np.uint32), g21[f"{case}/frequency_grid"].view(np.uint32))
    assert ds.frequency_grid is grid
    for i in items:
        keys = list(g21[f"{case}/{i}/keys"])
        meta = ds.metadata(i)
        assert keys[-2:] == ["spectrum", "max_int"] and "transitions" not in keys
        assert list(meta.keys()) == keys[:-2] + ["max_int"]
        for k, v in meta.items():
            ref = g21[f"{case}/{i}/{k}"]
            assert v.dtype == torch.float32 and tuple(v.shape) == ref.shape
            assert np.array_equal(v.numpy().view(np.uint32), ref.view(np.uint32)), (case, i, k)


@needs_h5
def test_falsy_bounds_mean_the_defaults(fixture_h5):
    from rho_diffusion_amd.data import SpectroscopyDataset
    ref = np.linspace(1000, 32000, 64, dtype=np.float32)
    for lo, hi in ((None, None), (0, 0), (0.0, None), (1000, 32000)):
        assert np.array_equal(SpectroscopyDataset(fixture_h5, lo, hi, grid_size=64, device="cpu").frequency_grid, ref)
    assert np.array_equal(SpectroscopyDataset(fixture_h5, 5.0, 7.0, grid_size=9, device="cpu").frequency_grid,
                          np.linspace(5.0, 7.0, 9, dtype=np.float32))
    assert SpectroscopyDataset(fixture_h5, device="cpu").grid_size == 50_000


@needs_h5
def test_lines_are_packed_sorted_and_clipped_as_numpy_does(fixture_h5):
    from rho_diffusion_amd.data import SpectroscopyDataset
    from rho_diffusion_amd.data.spectroscopy import pack_lines
    fx = build_fixture()
    ds = SpectroscopyDataset(fixture_h5, device="cpu")
    offsets = ds.offsets.numpy()
    counts = [fx[f"{i}/transitions"].shape[1] for i in range(5)]
    assert ds.offsets.dtype == torch.int64 and list(offsets) == [0] + list(np.cumsum(counts))
    assert ds.centers.dtype == ds.intensity.dtype == torch.float32 and ds.centers.numel() == ds.intensity.numel() == sum(counts)
    for i in range(5):
        c, li = np.array(fx[f"{i}/transitions"]).astype(np.float32)
        inten = 10 ** np.clip(li, -10.0, -2.0)
        assert inten.dtype == np.float32
        order = np.argsort(c, kind="stable")
        got_c, got_i = ds.centers.numpy()[offsets[i]:offsets[i + 1]], ds.intensity.numpy()[offsets[i]:offsets[i + 1]]
        assert np.all(np.diff(got_c) >= 0)
        assert np.array_equal(got_c.view(np.uint32), c[order].view(np.uint32))
        assert np.array_equal(got_i.view(np.uint32), inten[order].view(np.uint32))
        assert float(ds.max_int[i]) == float(np.float32(10 ** np.clip(li, -10.0, -2.0).max()))
    # stable: equal centres keep their file order (item 3 has 8100 twice, with intensities 1e-4 then 1e-5)
    c3 = ds.centers.numpy()[offsets[3]:offsets[4]]
    i3 = ds.intensity.numpy()[offsets[3]:offsets[4]]
    first = int(np.flatnonzero(c3 == 8100.0)[0])
    assert c3[first + 1] == 8100.0 and 0.99e-4 < i3[first] < 1.01e-4 and 0.99e-5 < i3[first + 1] < 1.01e-5
    # an item without lines: an empty range, max_int NaN
    c, inten, off, mx = pack_lines([np.zeros((2, 0)), np.array([[3.0, 1.0], [-3.0, -30.0]])])
    assert list(off) == [0, 0, 2] and np.isnan(mx[0]) and list(c) == [1.0, 3.0]
    assert np.array_equal(inten, 10 ** np.array([-10.0, -3.0], dtype=np.float32))
    with pytest.raises(ValueError):
        pack_lines([np.zeros((3, 4))])


def test_missing_file_assertion_has_the_reference_message(tmp_path):
    from rho_diffusion_amd.data import SpectroscopyDataset
    missing = tmp_path / "nope.h5"
    with pytest.raises(AssertionError, match=re.escape(f"Target HDF5 not found; passed {missing}.")):
        SpectroscopyDataset(str(missing), device="cpu")
    with pytest.raises(AssertionError, match="two-tuple"):
        SpectroscopyDataset(__file__, linewidth=(1.0, 0.1, 0.2), device="cpu")


@needs_h5
def test_cpu_device_has_no_spectrum_path(fixture_h5):
    from rho_diffusion_amd.data import SpectroscopyDataset
    from rho_diffusion_amd.hip import RhoHipError
    ds = SpectroscopyDataset(fixture_h5, grid_size=128, device="cpu")
    with pytest.raises(RhoHipError):
        ds[0]
    with pytest.raises(RhoHipError):
        ds.batch(2)
    with pytest.raises(RhoHipError):
        ds.batch([0, 1], widths=[1.0, 1.0])
    with pytest.raises(RhoHipError):
        SpectroscopyDataset.simulate_lineprofile(ds.frequency_grid, np.array([1500.0]), np.array([1e-3]), 1.0, device="cpu")
    with pytest.raises(IndexError):
        ds.metadata(5)
    assert float(ds.metadata(-1)["max_int"]) == float(ds.max_int[4])


@needs_h5
def test_width_rule_of_batch(fixture_h5):
    """The reference's linewidth property (:61-71): a float is a constant width, a 2-tuple is (mu, sigma), anything else (an int
    included) is (1.0, 0.1)."""
    from rho_diffusion_amd.data import SpectroscopyDataset
    mk = lambda lw: SpectroscopyDataset(fixture_h5, grid_size=64, linewidth=lw, device="cpu")          # noqa: E731
    assert mk(None).width_rule() == (1.0, 0.1)
    assert mk(0.8).width_rule() == (0.8, 0.0)
    assert mk((1.4, 0.25)).width_rule() == (1.4, 0.25)
    assert mk(2).width_rule() == (1.0, 0.1)
    ds = mk(-0.75)
    w = ds.draw_widths(5)                                                   # a constant width needs no GPU
    assert w.dtype == torch.float32 and w.tolist() == [0.75] * 5
    assert ds.linewidth == -0.75


def test_simulate_lineprofile_rejects_bad_arguments():
    from rho_diffusion_amd.data import SpectroscopyDataset
    sim = SpectroscopyDataset.simulate_lineprofile
    grid = np.linspace(0.0, 1.0, 16, dtype=np.float32)
    with pytest.raises(ValueError, match="monotone"):
        sim(np.array([0.0, 2.0, 1.0], dtype=np.float32), np.array([1.0]), np.array([1.0]), 1.0, device="cpu")
    with pytest.raises(ValueError):
        sim(grid, np.array([0.5, 0.6]), np.array([1.0]), 1.0, device="cpu")
    with pytest.raises(ValueError):
        sim(grid, np.array([0.5, 0.6, 0.7]), np.array([1.0, 1.0, 1.0]), np.array([1.0, 2.0]), device="cpu")
