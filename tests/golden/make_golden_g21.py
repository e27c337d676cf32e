"""Generate tests/golden/g21_spectroscopy.npz from the REAL reference: SpectroscopyDataset (rho_diffusion/data/spectroscopy.py:35-189).

Run in the build container only:  ``python tests/golden/make_golden_g21.py``.  The reference module is imported in place through
``make_golden.load_reference`` (the stand-in-module recipe of make_golden_g20.py); ``h5py.File`` is a stand-in over the in-memory
arrays of ``build_fixture`` (context manager, ``len``, ``f[str(i)].items()`` in name order) - the same arrays the tests write into an
HDF5 file with ``h5io``.  einops is the real package.

What this pins, per case of ``CASES`` and item: the reference's ``ds[i]`` under ``random.seed(seed)`` - the spectrum, ``max_int``,
the other members, the key order and the width it drew (read by re-seeding and drawing once more) - for a 4096-point grid on the
default range (given as falsy bounds) and on a narrow custom range, and for one item on the default 50 000-point grid; and
``simulate_lineprofile`` for a scalar width and for one width per line (no masked line).  The fixture has lines outside the range on
both sides and exactly on both bounds (item 1), log10 intensities beyond both clip limits (item 1), transitions stored as float64
(item 2) and int32 (item 3), and an item whose every line is out of range (item 4: the reference divides 0 by 0, a NaN row).

The fixture is an integer hash: no RNG, rebuilt by the tests.  Only inputs' parameters and outputs are written, float32; nothing
here runs on the GPU box."""
from __future__ import annotations

import importlib
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (dataset kwargs, items, seed).  "wide" passes falsy bounds: the defaults 1000 / 32000 (spectroscopy.py:100-109)
CASES = {
    "wide": (dict(min_freq=0, max_freq=None, grid_size=4096), [0, 1, 2, 3, 4], 11),
    "narrow": (dict(min_freq=8000.0, max_freq=9000.0, grid_size=4096), [0, 1, 2, 3], 23),
    "default": (dict(), [0], 5),
}
SIM_GRID = (8000.0, 9000.0, 4096)        # np.linspace(*SIM_GRID, dtype=float32) of the simulate_lineprofile goldens
SIM_WIDTH = 0.9


def unit(n: int, salt: int) -> np.ndarray:
    """float64 [n] in [0, 1): a multiplicative hash of the element index."""
    a = np.arange(n, dtype=np.int64) + salt * 1000003
    return ((a * 2654435761) % (1 << 32)).astype(np.float64) / float(1 << 32)


def build_fixture() -> dict:
    """{"<i>/transitions": [2, C], "<i>/constants": [3], ...}: five items, see the module docstring."""
    out = {}
    # 0: 300 lines over the default range and 60 more inside [8000, 9000]
    c = np.concatenate([1000.0 + 31000.0 * unit(300, 1), 8000.0 + 1000.0 * unit(60, 2)])
    li = np.concatenate([-7.0 + 4.5 * unit(300, 3), -6.0 + 3.0 * unit(60, 4)])
    out["0/transitions"] = np.stack([c, li]).astype(np.float32)
    out["0/constants"] = np.array([5123.25, 1804.5, 1290.125], dtype=np.float64)
    out["0/zeta"] = np.array([[1, -2], [3, 40000]], dtype=np.int32)          # sorts after "transitions"
    # 1: outside on both sides, exactly on the bounds of both ranges, log10 I beyond both clip limits
    c = np.array([500.0, 999.5, 1000.0, 1000.5, 7999.5, 8000.0, 8000.25, 8500.0, 8999.75, 9000.0, 9000.5, 15000.0, 31999.5, 32000.0,
                  32000.5, 40000.0])
    li = np.array([-3.0, -2.5, -12.0, -4.0, -1.0, -3.5, -11.0, 0.5, -2.0, -10.0, -2.25, -1.5, -3.0, -2.75, -1.0, -2.0])
    out["1/transitions"] = np.stack([c, li]).astype(np.float32)
    out["1/constants"] = np.array([1.0, 2.0, 3.0], dtype=np.float64)
    # 2: float64 transitions that float32 does not hold exactly
    c = np.concatenate([1000.0 + 31000.0 * unit(40, 5) + 1e-7, 8000.0 + 1000.0 * unit(25, 6) + 1e-7])
    li = np.concatenate([-6.0 + 3.5 * unit(40, 7), -5.0 + 2.0 * unit(25, 8)])
    out["2/transitions"] = np.stack([c, li]).astype(np.float64)
    out["2/constants"] = np.array([0.1, 0.2, 0.3], dtype=np.float64)
    # 3: int32 transitions (integer centres, integer log10 intensities, some beyond the clip limits)
    c = np.array([31000, 8100, 8100, 8101, 8800, 2000, 8450, 8449, 12, 99999], dtype=np.int32)
    li = np.array([-3, -4, -5, -3, -20, -2, 0, -6, -3, -3], dtype=np.int32)
    out["3/transitions"] = np.stack([c, li])
    out["3/constants"] = np.array([7.0, 8.0, 9.0], dtype=np.float64)
    # 4: every line out of range
    out["4/transitions"] = np.array([[100.0, 500.0, 40000.0], [-3.0, -2.5, -4.0]], dtype=np.float32)
    out["4/constants"] = np.array([0.0, 0.0, 0.0], dtype=np.float64)
    return out


def sim_inputs():
    """(grid float32, centers float32, intensities float32 (linear), per-line widths float64) of the simulate_lineprofile goldens:
    every line inside the grid, as the reference's per-line broadcast needs."""
    grid = np.linspace(*SIM_GRID, dtype=np.float32)
    c = (8000.0 + 1000.0 * unit(80, 9)).astype(np.float32)
    inten = (10 ** (-6.0 + 4.0 * unit(80, 10))).astype(np.float32)
    widths = np.array([0.75, 1.0, 1.25, 0.875, 1.5], dtype=np.float64)[np.arange(80) % 5]
    return grid, c, inten, widths


def main():
    sys.path.insert(0, HERE)
    from make_golden import load_reference
    load_reference()
    arrays = build_fixture()
    n_items = len({k.split("/")[0] for k in arrays})

    class Group:
        def __init__(self, name):
            self.name = name

        def items(self):
            return sorted((k.split("/")[1], v) for k, v in arrays.items() if k.split("/")[0] == self.name)

    class File:
        """h5py.File over the fixture arrays."""

        def __init__(self, fn, mode="r"):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def __len__(self):
            return n_items

        def __getitem__(self, name):
            return Group(name)

    sys.modules["h5py"].File = File
    SP = importlib.import_module("rho_diffusion.data.spectroscopy")
    g = {}
    for name, (kw, items, seed) in CASES.items():
        ds = SP.SpectroscopyDataset(os.path.abspath(__file__), **kw)      # any existing path: the stand-in File ignores it
        g[f"{name}/frequency_grid"] = ds.frequency_grid
        try:
            len(ds)
            g[f"{name}/len_error"] = np.array("")
        except Exception as exc:                                          # noqa: BLE001 - the reference's own failure is what is pinned
            g[f"{name}/len_error"] = np.array(type(exc).__name__)
        for i in items:
            random.seed(seed + i)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                           # item 4: 0 / 0
                data = ds[i]
            random.seed(seed + i)
            g[f"{name}/{i}/width"] = np.float64(np.abs(random.gauss(1.0, 0.1)))
            g[f"{name}/{i}/keys"] = np.array(list(data.keys()))
            for k, v in data.items():
                assert v.dtype.is_floating_point and v.element_size() == 4
                g[f"{name}/{i}/{k}"] = v.numpy()
    grid, c, inten, widths = sim_inputs()
    g["sim/scalar"] = SP.SpectroscopyDataset.simulate_lineprofile(grid, c, inten, SIM_WIDTH).astype(np.float32)
    g["sim/per_line"] = SP.SpectroscopyDataset.simulate_lineprofile(grid, c, inten, widths).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "g21_spectroscopy.npz"), **g)
    print({k: v.shape for k, v in g.items()})
    print(os.path.getsize(os.path.join(HERE, "g21_spectroscopy.npz")), "bytes")


if __name__ == "__main__":
    main()
