"""The reference's SpectroscopyDataset (rho_diffusion/data/spectroscopy.py:35-189) with its line profiles computed on the device.

The file layout is the reference's: root groups ``"0" .. "N-1"``, each with ``transitions`` [2, C] (row 0 the line centres, row 1
their log10 intensities, any numeric dtype, cast to float32) and any number of other numeric members.  The HDF5 file is read once,
through ``h5io`` (h5py is not needed).

The reference opens the file in every ``__getitem__`` and builds a float64 [lines, grid_size] temporary on the host (0.4 - 3 s per
item on the default grid).  Here the lines of all items are packed once in CSR form, sorted by centre inside an item, with the clip
to [-10, -2] and ``10 **`` already applied in numpy (bit-equal to the reference's float32 values), and stay resident on the GPU;
``rho_line_profile`` evaluates a whole batch in float32, visiting only the lines within reach of each tile of grid points, and
divides by the row maximum.  ``batch(B)`` is what a training loop should call.

Where this differs from the reference:
  * ``len(ds)`` returns the number of root groups (the reference's ``__len__`` is a cached_property, so ``len(ds)`` raises TypeError);
  * the spectrum is summed in float32 (the reference takes float32 differences and squares, then sums in float64);
  * ``simulate_lineprofile`` with one width per line also works when lines fall outside the grid (the mask applies to the widths;
    the reference's broadcast fails there), needs a monotone grid, and returns a float32 tensor on the device;
  * an item without transitions has ``max_int`` NaN and a NaN spectrum (the reference raises on its empty ``max``);
  * a CPU ``device`` loads the metadata only and raises RhoHipError on any spectrum."""
from __future__ import annotations

import random
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from .. import h5io, hip
from ..engine import ops
from ..registry import registry

__all__ = ["SpectroscopyDataset"]


def pack_lines(transitions) -> tuple:
    """CSR packing of per-item ``transitions`` [2, C]: (centers float32 [total], intensity float32 [total], offsets int64 [N + 1],
    max_int float32 [N]).  Inside an item the lines are sorted by centre (stable); intensity = 10 ** clip(log10 I, -10, -2) in
    float32 and max_int = 10 ** max(clipped), masked lines included, both as spectroscopy.py:121-129 computes them."""
    centers, intensity, offsets, max_int = [], [], [0], []
    for t in transitions:
        t = np.array(t).astype(np.float32)
        if t.ndim != 2 or t.shape[0] != 2:
            raise ValueError(f"transitions must be [2, C] (centres, log10 intensities), got {t.shape}")
        c, logi = t
        logi = np.clip(logi, -10.0, -2.0)
        order = np.argsort(c, kind="stable")
        centers.append(c[order])
        intensity.append((10 ** logi)[order])
        max_int.append(10 ** logi.max() if logi.size else np.float32("nan"))
        offsets.append(offsets[-1] + c.shape[0])
    cat = lambda parts: np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, np.float32)       # noqa: E731
    return cat(centers), cat(intensity), np.asarray(offsets, dtype=np.int64), np.asarray(max_int, dtype=np.float32)


@registry.register_dataset("SpectroscopyDataset")
class SpectroscopyDataset(torch.utils.data.Dataset):
    """spectroscopy.py:35-189.  Constructor of the reference plus ``device`` (the lines live there).

    ``ds[i]``: dict of the group's other members in name order (float32), then ``"spectrum"`` float32 [1, grid_size] and
    ``"max_int"`` float32 [1], all on the device.  The width is ``abs(random.gauss(1.0, 0.1))`` from Python's ``random``, as
    spectroscopy.py:118 draws it (``linewidth`` is ignored there, as in the reference): under the same ``random.seed`` the item is
    the reference's.

    ``batch(B)`` draws B rows of a device-side permutation (a shuffled epoch; a new permutation when fewer than B rows are left),
    ``batch(index, widths=None)`` takes the given rows; both return a dict of [B, ...] tensors on the device with one profile
    launch.  Without ``widths`` they are drawn on the device (rho_philox_normal) by the rule of the reference's ``linewidth``
    property (:61-71): a float is a constant width, a 2-tuple (mu, sigma) gives abs(mu + sigma z), anything else (1.0, 0.1)."""

    def __init__(self, h5_path, min_freq: Optional[float] = None, max_freq: Optional[float] = None, grid_size: int = 50_000,
                 linewidth=None, device="cuda", seed: int = 0):
        super().__init__()
        self.h5_path = h5_path
        self.min_freq = min_freq
        self.max_freq = max_freq
        self.grid_size = int(grid_size)
        self.linewidth = linewidth
        self.device = torch.device(device)
        self.seed = int(seed)
        self._philox_offset = 0
        self._perm, self._cursor = None, 0
        self._err_flag = None
        self._frequency_grid = None
        self._grid_dev = None
        self.load()

    # ---- the reference's properties
    @property
    def linewidth(self):
        return self._linewidth

    @linewidth.setter
    def linewidth(self, value) -> None:
        if isinstance(value, tuple):
            assert len(value) == 2, "Expected two-tuple for linewidth specification."
        self._linewidth = value

    @property
    def h5_path(self) -> Path:
        return self._h5_path

    @h5_path.setter
    def h5_path(self, value) -> None:
        if isinstance(value, str):
            value = Path(value)
        assert value.exists(), f"Target HDF5 not found; passed {value}."
        self._h5_path = value

    def __len__(self) -> int:
        return self._n

    @property
    def frequency_grid(self) -> np.ndarray:
        """spectroscopy.py:99-109: a falsy bound means the default."""
        if self._frequency_grid is None:
            min_freq = self.min_freq
            if not min_freq:
                min_freq = 1000
            max_freq = self.max_freq
            if not max_freq:
                max_freq = 32000
            self._frequency_grid = np.linspace(min_freq, max_freq, self.grid_size, dtype=np.float32)
        return self._frequency_grid

    def width_rule(self) -> tuple:
        """(mu, sigma) of batch()'s widths abs(mu + sigma z), by the reference's ``linewidth`` property: a float is constant
        (sigma 0), a tuple is (mu, sigma), anything else (1.0, 0.1)."""
        lw = self._linewidth
        if isinstance(lw, float):
            return float(lw), 0.0
        if isinstance(lw, tuple):
            mu, sigma = lw
            return float(mu), float(sigma)
        return 1.0, 0.1

    # ---- loading
    def load(self) -> None:
        path = str(self.h5_path)
        groups = h5io.datasets(path)
        self._n = len(groups)
        transitions, members = [], []
        for i in range(self._n):
            data = {key: np.array(h5io.read(path, f"{i}/{key}")).astype(np.float32) for key in h5io.datasets(path, str(i))}
            transitions.append(data.pop("transitions"))
            members.append(data)
        centers, intensity, offsets, max_int = pack_lines(transitions)
        self.members = members                                   # per item: {name: float32 array}, in name order
        self.max_int = torch.from_numpy(max_int)                 # float32 [N] on the host
        self.centers = torch.from_numpy(centers).to(self.device)
        self.intensity = torch.from_numpy(intensity).to(self.device)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self._max_int_dev = self.max_int.to(self.device)
        # members every item has with one shape are stacked on the device for batch()
        self._stacked = {}
        if members:
            for key, first in members[0].items():
                if all(key in m and m[key].shape == first.shape for m in members):
                    self._stacked[key] = torch.from_numpy(np.stack([m[key] for m in members])).to(self.device)

    def metadata(self, i: int) -> dict:
        """Item i without its spectrum, on the host: the other members in name order, then ``max_int`` [1]."""
        i = self._row(i)
        out = {k: torch.from_numpy(v) for k, v in self.members[i].items()}
        out["max_int"] = self.max_int[i:i + 1].clone()
        return out

    # ---- items
    def _require_gpu(self) -> None:
        if self.device.type != "cuda":
            raise hip.RhoHipError("SpectroscopyDataset computes its spectra on the GPU (rho_line_profile); there is no CPU path")

    def _row(self, idx) -> int:
        n = len(self)
        i = int(idx)
        if not -n <= i < n:
            raise IndexError(f"index {idx} is out of bounds for dimension 0 with size {n}")
        return i % n

    def _grid(self) -> torch.Tensor:
        if self._grid_dev is None:
            self._grid_dev = torch.from_numpy(self.frequency_grid).to(self.device)
        return self._grid_dev

    def __getitem__(self, idx) -> dict:
        self._require_gpu()
        i = self._row(idx)
        width = np.abs(random.gauss(1.0, 0.1))                   # spectroscopy.py:118
        spectrum = ops.line_profile(self._grid(), self.centers, self.intensity, self.offsets,
                                    torch.tensor([i], dtype=torch.int64, device=self.device),
                                    torch.tensor([width], dtype=torch.float32, device=self.device))
        data = {k: torch.from_numpy(v).to(self.device) for k, v in self.members[i].items()}
        data["spectrum"] = spectrum                              # [1, grid_size]: the channel axis of :134
        data["max_int"] = self._max_int_dev[i:i + 1]
        return data

    def draw_widths(self, n: int) -> torch.Tensor:
        """float32 [n] on the device by ``width_rule``; the normals come from the Philox stream (seed, running offset)."""
        mu, sigma = self.width_rule()
        if sigma == 0.0:
            return torch.full((n,), abs(mu), dtype=torch.float32, device=self.device)
        z = ops.philox_normal(torch.empty(n, dtype=torch.float32, device=self.device), self.seed, self._philox_offset)
        self._philox_offset += (n + 3) // 4
        return (mu + sigma * z).abs_()

    def batch(self, batch, widths=None) -> dict:
        """Dict of [B, ...] tensors on the device: the members every item has with one shape, ``"spectrum"`` [B, 1, grid_size],
        ``"max_int"`` [B, 1], then ``"width"`` [B], the widths used.  ``batch`` = B (rows of a device-side permutation) or an index tensor / sequence of rows in [0, len);
        ``widths``: float32 [B], drawn by ``draw_widths`` when None."""
        self._require_gpu()
        if isinstance(batch, (int, np.integer)):
            idx, poll = self._draw(int(batch)), False
        else:
            idx, poll = torch.as_tensor(batch).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous(), True
        B = idx.numel()
        if widths is None:
            widths = self.draw_widths(B)
        else:
            widths = torch.as_tensor(widths).to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        if not poll and self._err_flag is None:
            self._err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        spectrum = ops.line_profile(self._grid(), self.centers, self.intensity, self.offsets, idx, widths,
                                    err_flag=None if poll else self._err_flag)        # raises on a bad index before the gathers
        data = {k: v[idx] for k, v in self._stacked.items()}
        data["spectrum"] = spectrum.unsqueeze(1)
        data["max_int"] = self._max_int_dev[idx].unsqueeze(1)
        data["width"] = widths
        return data

    def check_errors(self) -> None:
        """Host poll of the error flag of the ``batch(B)`` launches (one synchronisation: call it outside the hot loop)."""
        if self._err_flag is not None:
            ops.line_profile_check(self._err_flag)

    def _draw(self, batch_size: int) -> torch.Tensor:
        n = len(self)
        if not 0 < batch_size <= n:
            raise ValueError(f"batch size {batch_size} must lie in [1, {n}]")
        if self._perm is None or self._cursor + batch_size > n:
            self._perm = torch.randperm(n, device=self.device)
            self._cursor = 0
        idx = self._perm[self._cursor:self._cursor + batch_size]
        self._cursor += batch_size
        return idx

    @staticmethod
    def simulate_lineprofile(frequency_grid, centers, intensities, width, device="cuda") -> torch.Tensor:
        """spectroscopy.py:142-189 on the device: the unnormalised float32 profile [grid] of one set of lines (linear
        intensities), through the kernel of the items.  Arrays or tensors; ``width``: a scalar, or one width per line.  Lines
        outside [grid.min(), grid.max()] are masked, their widths with them.  The grid must be monotone."""
        as_np = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float32)   # noqa: E731
        grid, c, inten = as_np(frequency_grid).reshape(-1), as_np(centers).reshape(-1), as_np(intensities).reshape(-1)
        if c.shape != inten.shape:
            raise ValueError(f"centers {c.shape} and intensities {inten.shape} differ in length")
        step = np.diff(grid)
        if grid.size == 0 or not (np.all(step >= 0) or np.all(step <= 0)):
            raise ValueError("simulate_lineprofile: the frequency grid must be non-empty and monotone")
        w = as_np(width).reshape(-1)
        if w.size not in (1, c.size):
            raise ValueError(f"width must be a scalar or one value per line, got {w.size} for {c.size} lines")
        order = np.argsort(c, kind="stable")
        dev = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                                                 # noqa: E731
        per_line = w.size == c.size and w.size != 1
        out = ops.line_profile(up(grid), up(c[order]), up(inten[order]), up(np.array([0, c.size], dtype=np.int64)),
                               torch.zeros(1, dtype=torch.int64, device=dev),
                               up(np.array([np.abs(w).max() if w.size else 1.0], dtype=np.float32)),
                               line_width=up(w[order]) if per_line else None, normalise=False)
        return out[0]
