"""The reference's DeepGalaxyDataset (rho_diffusion/data/deep_galaxy.py:38-317) with its default transform on the device.

The file layout, selection and labels are the reference's: root groups ``s_<s>_m_<m>`` chosen by ``re.compile(pattern).match``
(in the file's name order), datasets ``images_camera_NN`` [n, H, W, C] and ``t_myr_camera_NN`` [n] per camera, an inclusive
``t_lim`` filter, labels float32 [N, 4] = (s, m, t, c), ``loaded_parameter_space`` (sorted unique values) and ``num_classes``
(unique t).  The HDF5 file is read through ``h5io`` (h5py is not needed).

The images differ in where they live and when they are transformed.  The reference keeps a float32 copy of the whole set on the
host, [N, C, W, H] after ``swapaxes(1, 3)``, and runs CenterCrop(256) -> Resize((128, 128)) -> 2 t - 1 per item in the DataLoader.
Here the rows stay resident on the GPU in their stored dtype (uint8 for DeepGalaxy: a quarter of the float32 copy), next to the
per-row maximum of the camera dataset they came from, and ``rho_crop_resize`` normalises, swaps, crops, resizes and rescales a
whole batch in one launch.  ``batch(B)`` is what a training loop should call.  A user ``transform`` is honoured per item on the
normalised [C, W, H] tensor, as in the reference - the slow path, in PyTorch on the device."""
from __future__ import annotations

import re
from typing import Optional

import numpy as np
import torch

from .. import h5io, hip
from ..engine import ops
from ..registry import registry
from .parameter_space import DiscreteParameterSpace

__all__ = ["DeepGalaxyDataset"]


def _storage_dtype(dtypes) -> np.dtype:
    """One resident dtype for the selected cameras whose division gives numpy's result for every row.  uint8 alone stays uint8.
    uint8 + float32 is stored as float32: an exact integer quotient correctly rounded to float32 equals numpy's float64 quotient
    rounded to float32, because double rounding through float64 (53 >= 2 * 24 + 2 bits) is exact for division.  Everything else
    (float64, other integer types) is stored as float64, where integers divide as numpy divides them and float32 rows again round
    to the float32 quotient."""
    kinds = {np.dtype(d) for d in dtypes}
    for d in kinds:
        if d.kind not in "uif" or d == np.float16:
            raise ValueError(f"DeepGalaxyDataset: unsupported image dtype {d}")
    if kinds == {np.dtype(np.uint8)}:
        return np.dtype(np.uint8)
    if kinds <= {np.dtype(np.uint8), np.dtype(np.float32)}:
        return np.dtype(np.float32)
    return np.dtype(np.float64)


@registry.register_dataset("DeepGalaxyDataset")
class DeepGalaxyDataset(torch.utils.data.Dataset):
    """deep_galaxy.py:38-317.  Constructor of the reference plus ``device`` (the images live there; a CPU device loads the labels
    and raises RhoHipError on any item) and ``antialias`` (torchvision's tensor Resize antialiases from 0.17 on; False gives the
    plain bilinear of older torchvision).  Items: ``ds[i]`` = (float32 [C, 128, 128] on the device, label float32 [4]);
    ``batch(B)`` draws B rows of a device-side permutation (a shuffled epoch, scripts/training.py:100-104; a new permutation when
    fewer than B rows are left), ``batch(index)`` takes the given rows; both return ([B, C, 128, 128], labels [B, 4]) on the
    device with one transform launch."""

    parameter_space = DiscreteParameterSpace(
        param_dict={"s": [0.25, 0.5, 0.75, 1, 1.25, 1.5],
                    "m": [0.25, 0.5, 0.75, 1, 1.25, 1.5],
                    "t": list(range(300, 655, 5)),
                    "c": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]},
        sampler=None)
    crop_size = 256                  # torchvision.transforms.CenterCrop(256), deep_galaxy.py:87
    image_size = (128, 128)          # torchvision.transforms.Resize((128, 128)), :88

    def __init__(self, path: str, use_emb_as_labels: bool = True, dset_name_pattern: str = "s_*", camera_pos: list = [0],
                 t_lim: list = None, transform=None, target_transform=None, device="cuda", antialias: bool = True):
        self.h5fn = path
        self.use_emb_labels = use_emb_as_labels
        self.labels = None
        self.num_classes = 0
        self.dset_name_pattern = (dset_name_pattern,)
        self.camera_pos = camera_pos
        self.t_lim = t_lim
        self.loaded_parameter_space = DiscreteParameterSpace(param_dict={"s": [], "m": [], "t": [], "c": []})
        self.attributes = ["s", "m", "t", "c"]
        self.transform = transform
        self.target_transform = target_transform
        self.device = torch.device(device)
        self.antialias = bool(antialias)
        self.selected_datasets = []
        self._taps = None
        self._perm, self._cursor = None, 0
        self._err_flag = None
        self.load(dset_name_pattern, camera_pos, t_lim)

    def __len__(self) -> int:
        return int(self.raw.shape[0])

    def _require_gpu(self) -> None:
        if self.device.type != "cuda":
            raise hip.RhoHipError("DeepGalaxyDataset transforms its images on the GPU (rho_crop_resize); there is no CPU path")

    def __getitem__(self, idx):
        self._require_gpu()
        n = len(self)
        i = int(idx)
        if not -n <= i < n:
            raise IndexError(f"index {idx} is out of bounds for dimension 0 with size {n}")
        i %= n
        if self.transform is not None:
            image = self.transform(self.normalised(i))
        else:
            image = self._crop_resize(torch.tensor([i], dtype=torch.int64, device=self.device), poll=True)[0]
        label = self.labels[i]
        if self.target_transform:
            label = self.target_transform(label)
        return image, label

    def batch(self, batch):
        """([B, C, 128, 128], labels [B, 4]) on the device: ``batch`` = B (rows of a device-side permutation) or an index tensor /
        sequence of rows in [0, len)."""
        self._require_gpu()
        if isinstance(batch, (int, np.integer)):
            idx, poll = self._draw(int(batch)), False
        else:
            idx, poll = torch.as_tensor(batch).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous(), True
        if self.transform is not None:
            images = torch.stack([self.transform(self.normalised(i)) for i in idx.tolist()])
        else:
            images = self._crop_resize(idx, poll)          # raises on a bad index before the label gather below
        labels = self._labels_dev[idx]
        if self.target_transform:
            labels = torch.stack([self.target_transform(l) for l in labels])
        return images, labels

    def normalised(self, i: int) -> torch.Tensor:
        """Row i as the reference's ``self.data[i]``: images / np.max(images) in numpy's promotion, float32 [C, W, H]."""
        x = self.raw[i]
        if x.dtype == torch.float32:
            v = x / self.rowmax[i].to(torch.float32)
        else:
            v = (x.to(torch.float64) / self.rowmax[i]).to(torch.float32)
        return v.permute(2, 1, 0).contiguous()

    def check_errors(self) -> None:
        """Host poll of the error flag of the ``batch(B)`` launches (one synchronisation: call it outside the hot loop)."""
        if self._err_flag is not None:
            ops.crop_resize_check(self._err_flag)

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

    def _crop_resize(self, idx: torch.Tensor, poll: bool) -> torch.Tensor:
        if self._taps is None:
            _, H, W, _ = self.raw.shape
            self._taps = ops.crop_resize_taps(H, W, self.crop_size, self.image_size, self.antialias, self.device)
        if not poll and self._err_flag is None:
            self._err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        return ops.crop_resize(self.raw, self.rowmax, idx, self.crop_size, self.image_size, self.antialias, taps=self._taps,
                               err_flag=None if poll else self._err_flag)

    def load(self, dset_name_pattern, camera_pos, t_lim):
        images, rowmax, labels = self._load_all(dset_name_pattern=dset_name_pattern, camera_pos=camera_pos, t_lim=t_lim)
        self.raw = torch.from_numpy(images).to(self.device)          # [N, H, W, C] in the stored dtype
        self.rowmax = torch.from_numpy(rowmax).to(self.device)       # float64 [N]
        self.labels = labels
        self._labels_dev = labels.to(self.device)

    def _load_all(self, dset_name_pattern="*", camera_pos="*", t_lim=None):
        """deep_galaxy.py:165-281 (+ _load_dataset :283-299 and _get_labels :301-317)."""
        full_dset_list = h5io.datasets(self.h5fn)
        r = re.compile(dset_name_pattern)
        matched_dset_list = list(filter(r.match, full_dset_list))
        self.selected_datasets = matched_dset_list
        if isinstance(camera_pos, int):
            camera_pos = [camera_pos]
        elif isinstance(camera_pos, str) and camera_pos == "*":
            camera_pos = range(0, 14)
        images_set, max_set, m_set, s_set, t_set, c_set = [], [], [], [], [], []
        for dset_name in matched_dset_list:
            for cpos in camera_pos:
                images = h5io.read(self.h5fn, "/%s/images_camera_%02d" % (dset_name, cpos))
                if images.ndim != 4:
                    raise ValueError(f"/{dset_name}/images_camera_{cpos:02d}: expected [n, H, W, C] images, got {images.shape}")
                mx = np.max(images) if images.size else 0
                s = float(dset_name.split("_")[1])
                m = float(dset_name.split("_")[3])
                labels_t = h5io.read(self.h5fn, "%s/t_myr_camera_%02d" % (dset_name, cpos))
                labels_s = np.array([s] * labels_t.shape[0])
                labels_m = np.array([m] * labels_t.shape[0])
                labels_c = np.ones(labels_m.shape, dtype=np.int32) * cpos
                if t_lim is not None:
                    t_low, t_high = np.min(t_lim), np.max(t_lim)
                    flags = np.logical_and(labels_t >= t_low, labels_t <= t_high)
                    images, labels_t, labels_m, labels_s, labels_c = (images[flags], labels_t[flags], labels_m[flags],
                                                                      labels_s[flags], labels_c[flags])
                images_set.append(images)
                max_set.append(np.full(images.shape[0], mx, dtype=np.float64))
                m_set.append(labels_m)
                s_set.append(labels_s)
                t_set.append(labels_t)
                c_set.append(labels_c)
        if not images_set or sum(a.shape[0] for a in images_set) == 0:
            raise ValueError(f"DeepGalaxyDataset: no image of {self.h5fn} matches pattern {dset_name_pattern!r}, cameras "
                             f"{list(camera_pos)}, t_lim {t_lim}")
        storage = _storage_dtype([a.dtype for a in images_set])
        images = np.concatenate([a.astype(storage, copy=False) for a in images_set], axis=0)
        rowmax = np.concatenate(max_set)
        labels_m_set, labels_s_set = np.concatenate(m_set), np.concatenate(s_set)
        labels_t_set, labels_cpos_set = np.concatenate(t_set), np.concatenate(c_set)

        lps = self.loaded_parameter_space
        lps["m"] = np.unique(labels_m_set)
        lps["s"] = np.unique(labels_s_set)
        lps["t"] = np.unique(labels_t_set)
        lps["c"] = np.unique(labels_cpos_set)
        num_classes = np.unique(labels_t_set).shape[0]
        for key in ("m", "s", "t", "c"):
            lps[key] = sorted(lps[key])
        loaded_parameters = {"m": labels_m_set, "s": labels_s_set, "t": labels_t_set, "c": labels_cpos_set}
        labels_tensor = torch.zeros((len(labels_m_set), len(self.attributes)), dtype=torch.float)
        for i, attr in enumerate(self.attributes):
            labels_tensor[:, i] = torch.tensor(loaded_parameters[attr], dtype=torch.float)
        self.num_classes = num_classes
        return images, rowmax, labels_tensor
