"""The reference's MNISTDataset and CIFAR10Dataset (rho_diffusion/data/wrappers.py:37-116) with their default transforms on the device.

The reference subclasses torchvision's MNIST / CIFAR10: the files are decoded once, and every item is built on the host as a
PIL.Image and run through Resize((32, 32)) (MNIST only) -> ToTensor() -> 2 t - 1 in the DataLoader's workers.  Here the files are
read directly (torchvision is not needed), the uint8 rows [N, H, W, C] stay resident on the GPU, and ``rho_u8_image_batch`` turns a
batch of row indices into the float32 [B, C, oh, ow] training input in one launch.  Resize on a PIL.Image is Pillow's fixed-point
bilinear resample and ToTensor / 2 t - 1 is a table over the 256 byte values, so the device items equal the host path's bit for bit
(tests/golden/make_golden_g22.py).  ``batch(B)`` is what a training loop should call.  A user ``transform`` is honoured per item on
a PIL.Image, as torchvision does - the slow host path, which needs Pillow.

Files are torchvision's on-disk layout, read from ``root`` as they are:
  MNIST     root/MNIST/raw/{train,t10k}-images-idx3-ubyte and -labels-idx1-ubyte (a .gz of the same name is accepted)
  CIFAR-10  root/cifar-10-batches-py/data_batch_1..5 (train) or test_batch (test), and batches.meta
No md5 check is made, and nothing is ever downloaded: ``download`` is accepted for signature compatibility only and missing files
raise FileNotFoundError.  This module opens no network connection."""
from __future__ import annotations

import gzip
import os
import pickle
import struct

import numpy as np
import torch

from .. import hip
from ..engine import ops
from ..registry import registry
from .parameter_space import DiscreteParameterSpace

__all__ = ["CIFAR10Dataset", "MNISTDataset"]


def read_idx(path: str) -> np.ndarray:
    """The uint8 array of an IDX file (``path`` or ``path``.gz): bytes 0, 0, 0x08, ndim, big-endian uint32 dims, the payload."""
    if os.path.exists(path):
        with open(path, "rb") as f:
            blob = f.read()
    else:
        try:
            with gzip.open(path + ".gz", "rb") as f:
                blob = f.read()
        except (EOFError, gzip.BadGzipFile) as exc:
            raise ValueError(f"{path}.gz: truncated or malformed gzip file ({exc})") from exc
    if len(blob) < 4 or blob[0] != 0 or blob[1] != 0 or blob[2] != 0x08 or blob[3] == 0:
        raise ValueError(f"{path}: not a uint8 IDX file (magic {blob[:4].hex()})")
    ndim = blob[3]
    if len(blob) < 4 + 4 * ndim:
        raise ValueError(f"{path}: truncated IDX header")
    dims = struct.unpack(f">{ndim}I", blob[4:4 + 4 * ndim])
    size = int(np.prod(dims, dtype=np.int64))
    if len(blob) - 4 - 4 * ndim != size:
        raise ValueError(f"{path}: header says {dims} = {size} bytes, the file holds {len(blob) - 4 - 4 * ndim}")
    return np.frombuffer(blob, dtype=np.uint8, offset=4 + 4 * ndim).reshape(dims).copy()


class _U8ImageDataset(torch.utils.data.Dataset):
    """What the two datasets share: uint8 rows resident on the device, integer labels, and the one-launch default transform."""

    classes: list = []
    _gz_ok = False

    def __init__(self, root: str, transform, target_transform, train: bool, download: bool, device, image_size):
        self.root = os.path.expanduser(root) if isinstance(root, str) else str(root)
        self.transform = transform
        self.target_transform = target_transform
        self.train = bool(train)
        self.download = download            # never acted on: this build does not download
        self.device = torch.device(device)
        self.image_size = None if image_size is None else ops._pair(image_size)
        self.parameter_space = DiscreteParameterSpace(param_dict={"labels": [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]})
        self.loaded_parameter_space = None
        self.attributes = None
        self._taps = self._lut = None
        self._perm, self._cursor = None, 0
        self._err_flag = None
        missing = [p for p in self._files() if not (os.path.exists(p) or (self._gz_ok and os.path.exists(p + ".gz")))]
        if missing:
            raise FileNotFoundError(
                f"{type(self).__name__}: {', '.join(missing)} not found.  This build never downloads (download={download!r} is "
                "accepted for compatibility only): place the files of torchvision's layout under root.")
        images, labels = self._load()
        if images.shape[0] != labels.shape[0]:
            raise ValueError(f"{type(self).__name__}: {images.shape[0]} images but {labels.shape[0]} labels under {self.root}")
        self._host = images                                                          # uint8 [N, H, W, C]
        self._labels = labels.astype(np.int64)
        self.raw = torch.from_numpy(images).to(self.device)
        self._labels_dev = torch.from_numpy(self._labels).to(self.device)
        self.class_to_idx = {name: i for i, name in enumerate(self.classes)}

    def _files(self) -> list:
        raise NotImplementedError

    def _load(self):
        raise NotImplementedError

    def _pil(self, i: int):
        raise NotImplementedError

    def __len__(self) -> int:
        return int(self._host.shape[0])

    def _require_gpu(self) -> None:
        if self.device.type != "cuda":
            raise hip.RhoHipError(f"{type(self).__name__} transforms its images on the GPU (rho_u8_image_batch); there is no CPU path")

    def _user_item(self, i: int):
        try:
            import PIL.Image  # noqa: F401
        except ImportError as exc:
            raise ImportError(f"{type(self).__name__}: a user transform runs on a PIL.Image per item and needs Pillow") from exc
        image = self.transform(self._pil(i))
        return image.to(self.device) if isinstance(image, torch.Tensor) else image

    def __getitem__(self, idx):
        self._require_gpu()
        n = len(self)
        i = int(idx)
        if not -n <= i < n:
            raise IndexError(f"index {idx} is out of bounds for dimension 0 with size {n}")
        i %= n
        if self.transform is not None:
            image = self._user_item(i)
        else:
            image = self._transform(torch.tensor([i], dtype=torch.int64, device=self.device), poll=True)[0]
        label = int(self._labels[i])
        if self.target_transform is not None:
            label = self.target_transform(label)
        return image, label

    def batch(self, batch):
        """([B, C, oh, ow] float32, labels int64 [B]) on the device: ``batch`` = B (rows of a device-side permutation, a shuffled
        epoch; a new permutation when fewer than B rows are left) or an index tensor / sequence of rows in [0, len).  One transform
        launch.  ``batch(B)`` does not synchronise: poll ``check_errors()`` outside the hot loop; ``batch(index)`` raises IndexError
        on a row outside [0, len) itself."""
        self._require_gpu()
        if isinstance(batch, (int, np.integer)):
            idx, poll = self._draw(int(batch)), False
        else:
            idx, poll = torch.as_tensor(batch).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous(), True
        if self.transform is not None:
            images = torch.stack([self._user_item(i) for i in idx.tolist()])
        else:
            images = self._transform(idx, poll)            # raises on a bad index before the label gather below
        labels = self._labels_dev[idx]
        if self.target_transform is not None:
            labels = torch.as_tensor([self.target_transform(int(l)) for l in labels.tolist()], device=self.device)
        return images, labels

    def check_errors(self) -> None:
        """Host poll of the error flag of the ``batch(B)`` launches (one synchronisation: call it outside the hot loop)."""
        if self._err_flag is not None:
            self._poll(self._err_flag)

    @staticmethod
    def _poll(flag: torch.Tensor) -> None:
        try:
            ops.u8_image_check(flag)
        except hip.RhoHipError as exc:
            if "outside" in str(exc):
                raise IndexError(str(exc)) from exc
            raise

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

    def _transform(self, idx: torch.Tensor, poll: bool) -> torch.Tensor:
        _, H, W, _ = self.raw.shape
        size = (H, W) if self.image_size is None else self.image_size
        if self._taps is None:
            self._taps = ops.u8_image_taps(H, W, size, self.device)
            self._lut = ops.u8_image_lut(self.device)
        if poll:
            flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        else:
            if self._err_flag is None:
                self._err_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            flag = self._err_flag
        out = ops.u8_image_batch(self.raw, idx, size, lut=self._lut, taps=self._taps, err_flag=flag)
        if poll:
            self._poll(flag)
        return out


@registry.register_dataset("MNISTDataset")
class MNISTDataset(_U8ImageDataset):
    """wrappers.py:78-116.  The reference's constructor (root, transform, target_transform, train=True, download=True) plus ``device``
    (the images live there; a CPU device loads files and labels and raises RhoHipError on any item) and ``image_size`` (the Resize of the
    default transform, (32, 32); None: no resize).  ``data`` uint8 [N, 28, 28] and ``targets`` int64 [N] are host tensors shaped as
    torchvision's; ``raw`` is the device-resident uint8 [N, 28, 28, 1].  Items: ``ds[i]`` = (float32 [1, 32, 32] on the device, int
    label); ``batch`` as documented there."""

    classes = ["0 - zero", "1 - one", "2 - two", "3 - three", "4 - four", "5 - five", "6 - six", "7 - seven", "8 - eight", "9 - nine"]
    _gz_ok = True

    def __init__(self, root: str, transform=None, target_transform=None, train: bool = True, download: bool = True, device="cuda",
                 image_size=(32, 32)):                 # t.Resize((32, 32)), wrappers.py:112
        super().__init__(root, transform, target_transform, train, download, device, image_size)

    def _files(self) -> list:
        stem = "train" if self.train else "t10k"
        d = os.path.join(self.root, "MNIST", "raw")
        return [os.path.join(d, f"{stem}-images-idx3-ubyte"), os.path.join(d, f"{stem}-labels-idx1-ubyte")]

    def _load(self):
        image_file, label_file = self._files()
        images, labels = read_idx(image_file), read_idx(label_file)
        if images.ndim != 3:
            raise ValueError(f"{image_file}: expected [n, rows, cols] images, got {images.shape}")
        if labels.ndim != 1:
            raise ValueError(f"{label_file}: expected [n] labels, got {labels.shape}")
        self.data = torch.from_numpy(images)
        self.targets = torch.from_numpy(labels.astype(np.int64))
        return images[..., None], labels

    def _pil(self, i: int):
        from PIL import Image
        return Image.fromarray(self._host[i, :, :, 0], mode="L")


@registry.register_dataset("CIFAR10Dataset")
class CIFAR10Dataset(_U8ImageDataset):
    """wrappers.py:37-75.  The reference's constructor plus ``device`` and ``image_size`` as MNISTDataset's; the default transform has
    no Resize (``image_size`` None), so the launch is a gather, HWC -> CHW and the table.  ``data`` is a numpy uint8 [N, 32, 32, 3] and
    ``targets`` a list of ints, as torchvision's; ``classes`` come from batches.meta; ``raw`` is the device-resident uint8
    [N, 32, 32, 3].  The pickles are loaded with encoding="latin1"; no md5 check is made."""

    base_folder = "cifar-10-batches-py"

    def __init__(self, root: str, transform=None, target_transform=None, train: bool = True, download: bool = True, device="cuda",
                 image_size=None):
        super().__init__(root, transform, target_transform, train, download, device, image_size)

    def _files(self) -> list:
        names = [f"data_batch_{k}" for k in range(1, 6)] if self.train else ["test_batch"]
        return [os.path.join(self.root, self.base_folder, n) for n in names + ["batches.meta"]]

    def _load(self):
        *batches, meta = self._files()
        data, targets = [], []
        for path in batches:
            with open(path, "rb") as f:
                try:
                    entry = pickle.load(f, encoding="latin1")
                except Exception as exc:                      # noqa: BLE001 - any unpickling failure is a malformed file
                    raise ValueError(f"{path}: not a CIFAR-10 batch pickle ({type(exc).__name__}: {exc})") from exc
            if not isinstance(entry, dict) or "data" not in entry or not ("labels" in entry or "fine_labels" in entry):
                raise ValueError(f"{path}: a CIFAR-10 batch holds 'data' and 'labels'")
            rows = np.asarray(entry["data"], dtype=np.uint8)
            if rows.ndim != 2 or rows.shape[1] != 3072:
                raise ValueError(f"{path}: expected data [n, 3072], got {rows.shape}")
            labels = list(entry["labels"] if "labels" in entry else entry["fine_labels"])
            if len(labels) != rows.shape[0]:
                raise ValueError(f"{path}: {rows.shape[0]} images but {len(labels)} labels")
            data.append(rows)
            targets.extend(int(l) for l in labels)
        with open(meta, "rb") as f:
            try:
                names = pickle.load(f, encoding="latin1")["label_names"]
            except Exception as exc:                          # noqa: BLE001
                raise ValueError(f"{meta}: no 'label_names' ({type(exc).__name__}: {exc})") from exc
        self.classes = list(names)
        images = np.ascontiguousarray(np.vstack(data).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
        self.data = images
        self.targets = targets
        return images, np.asarray(targets, dtype=np.int64)

    def _pil(self, i: int):
        from PIL import Image
        return Image.fromarray(self._host[i])
