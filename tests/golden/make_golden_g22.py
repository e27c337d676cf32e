"""Generate tests/golden/g22_image_datasets.npz: the items of the reference's MNISTDataset and CIFAR10Dataset
(rho_diffusion/data/wrappers.py:37-116) under their default transforms, for small synthetic fixtures.

Run in the build container only:  ``python tests/golden/make_golden_g22.py``.  torchvision is not installed there, so the reference's
classes (subclasses of torchvision.datasets.MNIST / CIFAR10) cannot be imported.  What they do per item is restated through the two
libraries that carry the arithmetic: torchvision's ``Resize`` on a PIL.Image is ``Image.resize(size[::-1], BILINEAR)`` - Pillow's own
fixed-point resample - and ``ToTensor`` on a PIL.Image is ``torch.from_numpy(array).permute(2, 0, 1).float().div(255)``; the Lambda is
``t * 2 - 1``.  So: ``Image.fromarray`` (mode "L" / "RGB", as MNIST.__getitem__ / CIFAR10.__getitem__ build it) -> ``resize`` (MNIST only)
-> from_numpy / permute / float / div(255) -> * 2 - 1, with Pillow and torch doing the work.  Inputs and float32 outputs are recorded.

The fixtures: 8 MNIST-like 28 x 28 rows and 4 CIFAR-like 32 x 32 x 3 rows, each with a label; row 0 is all 0, row 1 all 255, row 2 a
0 / 255 checkerboard, the others the top byte of an integer hash (no RNG).

Also defined here, and imported by the tests as ``make_golden_g20.center_crop`` is: ``pil_taps`` / ``pil_resize_u8``, Pillow's
ImagingResample for 8-bit images restated in pure numpy integers (no Pillow needed: this is what runs next to the GPU), ``lut``, and
the fixture writers ``write_idx`` / ``write_mnist`` / ``write_cifar_batches`` in torchvision's on-disk layout."""
from __future__ import annotations

import gzip
import math
import os
import pickle
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

MNIST_SIZE = (32, 32)                 # Resize((32, 32)), wrappers.py:112
PRECISION_BITS = 32 - 8 - 2           # Pillow, src/libImaging/Resample.c
CIFAR_NAMES = ["airplane", "automobile", "bird", "cat", "deer", "dog", "frog", "horse", "ship", "truck"]


def _hashed(shape, salt: int) -> np.ndarray:
    a = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape) + salt * 1000003
    return (((a * 2654435761) % (1 << 32)) >> 24).astype(np.uint8)


def _rows(n: int, shape, salt: int) -> np.ndarray:
    out = np.stack([_hashed(shape, salt + i) for i in range(n)])
    out[0] = 0
    out[1] = 255
    yy, xx = np.indices(shape[:2])
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    out[2] = board if len(shape) == 2 else board[..., None]
    return out


def mnist_fixture():
    """(uint8 [8, 28, 28], int64 [8])."""
    return _rows(8, (28, 28), 1), np.array([5, 0, 4, 1, 9, 2, 1, 3], dtype=np.int64)


def cifar_fixture():
    """(uint8 [4, 32, 32, 3], int64 [4])."""
    return _rows(4, (32, 32, 3), 11), np.array([6, 9, 9, 4], dtype=np.int64)


# ----------------------------------------------------------------------------- Pillow's resample in numpy integers
def pil_taps(in_size: int, out_size: int):
    """precompute_coeffs + normalize_coeffs_8bpc of Resample.c for the bilinear filter over a whole axis, in Python floats (C
    doubles): (start int32 [out], count int32 [out], coef int32 [out, ksize])."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    start = np.zeros(out_size, dtype=np.int32)
    count = np.zeros(out_size, dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        start[xx], count[xx] = xmin, xmax
        for x, v in enumerate(w):
            coef[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))
    return start, count, coef


def _pass(img: np.ndarray, axis: int, taps) -> np.ndarray:
    """One pass of ImagingResample over ``axis`` of uint8 [h, w, c]: clip8((2^21 + sum px * coef) >> 22), int64 accumulators."""
    start, count, coef = (np.asarray(t) for t in taps)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((len(start),) + src.shape[1:], dtype=np.uint8)
    for o in range(len(start)):
        s, n = int(start[o]), int(count[o])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef[o, :n].astype(np.int64), src[s:s + n], axes=(0, 0))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def pil_resize_u8(img: np.ndarray, size, taps=pil_taps) -> np.ndarray:
    """``PIL.Image.fromarray(img).resize((size[1], size[0]), BILINEAR)`` for uint8 [h, w] or [h, w, c] and size = (out_h, out_w), in
    numpy integers: the horizontal pass first, then the vertical one, each rounded to uint8; a pass whose size does not change is
    skipped.  ``taps(in_size, out_size)`` supplies the tables (default: ``pil_taps``; the tests also pass the library's)."""
    a = img[..., None] if img.ndim == 2 else img
    oh, ow = int(size[0]), int(size[1])
    if a.shape[1] != ow:
        a = _pass(a, 1, taps(a.shape[1], ow))
    if a.shape[0] != oh:
        a = _pass(a, 0, taps(a.shape[0], oh))
    a = np.ascontiguousarray(a)
    return a[..., 0] if img.ndim == 2 else a


def lut() -> np.ndarray:
    """float32 [256]: ToTensor + (t * 2) - 1 per uint8 value, in float32 steps (/ 255 rounded, * 2 exact, - 1 rounded)."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    return v * np.float32(2) - np.float32(1)


def restate(raw: np.ndarray, size=None) -> np.ndarray:
    """Items float32 [n, c, oh, ow] of uint8 rows [n, h, w] / [n, h, w, c] without Pillow or torch: pil_resize_u8 + lut, HWC -> CHW."""
    table = lut()
    out = []
    for img in raw:
        u = img if size is None else pil_resize_u8(img, size)
        u = u[..., None] if u.ndim == 2 else u
        out.append(table[u].transpose(2, 0, 1))
    return np.ascontiguousarray(np.stack(out))


# ----------------------------------------------------------------------------- fixture files in torchvision's layout
def write_idx(path, array: np.ndarray, compress: bool = False) -> None:
    """An IDX file of a uint8 array: bytes 0, 0, 0x08, ndim, big-endian uint32 dims, the payload (gzip-compressed on request)."""
    array = np.ascontiguousarray(array, dtype=np.uint8)
    blob = bytes([0, 0, 0x08, array.ndim]) + struct.pack(f">{array.ndim}I", *array.shape) + array.tobytes()
    opener = gzip.open if compress else open
    with opener(path, "wb") as f:
        f.write(blob)


def write_mnist(root, train, test, compress: bool = False) -> None:
    """root/MNIST/raw/{train,t10k}-{images-idx3,labels-idx1}-ubyte[.gz] from (images [n, 28, 28], labels [n]) pairs."""
    d = os.path.join(str(root), "MNIST", "raw")
    os.makedirs(d, exist_ok=True)
    ext = ".gz" if compress else ""
    for stem, (images, labels) in (("train", train), ("t10k", test)):
        write_idx(os.path.join(d, f"{stem}-images-idx3-ubyte{ext}"), images, compress)
        write_idx(os.path.join(d, f"{stem}-labels-idx1-ubyte{ext}"), np.asarray(labels, dtype=np.uint8), compress)


def write_cifar_batches(root, train, test, names=CIFAR_NAMES) -> None:
    """root/cifar-10-batches-py/{data_batch_1..5, test_batch, batches.meta} from (images [n, 32, 32, 3], labels [n]) pairs: pickled
    dicts with ``data`` uint8 [n, 3072] (channel planes, as the real files) and ``labels``; the train rows are dealt over the five
    files in order."""
    d = os.path.join(str(root), "cifar-10-batches-py")
    os.makedirs(d, exist_ok=True)

    def dump(name, images, labels):
        images = np.asarray(images, dtype=np.uint8).reshape(-1, 32, 32, 3)
        data = np.ascontiguousarray(images.transpose(0, 3, 1, 2)).reshape(-1, 3072)
        with open(os.path.join(d, name), "wb") as f:
            pickle.dump({"batch_label": name, "labels": [int(l) for l in labels], "data": data,
                         "filenames": [f"{name}_{i}.png" for i in range(len(data))]}, f, protocol=2)

    images, labels = train
    parts = np.array_split(np.arange(len(images)), 5)
    for k, rows in enumerate(parts):
        dump(f"data_batch_{k + 1}", np.asarray(images)[rows], np.asarray(labels)[rows])
    dump("test_batch", *test)
    with open(os.path.join(d, "batches.meta"), "wb") as f:
        pickle.dump({"label_names": list(names), "num_cases_per_batch": 10000, "num_vis": 3072}, f, protocol=2)


def main():
    import torch
    from PIL import Image

    def item(array, mode, size):
        img = Image.fromarray(array, mode=mode)                                     # MNIST.__getitem__ / CIFAR10.__getitem__
        if size is not None:
            img = img.resize(tuple(size)[::-1], Image.BILINEAR)                     # t.Resize(size) on a PIL.Image
        a = np.array(img, copy=True)
        a = a[:, :, None] if a.ndim == 2 else a
        t = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().float().div(255)      # t.ToTensor()
        return ((t * 2) - 1).numpy()                                                # t.Lambda(lambda t: (t * 2) - 1)

    g = {}
    raw, labels = mnist_fixture()
    g["mnist/raw"], g["mnist/labels"] = raw, labels
    g["mnist/out"] = np.stack([item(r, "L", MNIST_SIZE) for r in raw])
    raw, labels = cifar_fixture()
    g["cifar/raw"], g["cifar/labels"] = raw, labels
    g["cifar/out"] = np.stack([item(r, "RGB", None) for r in raw])
    for k in ("mnist", "cifar"):
        assert g[f"{k}/out"].dtype == np.float32
        size = MNIST_SIZE if k == "mnist" else None
        assert np.array_equal(g[f"{k}/out"], restate(g[f"{k}/raw"], size)), k
    np.savez_compressed(os.path.join(HERE, "g22_image_datasets.npz"), **g)
    print({k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
