"""Generate tests/golden/g20_deep_galaxy.npz from the REAL reference: DeepGalaxyDataset (rho_diffusion/data/deep_galaxy.py:38-317) and
DiscreteParameterSpace (rho_diffusion/data/parameter_space.py:9-92).

Run in the build container only:  ``python tests/golden/make_golden_g20.py``.  The reference modules are imported in place through
``make_golden.load_reference`` (the stand-in-module recipe of make_golden_g18.py) with two more stand-ins: ``h5py.File`` is a dict over
the arrays of ``build_fixture`` (the same arrays the tests write into an HDF5 file with ``h5io``), and torchvision's ``Compose`` /
``CenterCrop`` / ``Resize`` / ``Lambda`` are restated in torch - CenterCrop by torchvision's rule (offset int(round((h - ch) / 2)),
zero padding of ((cw - w) // 2, (ch - h) // 2, (cw - w + 1) // 2, (ch - h + 1) // 2) when the crop is larger), Resize through
F.interpolate(mode="bilinear", align_corners=False) with an explicit antialias.

What this pins: the reference's data handling - group selection (re.match over the file's names), camera selection (list / int),
the inclusive t_lim filter, images / np.max(images) per camera dataset in numpy's dtype promotion (uint8 and float32 cameras),
swapaxes(1, 3), the float32 label packing (s, m, t, c), loaded_parameter_space, num_classes, len - and the items of the default
transform at a few indices for both antialias settings.  What it does not pin: torchvision's own arithmetic, which is restated here
through F.interpolate.  The raw images are an integer hash of (camera, row, y, x): no RNG, rebuilt by the tests.  Only inputs'
parameters and outputs are written; nothing here runs on the GPU box."""
from __future__ import annotations

import ast
import contextlib
import importlib
import io
import numbers
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))

H, W = 263, 301      # raw [n, H, W, 1]: after the swap the image is 301 x 263, crop margins 45 / 7 are odd (round half to even)
# (group, camera, stored dtype, t_myr per row); "t_1.0_m_1.0" does not match "s_*"
CAMERAS = [
    ("s_0.5_m_1.0", 0, "uint8", [390.0, 400.0, 455.0, 520.0, 525.0]),
    ("s_0.5_m_1.0", 1, "float32", [400.0, 410.0, 415.0, 600.0]),
    ("s_1.25_m_0.25", 0, "float32", [405.0, 410.0, 600.0, 500.0]),
    ("s_1.25_m_0.25", 1, "uint8", [300.0, 450.0, 455.0]),
    ("t_1.0_m_1.0", 0, "uint8", [400.0, 405.0]),
]
# dataset kwargs per case: "example" is examples/config_deep_galaxy.json's dataset.kwargs (path aside)
CONFIGS = {
    "example": dict(use_emb_as_labels=False, dset_name_pattern="s_*", camera_pos=[0], t_lim=[400, 520]),
    "cams": dict(dset_name_pattern="s_", camera_pos=[1, 0]),
    "intcam": dict(dset_name_pattern="s_1", camera_pos=1, t_lim=[520, 300]),
}
ITEMS = {"example": [1, 4], "intcam": [1]}          # rows whose default-transform items are recorded (both antialias settings)


def pixels(k: int, n: int, dtype: str) -> np.ndarray:
    """Camera k's raw rows [n, H, W, 1]: the top byte of a multiplicative hash of the element index."""
    a = np.arange(n * H * W, dtype=np.int64).reshape(n, H, W, 1) + k * 1000003
    u = ((a * 2654435761) % (1 << 32)) >> 24
    if dtype == "uint8":
        return u.astype(np.uint8)
    return u.astype(np.float32) * np.float32(0.0371) + np.float32(0.25)


def build_fixture() -> dict:
    """{"<group>/images_camera_NN": [n, H, W, 1], "<group>/t_myr_camera_NN": float64 [n]}."""
    out = {}
    for k, (g, cam, dt, t) in enumerate(CAMERAS):
        out[f"{g}/images_camera_{cam:02d}"] = pixels(k, len(t), dt)
        out[f"{g}/t_myr_camera_{cam:02d}"] = np.asarray(t, dtype=np.float64)
    return out


def center_crop(img: torch.Tensor, size) -> torch.Tensor:
    """torchvision.transforms.functional.center_crop on a tensor [..., h, w]."""
    ch, cw = size
    h, w = img.shape[-2:]
    if cw > w or ch > h:
        pad = [(cw - w) // 2 if cw > w else 0, (ch - h) // 2 if ch > h else 0,
               (cw - w + 1) // 2 if cw > w else 0, (ch - h + 1) // 2 if ch > h else 0]
        img = F.pad(img, (pad[0], pad[2], pad[1], pad[3]), value=0.0)
        h, w = img.shape[-2:]
        if (h, w) == (ch, cw):
            return img
    top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
    return img[..., top:top + ch, left:left + cw]


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class Lambda:
    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x):
        return self.fn(x)


class CenterCrop:
    def __init__(self, size):
        self.size = (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(size)

    def __call__(self, img):
        return center_crop(img, self.size)


class Resize:
    antialias = True          # the setting of the current run (torchvision >= 0.17 defaults to True)

    def __init__(self, size, antialias=None):
        self.size = list(size)

    def __call__(self, img):
        return F.interpolate(img[None], size=self.size, mode="bilinear", align_corners=False, antialias=Resize.antialias)[0]


def main():
    sys.path.insert(0, HERE)
    from make_golden import load_reference
    load_reference()
    arrays = build_fixture()

    class File:
        """h5py.File over the fixture arrays: keys() in name order, f[path][()]."""

        def __init__(self, fn, mode="r"):
            pass

        def keys(self):
            return sorted({k.split("/")[0] for k in arrays})

        def __getitem__(self, path):
            return arrays[path.lstrip("/")]

    sys.modules["h5py"].File = File
    sys.modules["torchvision.transforms"].__dict__.update(Compose=Compose, CenterCrop=CenterCrop, Resize=Resize, Lambda=Lambda)
    DG = importlib.import_module("rho_diffusion.data.deep_galaxy")
    PS = importlib.import_module("rho_diffusion.data.parameter_space")
    torch.set_num_threads(1)
    g = {}
    for name, kw in CONFIGS.items():
        for aa in (True, False):
            Resize.antialias = aa
            log = io.StringIO()
            with contextlib.redirect_stdout(log):
                ds = DG.DeepGalaxyDataset("fixture.h5", **kw)
            if aa:
                line = [l for l in log.getvalue().splitlines() if l.startswith("Selected datasets: ")][0]
                g[f"{name}/groups"] = np.array(ast.literal_eval(line[len("Selected datasets: "):]))
                g[f"{name}/labels"] = ds.labels.numpy()
                g[f"{name}/num_classes"] = np.int64(ds.num_classes)
                g[f"{name}/len"] = np.int64(len(ds))
                for k in ("s", "m", "t", "c"):
                    g[f"{name}/lps/{k}"] = np.asarray(ds.loaded_parameter_space[k], dtype=np.float64)
                g[f"{name}/lps/keys"] = np.array(list(ds.loaded_parameter_space.keys()))
            for i in ITEMS.get(name, []):
                image, label = ds[i]
                g[f"{name}/aa{int(aa)}/item{i}"] = image.numpy()
                g[f"{name}/aa{int(aa)}/label{i}"] = label.numpy()
    # DiscreteParameterSpace (parameter_space.py:68-92)
    space = DG.DeepGalaxyDataset.parameter_space
    g["ps/keys"] = np.array(list(space.keys()))
    g["ps/len"] = np.int64(len(space))
    g["ps/size"] = np.int64(space.size())
    g["ps/t"] = np.asarray(space["t"], dtype=np.float64)
    ps = PS.DiscreteParameterSpace(param_dict={"a": [1, 2], "b": None})
    ps.push_parameter("b", 5)
    g["ps/push_none"] = np.asarray(ps["b"], dtype=np.float64)
    try:
        ps.push_parameter("a", 3)
        g["ps/push_existing_error"] = np.array("")
    except Exception as exc:                                     # noqa: BLE001 - the reference's own failure is what is pinned
        g["ps/push_existing_error"] = np.array(type(exc).__name__)
    ps["c"] = [0.5]
    g["ps/items_after_set"] = np.array([f"{k}={v}" for k, v in ps.items()])
    np.savez_compressed(os.path.join(HERE, "g20_deep_galaxy.npz"), **g)
    print({k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
