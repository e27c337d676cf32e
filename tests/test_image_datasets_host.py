"""CPU: the host side of MNISTDataset / CIFAR10Dataset - Pillow's integer tap tables (rho_pil_resize_taps) against PIL.Image.resize,
the ToTensor / 2 t - 1 table, the g22 golden against the pure-numpy restatement, the file readers on fixture files, the registry and
the constructor surface.  Nothing here launches a kernel."""
import gzip
import os
import pickle

import numpy as np
import pytest
import torch

from make_golden_g22 import (CIFAR_NAMES, MNIST_SIZE, cifar_fixture, lut, mnist_fixture, pil_resize_u8, pil_taps, restate,
                             write_cifar_batches, write_idx, write_mnist)

# (h, w) -> (out_h, out_w)
GEOMETRIES = [((28, 28), (32, 32)), ((32, 32), (32, 32)), ((28, 28), (64, 64)), ((28, 28), (14, 14)), ((31, 29), (17, 40)),
              ((5, 7), (32, 32)), ((64, 64), (7, 9)), ((28, 20), (32, 48)), ((28, 28), (32, 28)), ((28, 28), (28, 32)),
              ((100, 3), (33, 3)), ((1, 1), (4, 4))]


def lib_taps(in_size, out_size):
    from rho_diffusion_amd.engine import ops
    return tuple(t.numpy() for t in ops.pil_resize_taps(in_size, out_size))


def images(h, w, c):
    """random, all-0, all-255, checkerboard and single-hot-pixel images of one shape."""
    shape = (h, w) if c == 1 else (h, w, c)
    rng = np.random.default_rng(h * 1000 + w * 10 + c)
    out = [rng.integers(0, 256, size=shape, dtype=np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)]
    board = np.zeros(shape, np.uint8)
    board[(np.indices((h, w)).sum(0) & 1) == 1] = 255
    hot = np.zeros(shape, np.uint8)
    hot[h // 2, w // 2] = 255
    return out + [board, hot]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_library_taps_reproduce_pillow_bit_for_bit(geom, c):
    pytest.importorskip("PIL")
    from PIL import Image
    (h, w), (oh, ow) = geom
    for k, img in enumerate(images(h, w, c)):
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(pil_resize_u8(img, (oh, ow), taps=lib_taps), ref), (geom, c, k)
        assert np.array_equal(pil_resize_u8(img, (oh, ow)), ref), (geom, c, k)            # the numpy tables the GPU tests use


def test_tap_tables_are_normalised_and_inside_the_axis():
    from rho_diffusion_amd import hip
    sizes = sorted({(a, b) for (h, w), (oh, ow) in GEOMETRIES for a, b in ((h, oh), (w, ow))})
    for in_size, out_size in sizes:
        start, count, coef = lib_taps(in_size, out_size)
        ksize = coef.shape[1]
        scale = max(in_size / out_size, 1.0)
        assert ksize == int(np.ceil(scale)) * 2 + 1 == hip.lib().rho_pil_resize_taps(in_size, out_size, None, None, None)
        assert np.all(start >= 0) and np.all(count >= 1) and np.all(count <= ksize) and np.all(start + count <= in_size)
        assert np.all(coef >= 0)
        assert np.all(np.abs(coef.sum(1).astype(np.int64) - (1 << 22)) <= ksize), (in_size, out_size)
        for o in range(out_size):
            assert not coef[o, count[o]:].any()
        for a, b in zip((start, count, coef), pil_taps(in_size, out_size)):
            assert np.array_equal(a, b)
    assert lib_taps(28, 14)[2].shape[1] == 5            # the antialiased support of a 2x reduction
    assert hip.lib().rho_pil_resize_taps(0, 4, None, None, None) < 0
    start = np.zeros(4, np.int32)
    assert hip.lib().rho_pil_resize_taps(4, 4, start.ctypes.data, None, None) < 0


def test_lut_is_totensor_and_the_lambda_bit_for_bit():
    from rho_diffusion_amd.engine import ops
    table = ops.u8_image_lut()
    u = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16)
    ref = u.float().div(255) * 2 - 1                        # ToTensor on a uint8 image, then (t * 2) - 1
    assert table.dtype == torch.float32 and torch.equal(table, ref.reshape(256))
    assert torch.equal(table, torch.from_numpy(lut()))
    assert float(table[0]) == -1.0 and float(table[255]) == 1.0


def test_golden_equals_the_numpy_restatement(golden_dir):
    g = np.load(os.path.join(golden_dir, "g22_image_datasets.npz"))
    for name, fixture, size in (("mnist", mnist_fixture, MNIST_SIZE), ("cifar", cifar_fixture, None)):
        raw, labels = fixture()
        assert np.array_equal(g[f"{name}/raw"], raw) and np.array_equal(g[f"{name}/labels"], labels)
        assert g[f"{name}/out"].dtype == np.float32
        assert np.array_equal(g[f"{name}/out"], restate(raw, size))
        if size is not None:                                # and through the library's tables
            assert np.array_equal(g[f"{name}/out"], np.stack([lut()[pil_resize_u8(r, size, taps=lib_taps)][None] for r in raw]))
        assert not raw[0].any() and raw[1].min() == 255 and set(np.unique(raw[2])) == {0, 255}
        assert np.all(g[f"{name}/out"][0] == -1.0) and np.all(g[f"{name}/out"][1] == 1.0)
    assert g["mnist/out"].shape == (8, 1, 32, 32) and g["cifar/out"].shape == (4, 3, 32, 32)


# ----------------------------------------------------------------------------- readers
@pytest.mark.parametrize("compress", [False, True], ids=["raw", "gz"])
def test_mnist_reader_and_split(tmp_path, compress):
    from rho_diffusion_amd.data import MNISTDataset
    raw, labels = mnist_fixture()
    write_mnist(tmp_path, (raw, labels), (raw[5:], labels[5:]), compress=compress)
    ds = MNISTDataset(str(tmp_path), device="cpu")
    assert ds.train and len(ds) == 8 and ds.root == str(tmp_path) and ds.image_size == (32, 32)
    assert isinstance(ds.data, torch.Tensor) and ds.data.dtype == torch.uint8 and ds.data.shape == (8, 28, 28)
    assert np.array_equal(ds.data.numpy(), raw)
    assert ds.targets.dtype == torch.int64 and ds.targets.tolist() == labels.tolist()
    assert ds.raw.dtype == torch.uint8 and ds.raw.shape == (8, 28, 28, 1) and np.array_equal(ds.raw[..., 0].numpy(), raw)
    assert ds.classes[3] == "3 - three" and ds.class_to_idx["7 - seven"] == 7
    test = MNISTDataset(str(tmp_path), train=False, device="cpu", image_size=None)
    assert not test.train and len(test) == 3 and np.array_equal(test.data.numpy(), raw[5:]) and test.image_size is None
    assert test.targets.tolist() == labels[5:].tolist()


def test_mnist_malformed_files_raise_value_error(tmp_path):
    from rho_diffusion_amd.data import MNISTDataset
    raw, labels = mnist_fixture()
    d = tmp_path / "MNIST" / "raw"

    def fresh():
        write_mnist(tmp_path, (raw, labels), (raw[:2], labels[:2]))

    fresh()
    blob = (d / "train-images-idx3-ubyte").read_bytes()
    (d / "train-images-idx3-ubyte").write_bytes(b"\x00\x00\x0d\x03" + blob[4:])          # float IDX, not uint8
    with pytest.raises(ValueError, match="IDX"):
        MNISTDataset(str(tmp_path), device="cpu")
    (d / "train-images-idx3-ubyte").write_bytes(b"\x89PNG" + blob[4:])
    with pytest.raises(ValueError, match="IDX"):
        MNISTDataset(str(tmp_path), device="cpu")
    (d / "train-images-idx3-ubyte").write_bytes(blob[:-100])                             # truncated payload
    with pytest.raises(ValueError, match="holds"):
        MNISTDataset(str(tmp_path), device="cpu")
    fresh()
    write_idx(d / "train-labels-idx1-ubyte", labels[:7].astype(np.uint8))                # 8 images, 7 labels
    with pytest.raises(ValueError, match="8 images but 7 labels"):
        MNISTDataset(str(tmp_path), device="cpu")
    fresh()
    write_idx(d / "train-labels-idx1-ubyte", raw)                                        # images where labels belong
    with pytest.raises(ValueError, match="labels"):
        MNISTDataset(str(tmp_path), device="cpu")
    fresh()
    os.remove(d / "train-images-idx3-ubyte")
    (d / "train-images-idx3-ubyte.gz").write_bytes(gzip.compress(blob)[:-40])            # truncated .gz
    with pytest.raises(ValueError):
        MNISTDataset(str(tmp_path), device="cpu")


def test_cifar_reader_meta_and_split(tmp_path):
    from rho_diffusion_amd.data import CIFAR10Dataset
    raw, labels = cifar_fixture()
    write_cifar_batches(tmp_path, (raw, labels), (raw[::-1][:3], labels[::-1][:3]))
    ds = CIFAR10Dataset(str(tmp_path), device="cpu")
    assert len(ds) == 4 and ds.image_size is None
    assert isinstance(ds.data, np.ndarray) and ds.data.dtype == np.uint8 and ds.data.shape == (4, 32, 32, 3)
    assert np.array_equal(ds.data, raw)
    assert isinstance(ds.targets, list) and ds.targets == labels.tolist()
    assert ds.raw.shape == (4, 32, 32, 3) and np.array_equal(ds.raw.numpy(), raw)
    assert ds.classes == CIFAR_NAMES and ds.class_to_idx["frog"] == 6
    test = CIFAR10Dataset(str(tmp_path), train=False, device="cpu")
    assert len(test) == 3 and np.array_equal(test.data, raw[::-1][:3]) and test.targets == labels[::-1][:3].tolist()
    # malformed pickles
    d = tmp_path / "cifar-10-batches-py"
    (d / "test_batch").write_bytes(b"not a pickle")
    with pytest.raises(ValueError, match="test_batch"):
        CIFAR10Dataset(str(tmp_path), train=False, device="cpu")
    with open(d / "test_batch", "wb") as f:
        pickle.dump({"data": np.zeros((2, 3072), np.uint8), "labels": [1]}, f)
    with pytest.raises(ValueError, match="2 images but 1 labels"):
        CIFAR10Dataset(str(tmp_path), train=False, device="cpu")


def test_absent_files_raise_and_nothing_is_downloaded(tmp_path):
    from rho_diffusion_amd.data import CIFAR10Dataset, MNISTDataset
    with pytest.raises(FileNotFoundError, match="never downloads") as e:
        MNISTDataset(str(tmp_path), download=True, device="cpu")
    assert os.path.join(str(tmp_path), "MNIST", "raw", "train-images-idx3-ubyte") in str(e.value)
    with pytest.raises(FileNotFoundError, match="never downloads") as e:
        CIFAR10Dataset(str(tmp_path), download=True, train=False, device="cpu")
    assert os.path.join(str(tmp_path), "cifar-10-batches-py", "test_batch") in str(e.value)
    assert os.listdir(tmp_path) == []
    # the module imports no URL / socket / subprocess machinery
    import rho_diffusion_amd.data.wrappers as W
    src = open(W.__file__).read()
    for word in ("urllib", "requests", "socket", "http", "subprocess", "os.system"):
        assert word not in src, word


def test_registry_surface_and_cpu_device(tmp_path):
    from rho_diffusion_amd.data import CIFAR10Dataset, DiscreteParameterSpace, MNISTDataset
    from rho_diffusion_amd.hip import RhoHipError
    from rho_diffusion_amd.registry import registry
    assert registry.get("datasets", "MNISTDataset") is MNISTDataset
    assert registry.get("datasets", "CIFAR10Dataset") is CIFAR10Dataset
    write_mnist(tmp_path, mnist_fixture(), mnist_fixture())
    write_cifar_batches(tmp_path, cifar_fixture(), cifar_fixture())
    for cls in (MNISTDataset, CIFAR10Dataset):
        ds = cls(str(tmp_path), device="cpu")
        assert isinstance(ds.parameter_space, DiscreteParameterSpace)
        assert list(ds.parameter_space["labels"]) == list(range(10))
        assert ds.attributes is None and ds.loaded_parameter_space is None
        with pytest.raises(RhoHipError, match="no CPU path"):
            ds[0]
        with pytest.raises(RhoHipError, match="no CPU path"):
            ds.batch(2)


def test_header_and_binding_declare_the_entry_points():
    from rho_diffusion_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rho_hip.h")).read()
    for name in ("rho_pil_resize_taps", "rho_u8_image_batch"):
        assert name in hip.SIGNATURES and f"{name}(" in header
        assert hasattr(hip.lib(), name)
    assert "wrappers.py" in header and "Resample.c" in header
