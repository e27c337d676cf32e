"""-m gpu: rho_u8_image_batch / MNISTDataset / CIFAR10Dataset on the device against Pillow's resample restated in numpy integers
(make_golden_g22.pil_resize_u8, pinned against PIL.Image.resize in test_image_datasets_host.py) plus the ToTensor / 2 t - 1 table, and
against the items recorded in tests/golden/g22_image_datasets.npz; one MNIST training step end to end.

Every image comparison is torch.equal: the arithmetic is integer plus a table lookup, so there is no tolerance.

Batch sizes follow the kernel's mapping: one item per workgroup and turn, a grid capped at 2048 workgroups.  B = 1 is one workgroup;
the unsorted list has repeats; B = 2048 + 257 makes 257 workgroups take a second item (and 1791 only one)."""
import os

import numpy as np
import pytest
import torch

from gpu_util import DEV
from make_golden_g22 import MNIST_SIZE, cifar_fixture, lut, mnist_fixture, pil_resize_u8, write_cifar_batches, write_mnist

pytestmark = pytest.mark.gpu

GRID_CAP = 2048
CASES = {   # name: (H, W, C, size or None)
    "mnist_default": (28, 28, 1, (32, 32)),
    "cifar_identity": (32, 32, 3, None),
    "down2_k5": (28, 28, 1, (14, 14)),
    "odd_rgb": (31, 29, 3, (17, 40)),
    "up_tiny": (5, 7, 1, (32, 32)),
    "down_wide": (64, 64, 1, (7, 9)),
}
N = 3


def rows(h, w, c, salt):
    a = np.arange(N * h * w * c, dtype=np.int64).reshape(N, h, w, c) + salt * 7919
    return (((a * 2654435761) % (1 << 32)) >> 24).astype(np.uint8)


def cpu_items(raw, size):
    """float32 [n, C, oh, ow] of uint8 rows [n, H, W, C]: Pillow's resample in numpy integers, the table, HWC -> CHW."""
    table = lut()
    return torch.from_numpy(np.stack([table[r if size is None else pil_resize_u8(r, size)].transpose(2, 0, 1) for r in raw]))


@pytest.fixture(scope="module")
def references():
    """Per case: (raw rows, the three restated items), computed once."""
    out = {}
    for k, (name, (h, w, c, size)) in enumerate(CASES.items()):
        raw = rows(h, w, c, salt=k + 1)
        out[name] = (raw, cpu_items(raw, size))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_u8_image_batch_equals_pillow_restated(case, references):
    from rho_diffusion_amd.engine import ops
    h, w, c, size = CASES[case]
    raw, ref = references[case]
    oh, ow = (h, w) if size is None else size
    raw_d = torch.from_numpy(raw).to(DEV)
    taps = ops.u8_image_taps(h, w, (oh, ow), DEV)
    big = (torch.arange(GRID_CAP + 257) * 7 + 2) % N
    for idx in (torch.tensor([2, 0, 0, 1, 2, 1, 1]), torch.tensor([1]), big):
        got = ops.u8_image_batch(raw_d, idx.to(DEV), size, taps=taps)
        assert got.shape == (len(idx), c, oh, ow) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), ref[idx]), (case, len(idx))


def test_saturated_rows_are_exactly_plus_and_minus_one():
    from rho_diffusion_amd.engine import ops
    for h, w, c, size in CASES.values():
        raw = torch.zeros(2, h, w, c, dtype=torch.uint8)
        raw[1] = 255
        got = ops.u8_image_batch(raw.to(DEV), torch.tensor([0, 1, 1], device=DEV), size).cpu()
        assert torch.all(got[0] == -1.0) and torch.all(got[1:] == 1.0)


def test_bad_index_is_flagged_and_valid_items_are_written(references):
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    raw, ref = references["mnist_default"]
    raw_d = torch.from_numpy(raw).to(DEV)
    for bad in ([0, N], [-1]):
        with pytest.raises(RhoHipError, match="outside"):
            ops.u8_image_batch(raw_d, torch.tensor(bad, device=DEV), MNIST_SIZE)
    # through a caller's flag: the launch does not raise, the bad item stays as it was, the others are written
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((4, 1, 32, 32), 7.0, device=DEV)
    ops.u8_image_batch(raw_d, torch.tensor([2, N, -5, 0], device=DEV), MNIST_SIZE, out=out, err_flag=flag)
    assert int(flag.item()) == 4
    assert torch.equal(out[0].cpu(), ref[2]) and torch.equal(out[3].cpu(), ref[0])
    assert torch.all(out[1:3] == 7.0)
    with pytest.raises(RhoHipError, match="outside"):
        ops.u8_image_check(flag)
    assert int(flag.item()) == 0
    got = ops.u8_image_batch(raw_d, torch.tensor([1, 2], device=DEV), MNIST_SIZE)          # the next launch is clean
    assert torch.equal(got.cpu(), ref[[1, 2]])


def test_shapes_beyond_the_lds_budget_and_mismatched_tables_are_refused():
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    raw = torch.zeros(1, 256, 256, 1, dtype=torch.uint8, device=DEV)                      # 64 KiB item + tables > 64 KiB
    with pytest.raises(RhoHipError, match="RHO_E_SHAPE"):
        ops.u8_image_batch(raw, torch.tensor([0], device=DEV), (32, 32))
    small = torch.zeros(1, 28, 28, 1, dtype=torch.uint8, device=DEV)
    with pytest.raises(RhoHipError, match="taps were built"):
        ops.u8_image_batch(small, torch.tensor([0], device=DEV), (32, 32), taps=ops.u8_image_taps(28, 28, (14, 14), DEV))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    root = tmp_path_factory.mktemp("g22")
    raw, labels = mnist_fixture()
    write_mnist(root, (raw, labels), (raw[:2], labels[:2]))
    raw, labels = cifar_fixture()
    write_cifar_batches(root, (raw, labels), (raw[:2], labels[:2]))
    return str(root)


@pytest.mark.parametrize("name", ["mnist", "cifar"])
def test_datasets_equal_the_golden(name, golden_dir, roots):
    from rho_diffusion_amd.data import CIFAR10Dataset, MNISTDataset
    g = np.load(os.path.join(golden_dir, "g22_image_datasets.npz"))
    ref, labels = torch.from_numpy(g[f"{name}/out"]), g[f"{name}/labels"]
    ds = (MNISTDataset if name == "mnist" else CIFAR10Dataset)(roots)
    n = len(ds)
    assert n == len(ref) and ds.raw.device.type == "cuda" and ds.raw.dtype == torch.uint8
    for i in range(n):
        image, label = ds[i]
        assert image.device.type == "cuda" and image.dtype == torch.float32
        assert torch.equal(image.cpu(), ref[i]) and type(label) is int and label == int(labels[i])
    assert torch.equal(ds[-1][0].cpu(), ref[n - 1])
    idx = [n - 1, 0, 2, 2, 1]
    images, lab = ds.batch(idx)
    assert images.device.type == "cuda" and lab.device.type == "cuda" and lab.dtype == torch.int64
    assert torch.equal(images.cpu(), ref[idx]) and lab.tolist() == labels[idx].tolist()
    images, lab = ds.batch(torch.tensor(idx, device=DEV))
    assert torch.equal(images.cpu(), ref[idx]) and lab.tolist() == labels[idx].tolist()
    # a bad index
    with pytest.raises(IndexError):
        ds[n]
    with pytest.raises(IndexError):
        ds.batch([0, n])
    # batch(B): N // B calls visit every row exactly once (the fixture's rows are pairwise different)
    B = 2
    seen = []
    for _ in range(n // B):
        images, lab = ds.batch(B)
        assert images.shape == (B,) + tuple(ref.shape[1:])
        for img, l in zip(images.cpu(), lab.tolist()):
            (i,) = [i for i in range(n) if torch.equal(img, ref[i])]
            assert int(labels[i]) == l
            seen.append(i)
    ds.check_errors()
    assert sorted(seen) == list(range(n))
    # the flag path of batch(B): a bad row is reported by check_errors(), not by the launch, and the valid rows are written
    images = ds._transform(torch.tensor([1, n, 0], device=DEV), poll=False)
    assert torch.equal(images[0].cpu(), ref[1]) and torch.equal(images[2].cpu(), ref[0])
    with pytest.raises(IndexError):
        ds.check_errors()
    ds.check_errors()                                       # the flag was cleared


def test_user_transform_runs_per_item_on_a_pil_image(roots):
    pytest.importorskip("PIL")
    from PIL import Image
    from rho_diffusion_amd.data import CIFAR10Dataset, MNISTDataset
    modes = []

    def tf(img):
        assert isinstance(img, Image.Image)
        modes.append(img.mode)
        return torch.from_numpy(np.array(img, copy=True)).float()

    ds = MNISTDataset(roots, transform=tf, target_transform=lambda l: l + 100)
    image, label = ds[3]
    assert image.device.type == "cuda" and torch.equal(image.cpu(), torch.from_numpy(mnist_fixture()[0][3]).float())
    assert label == int(mnist_fixture()[1][3]) + 100
    images, labels = ds.batch([3, 0])
    assert images.shape == (2, 28, 28) and torch.equal(images[0], image) and labels.tolist() == [label, int(mnist_fixture()[1][0]) + 100]
    ds = CIFAR10Dataset(roots, transform=tf)
    assert torch.equal(ds[1][0].cpu(), torch.from_numpy(cifar_fixture()[0][1]).float())
    assert set(modes) == {"L", "RGB"}


def test_mnist_training_step_fed_by_the_dataset(roots):
    """UNetv2 2-D on 32 x 32 MNIST items with MultiEmbeddings over the dataset's parameter space: the step fed by ds.batch(idx) has
    exactly the loss of the step fed by the CPU-restated batch (same t and noise; the inputs are bit-equal); three optimizer steps
    stay finite."""
    from torch import nn
    from rho_diffusion_amd.data import MNISTDataset
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    from rho_diffusion_amd.optim import HipAdamW
    ds = MNISTDataset(roots)
    torch.manual_seed(777)
    kw = dict(dims=2, in_channels=1, out_channels=1, model_channels=32, num_res_blocks=2, data_shape=[32, 32],
              attention_resolutions=[16, 8], use_scale_shift_norm=True, num_heads=4, num_classes=10, activation="SiLU",
              use_new_attention_order=False)
    ddpm = DDPM(UNet, kw, LinearSchedule(500), nn.MSELoss, timesteps=500, cond_fn="MultiEmbeddings",
                cond_fn_kwargs={"parameter_space": ds.parameter_space, "embedding_dim": 128})
    with torch.no_grad():
        for p in ddpm.backbone.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02)
    ddpm = ddpm.to(DEV)
    B = 8
    idx = torch.tensor([5, 0, 3, 3, 1, 4, 2, 7])
    gen = torch.Generator().manual_seed(3)
    t = torch.randint(0, 500, (B,), generator=gen)
    eps = torch.randn(B, 1, 32, 32, generator=gen).to(DEV)
    ddpm.random_timesteps = lambda n: t
    ddpm.noise = lambda data: eps
    x_dev, y = ds.batch(idx.to(DEV))
    x_cpu = cpu_items(mnist_fixture()[0][idx.numpy()][..., None], MNIST_SIZE).to(DEV)
    assert torch.equal(x_dev, x_cpu)
    assert y.tolist() == mnist_fixture()[1][idx.numpy()].tolist()
    loss_dev = float(ddpm.training_step([x_dev, y]))        # the forward pass has no atomics: equal inputs give equal losses
    loss_cpu = float(ddpm.training_step([x_cpu, y]))
    assert np.isfinite(loss_dev) and loss_dev == loss_cpu, (loss_dev, loss_cpu)
    opt = HipAdamW(ddpm.parameters(), lr=1e-4)
    for _ in range(3):
        x, y = ds.batch(idx.to(DEV))
        opt.zero_grad()
        loss = ddpm.training_step([x, y])
        loss.backward()
        opt.step()
        assert np.isfinite(float(loss))
    ds.check_errors()
