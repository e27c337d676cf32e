"""-m gpu: rho_crop_resize / DeepGalaxyDataset on the device against the CPU restatement of the reference's item path (rows / np.max
in numpy's promotion, float32, swapaxes(1, 3), torchvision's CenterCrop rule, F.interpolate, 2 t - 1) and against the reference's
items recorded in tests/golden/g20_deep_galaxy.npz; the example config's geometry end to end through training steps.

Tolerance: 2e-6 abs on the [-1, 1] output (the tap weights equal torch's bit for bit, test_deep_galaxy_host.py; only the summation
order differs); the identity geometry is bit-equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV
from make_golden_g20 import CONFIGS, ITEMS, build_fixture, center_crop

pytestmark = pytest.mark.gpu

CASES = {   # name: (N, H, W, C, crop (rows = the W axis, cols = the H axis), size)
    "default_512": (6, 512, 512, 1, (256, 256), (128, 128)),
    "nonsquare_odd": (5, 263, 301, 3, (200, 181), (72, 100)),
    "pad": (4, 90, 70, 1, (101, 96), (64, 48)),
    "pad_one_axis": (3, 90, 70, 3, (60, 100), (45, 50)),
    "upscale": (3, 40, 50, 1, (32, 40), (128, 96)),
}


def hashed(n, h, w, c, dtype, salt):
    a = np.arange(n * h * w * c, dtype=np.int64).reshape(n, h, w, c) + salt * 7919
    u = ((a * 2654435761) % (1 << 32)) >> 24
    return u.astype(np.uint8) if dtype == np.uint8 else (u.astype(np.float32) * np.float32(0.013) + np.float32(0.5)).astype(dtype)


def cpu_items(raw, rowmax, idx, crop, size, antialias):
    """The reference's per-item path on the CPU for rows ``idx`` of raw [N, H, W, C]."""
    out = []
    for i in idx:
        x = raw[i]
        v = x / np.float32(rowmax[i]) if x.dtype == np.float32 else (x / np.float64(rowmax[i])).astype(np.float32)
        t = torch.from_numpy(np.ascontiguousarray(v.astype(np.float32).transpose(2, 1, 0)))
        t = F.interpolate(center_crop(t, crop)[None], size=list(size), mode="bilinear", align_corners=False, antialias=antialias)[0]
        out.append(t * 2 - 1)
    return torch.stack(out)


def _dev(raw, rowmax):
    return torch.from_numpy(raw).to(DEV), torch.from_numpy(np.asarray(rowmax, dtype=np.float64)).to(DEV)


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_crop_resize_matches_cpu_interpolate(case, dtype, antialias):
    from rho_diffusion_amd.engine import ops
    N, H, W, C, crop, size = CASES[case]
    raw = hashed(N, H, W, C, dtype, salt=len(case))
    rowmax = [float(raw.max()) + (i % 3) for i in range(N)]           # a different maximum per row (camera datasets)
    idx = [N - 1, 1, 1, 0, N - 1, 2]                                  # repeated and unsorted
    raw_d, max_d = _dev(raw, rowmax)
    got = ops.crop_resize(raw_d, max_d, torch.tensor(idx, device=DEV), crop, size, antialias)
    torch.cuda.synchronize()
    ref = cpu_items(raw, rowmax, idx, crop, size, antialias)
    assert got.shape == ref.shape == (len(idx), C) + tuple(size)
    err = float((got.cpu() - ref).abs().max())
    assert err <= 2e-6, f"{case} {dtype.__name__} antialias={antialias}: max abs error {err:.3e}"


def test_crop_resize_float64_rows():
    from rho_diffusion_amd.engine import ops
    raw = hashed(3, 80, 90, 1, np.float64, salt=5)
    rowmax = [float(raw.max())] * 3
    raw_d, max_d = _dev(raw, rowmax)
    for aa in (True, False):
        got = ops.crop_resize(raw_d, max_d, torch.tensor([2, 0], device=DEV), (64, 70), (48, 40), aa)
        assert float((got.cpu() - cpu_items(raw, rowmax, [2, 0], (64, 70), (48, 40), aa)).abs().max()) <= 2e-6


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_identity_geometry_is_numpys_normalisation_bit_for_bit(dtype):
    """crop = size = image: the output is 2 v - 1 with v = (images / np.max(images)).astype(float32), bit-equal."""
    from rho_diffusion_amd.engine import ops
    N, H, W, C = 4, 37, 45, 3
    raw = hashed(N, H, W, C, dtype, salt=11)
    raw_d, max_d = _dev(raw, [float(raw.max())] * N)
    v = (raw / raw.max()).astype(np.float32)                          # numpy: uint8 / uint8 in float64, float32 / float32 in float32
    ref = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 2, 1))) * 2 - 1
    for aa in (True, False):
        got = ops.crop_resize(raw_d, max_d, torch.arange(N, device=DEV), (W, H), (W, H), aa)
        assert torch.equal(got.cpu(), ref)


def test_out_of_range_index_raises_and_the_next_launch_succeeds():
    from rho_diffusion_amd.engine import ops
    from rho_diffusion_amd.hip import RhoHipError
    raw = hashed(3, 64, 64, 1, np.uint8, salt=2)
    rowmax = [float(raw.max())] * 3
    raw_d, max_d = _dev(raw, rowmax)
    for bad in ([0, 3], [-1]):
        with pytest.raises(RhoHipError, match="outside"):
            ops.crop_resize(raw_d, max_d, torch.tensor(bad, device=DEV), 48, 32)
    got = ops.crop_resize(raw_d, max_d, torch.tensor([2, 0], device=DEV), 48, 32)
    assert float((got.cpu() - cpu_items(raw, rowmax, [2, 0], (48, 48), (32, 32), True)).abs().max()) <= 2e-6


@pytest.fixture(scope="module")
def fixture_h5(tmp_path_factory):
    from rho_diffusion_amd import h5io
    p = tmp_path_factory.mktemp("dgg") / "deep_galaxy.h5"
    h5io.write(p, build_fixture())
    return str(p)


def test_dataset_items_and_batches_equal_the_reference(golden_dir, fixture_h5):
    import os
    from rho_diffusion_amd.data import DeepGalaxyDataset
    from rho_diffusion_amd.hip import RhoHipError
    g = np.load(os.path.join(golden_dir, "g20_deep_galaxy.npz"))
    for name, rows in ITEMS.items():
        for aa in (True, False):
            ds = DeepGalaxyDataset(fixture_h5, antialias=aa, **CONFIGS[name])
            images, labels = ds.batch(torch.tensor(rows))
            for j, i in enumerate(rows):
                ref = torch.from_numpy(g[f"{name}/aa{int(aa)}/item{i}"])
                image, label = ds[i]
                assert image.device.type == "cuda" and image.shape == ref.shape == (1, 128, 128)
                assert float((image.cpu() - ref).abs().max()) <= 2e-6, (name, aa, i)
                assert float((images[j].cpu() - ref).abs().max()) <= 2e-6, (name, aa, i)
                assert torch.equal(label, torch.from_numpy(g[f"{name}/aa{int(aa)}/label{i}"]))
                assert torch.equal(labels[j].cpu(), label)
    ds = DeepGalaxyDataset(fixture_h5, **CONFIGS["example"])
    with pytest.raises(IndexError):
        ds[len(ds)]
    with pytest.raises(RhoHipError):
        ds.batch(torch.tensor([0, len(ds)]))
    # batch(B): rows of a device-side permutation, an epoch without repeats
    a, la = ds.batch(4)
    b, lb = ds.batch(2)
    ds.check_errors()
    seen = torch.cat([la, lb]).cpu()
    assert a.shape == (4, 1, 128, 128) and b.shape == (2, 1, 128, 128)
    assert sorted(map(tuple, seen.tolist())) == sorted(map(tuple, ds.labels.tolist()))
    # a user transform / target_transform runs per item on the normalised, swapped [C, W, H] row (the slow path)
    ds2 = DeepGalaxyDataset(fixture_h5, transform=lambda t: t[:, :8, :5], target_transform=lambda l: l[2], **CONFIGS["example"])
    raw, mx = ds2.raw.cpu().numpy(), ds2.rowmax.cpu().numpy()
    img, lab = ds2[4]
    v = raw[4] / np.float32(mx[4])
    assert torch.equal(img.cpu(), torch.from_numpy(np.ascontiguousarray(v.transpose(2, 1, 0)))[:, :8, :5])
    assert float(lab) == float(ds2.labels[4, 2])
    imgs, labs = ds2.batch([4, 0])
    assert imgs.shape == (2, 1, 8, 5) and torch.equal(imgs[0].cpu(), img.cpu()) and labs.shape == (2,)


def test_training_step_fed_by_the_dataset(fixture_h5):
    """examples/config_deep_galaxy.json's model (UNetv2 2-D 128^2, mc 32, num_classes 25, MultiEmbeddings(parameter_space,
    embedding_dim=128)): one training step fed by ds.batch(idx) has the loss of the same step fed by the CPU-restated batch (same t
    and noise); three optimizer steps stay finite."""
    from torch import nn
    from rho_diffusion_amd.data import DeepGalaxyDataset
    from rho_diffusion_amd.diffusion import DDPM, LinearSchedule
    from rho_diffusion_amd.models import UNet
    from rho_diffusion_amd.optim import HipAdamW
    ds = DeepGalaxyDataset(fixture_h5, **CONFIGS["example"])
    torch.manual_seed(777)
    kw = dict(dims=2, in_channels=1, out_channels=1, model_channels=32, num_res_blocks=2, data_shape=[128, 128],
              attention_resolutions=[16, 8], use_scale_shift_norm=True, num_heads=4, num_classes=25, activation="SiLU",
              use_new_attention_order=False)
    ddpm = DDPM(UNet, kw, LinearSchedule(500), nn.MSELoss, timesteps=500, cond_fn="MultiEmbeddings",
                cond_fn_kwargs={"parameter_space": ds.parameter_space, "embedding_dim": 128})
    with torch.no_grad():
        for p in ddpm.backbone.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0.0, 0.02)
    ddpm = ddpm.to(DEV)
    B = 8
    idx = torch.tensor([5, 0, 3, 3, 1, 4, 2, 0])
    gen = torch.Generator().manual_seed(3)
    t = torch.randint(0, 500, (B,), generator=gen)
    eps = torch.randn(B, 1, 128, 128, generator=gen).to(DEV)
    ddpm.random_timesteps = lambda n: t
    ddpm.noise = lambda data: eps
    x_dev, y = ds.batch(idx.to(DEV))
    x_cpu = cpu_items(ds.raw.cpu().numpy(), ds.rowmax.cpu().numpy(), idx.tolist(), (256, 256), (128, 128), True).to(DEV)
    assert float((x_dev - x_cpu).abs().max()) <= 2e-6
    loss_dev = float(ddpm.training_step([x_dev, y]))
    loss_cpu = float(ddpm.training_step([x_cpu, y]))
    assert abs(loss_dev - loss_cpu) <= 1e-5 * abs(loss_cpu), (loss_dev, loss_cpu)
    opt = HipAdamW(ddpm.parameters(), lr=1e-4)
    for _ in range(3):
        x, y = ds.batch(idx.to(DEV))
        opt.zero_grad()
        loss = ddpm.training_step([x, y])
        loss.backward()
        opt.step()
        assert np.isfinite(float(loss))
    ds.check_errors()
