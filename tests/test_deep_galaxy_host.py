"""CPU: DeepGalaxyDataset's host side against the real reference (tests/golden/g20_deep_galaxy.npz, tests/golden/make_golden_g20.py):
registry entry, the example config's kwargs on a fixture written into HDF5 groups, labels / loaded_parameter_space / num_classes / len
/ group order; DiscreteParameterSpace; nested h5io paths; the crop-resize taps against torch's F.interpolate; the new C-ABI symbols."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rho_diffusion_amd import h5io
from make_golden_g20 import CONFIGS, build_fixture, center_crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_h5 = pytest.mark.skipif(not h5io.available(), reason="libhdf5 not found on this machine")


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_deep_galaxy.npz"))


@pytest.fixture(scope="module")
def fixture_h5(tmp_path_factory):
    p = tmp_path_factory.mktemp("dg") / "deep_galaxy.h5"
    h5io.write(p, build_fixture())
    return str(p)


def _check_against_golden(ds, g, name):
    assert ds.selected_datasets == list(g[f"{name}/groups"])
    assert torch.equal(ds.labels, torch.from_numpy(g[f"{name}/labels"]))
    assert ds.labels.dtype == torch.float32
    assert len(ds) == int(g[f"{name}/len"]) and ds.num_classes == int(g[f"{name}/num_classes"])
    assert list(ds.loaded_parameter_space.keys()) == list(g[f"{name}/lps/keys"])
    for k in ("s", "m", "t", "c"):
        assert [float(v) for v in ds.loaded_parameter_space[k]] == list(g[f"{name}/lps/{k}"]), k


@needs_h5
def test_example_config_constructs_the_registered_dataset(g20, fixture_h5):
    """examples/config_deep_galaxy.json's dataset section through the registry, on a file with the DeepGalaxy group layout."""
    from rho_diffusion_amd import registry
    from rho_diffusion_amd.data import DeepGalaxyDataset
    cls = registry.get("datasets", "DeepGalaxyDataset")
    assert cls is DeepGalaxyDataset
    cfg = {"name": "DeepGalaxyDataset", "kwargs": {"path": "../../datasets/DeepGalaxy/output_bw_512.h5", "use_emb_as_labels": False,
                                                   "dset_name_pattern": "s_*", "camera_pos": [0], "t_lim": [400, 520]}}
    kwargs = dict(json.loads(json.dumps(cfg))["kwargs"], path=fixture_h5)
    assert {k: v for k, v in kwargs.items() if k != "path"} == CONFIGS["example"]
    ds = registry.get("datasets", cfg["name"])(**kwargs, device="cpu")
    _check_against_golden(ds, g20, "example")
    assert ds.raw.dtype == torch.float32 and tuple(ds.raw.shape) == (6, 263, 301, 1)      # a uint8 and a float32 camera
    assert ds.dset_name_pattern == ("s_*",) and ds.attributes == ["s", "m", "t", "c"]


@needs_h5
@pytest.mark.parametrize("name", ["cams", "intcam"])
def test_selection_cameras_and_t_lim_follow_the_reference(g20, fixture_h5, name):
    from rho_diffusion_amd.data import DeepGalaxyDataset
    ds = DeepGalaxyDataset(fixture_h5, device="cpu", **CONFIGS[name])
    _check_against_golden(ds, g20, name)
    if name == "intcam":
        assert ds.raw.dtype == torch.uint8                  # a uint8-only selection stays uint8 on the device
        assert torch.equal(ds.rowmax, torch.full((3,), float(build_fixture()["s_1.25_m_0.25/images_camera_01"].max()),
                                                 dtype=torch.float64))


@needs_h5
def test_cpu_device_has_no_item_path(fixture_h5):
    from rho_diffusion_amd.data import DeepGalaxyDataset
    from rho_diffusion_amd.hip import RhoHipError
    ds = DeepGalaxyDataset(fixture_h5, device="cpu")
    with pytest.raises(RhoHipError):
        ds[0]
    with pytest.raises(RhoHipError):
        ds.batch(2)
    with pytest.raises(ValueError):
        DeepGalaxyDataset(fixture_h5, device="cpu", dset_name_pattern="nothing")


def test_parameter_space_follows_the_reference(g20):
    """parameter_space.py:19-92: dict access, len, items, size; push_parameter on a None key gives [] as in the reference.  On a key
    that holds values the reference raises (isinstance with one argument, g20 records the error); here that branch appends."""
    from rho_diffusion_amd.data import DeepGalaxyDataset, DiscreteParameterSpace
    from rho_diffusion_amd.models import MultiEmbeddings
    space = DeepGalaxyDataset.parameter_space
    assert isinstance(space, DiscreteParameterSpace)
    assert list(space.keys()) == list(g20["ps/keys"]) and len(space) == int(g20["ps/len"])
    assert space.size() == int(g20["ps/size"]) and list(space["t"]) == list(g20["ps/t"])
    ps = DiscreteParameterSpace(param_dict={"a": [1, 2], "b": None})
    ps.push_parameter("b", 5)
    assert ps["b"] == list(g20["ps/push_none"]) == []
    assert str(g20["ps/push_existing_error"]) == "TypeError"
    ps.push_parameter("a", 3)
    ps.push_parameter("a", [2, 4])
    assert ps["a"] == [1, 2, 3, 4]
    ps.push_parameter("b", 5)
    ps["c"] = [0.5]
    assert [f"{k}={v}" for k, v in ps.items()] == ["a=[1, 2, 3, 4]", "b=[5]", "c=[0.5]"]
    assert repr(ps) == repr(ps.param_dict) and list(ps.parameters) == ["a", "b", "c"] and len(list(ps.values())) == 3
    torch.manual_seed(0)
    draw = space.sample(5)
    assert draw.shape == (5, 4) and all(float(draw[i, 2]) in space["t"] for i in range(5))
    with pytest.raises(NotImplementedError):
        from rho_diffusion_amd.data import AbstractParameterSpace
        AbstractParameterSpace().size()
    # MultiEmbeddings(parameter_space=..., embedding_dim=128) as scripts/training.py:119 builds it
    me = MultiEmbeddings(parameter_space=space, embedding_dim=128)
    assert {k: m.num_embeddings for k, m in me.embedding_layers.items()} == {"s": 6, "m": 6, "t": 71, "c": 14}


def test_reference_module_path_resolves_under_the_alias():
    import sys
    import rho_diffusion_amd
    saved = {k: v for k, v in sys.modules.items() if k == "rho_diffusion" or k.startswith("rho_diffusion.")}
    try:
        rho_diffusion_amd.install_alias()
        from rho_diffusion.data.parameter_space import DiscreteParameterSpace
        from rho_diffusion.data.deep_galaxy import DeepGalaxyDataset
        assert DiscreteParameterSpace is rho_diffusion_amd.data.DiscreteParameterSpace
        assert DeepGalaxyDataset is rho_diffusion_amd.data.DeepGalaxyDataset
    finally:
        for k in [k for k in sys.modules if k == "rho_diffusion" or k.startswith("rho_diffusion.")]:
            del sys.modules[k]
        sys.modules.update(saved)


@needs_h5
def test_h5io_nested_groups(tmp_path):
    p = tmp_path / "g.h5"
    a, t = np.arange(24, dtype=np.uint8).reshape(2, 3, 4, 1), np.array([1.5, 2.5])
    h5io.write(p, {"s_1_m_1/images_camera_00": a, "s_1_m_1/t_myr_camera_00": t, "deep/er/x": np.ones(3, np.float32), "flat": t})
    assert h5io.datasets(p) == ["deep", "flat", "s_1_m_1"]
    assert h5io.datasets(p, group="s_1_m_1") == ["images_camera_00", "t_myr_camera_00"]
    assert h5io.datasets(p, group="deep/er") == ["x"]
    assert np.array_equal(h5io.read(p, "/s_1_m_1/images_camera_00"), a) and h5io.read(p, "s_1_m_1/images_camera_00").dtype == np.uint8
    assert np.array_equal(h5io.read(p, "s_1_m_1/images_camera_00", 1), a[1])
    assert h5io.shape(p, "deep/er/x") == (3,) and np.array_equal(h5io.read(p, "s_1_m_1/t_myr_camera_00"), t)
    for missing in ("s_1_m_1/images_camera_01", "s_2_m_1/images_camera_00", "/nope/x/y"):
        with pytest.raises(KeyError):
            h5io.read(p, missing)
        with pytest.raises(KeyError):
            h5io.shape(p, missing)
    with pytest.raises(KeyError):
        h5io.datasets(p, group="nope")


GEOMETRIES = [(512, 256, 128), (301, 256, 128), (263, 256, 128), (263, 180, 100), (70, 101, 48), (90, 96, 64), (40, 32, 128),
              (50, 40, 96), (300, 299, 37), (64, 64, 64), (37, 53, 211)]


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=[f"{a}-{b}-{c}" for a, b, c in GEOMETRIES])
def test_crop_resize_taps_equal_torch_interpolate(geom, antialias):
    """rho_crop_resize_taps (host) = the weights torch's F.interpolate applies after torchvision's center crop, bit for bit: crops
    with odd margins, larger crops (padding), down- and upscales, identity."""
    from rho_diffusion_amd.engine import ops
    n, crop, out = geom
    start, weight = ops.crop_resize_axis_taps(n, crop, out, antialias)
    k = weight.shape[1]
    assert start.min() >= 0 and int(start.max()) + k <= n and bool((start[1:] >= start[:-1]).all())
    dense = torch.zeros(n, out)
    for o in range(out):
        dense[int(start[o]):int(start[o]) + k, o] += weight[o]
    eye = torch.eye(n)[:, None, None, :]
    ref = F.interpolate(center_crop(eye, (1, crop)), size=(1, out), mode="bilinear", align_corners=False, antialias=antialias)
    assert torch.equal(dense, ref[:, 0, 0, :])


def test_crop_resize_symbols_in_header_and_binding():
    from rho_diffusion_amd import hip
    header = open(os.path.join(ROOT, "include", "rho_hip.h")).read()
    for name in ("rho_crop_resize", "rho_crop_resize_taps"):
        assert re.search(rf"\b{name}\s*\(", header) and name in hip.SIGNATURES
    assert int(re.search(r"#define\s+RHO_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == hip.ABI_VERSION
    from rho_diffusion_amd.engine import ops
    with pytest.raises(hip.RhoHipError):
        ops.crop_resize_axis_taps(0, 256, 128, True)
