"""-m gpu: k_gemm1x1, the bf16 GEMM form of the wide 1x1x1 convolutions (csrc/gemm1x1.h), at the smallest shapes at which each of
its parts can go wrong, and the launches that must stay on k_conv.

Reference: fp32 matmul of the bf16-rounded operands on the CPU.  Bound: the project's bf16 forward-layer bound, rel-L2 < 6e-3
(fp32 fallback launches: 2e-5), as test_gpu_bench_shapes.py.  Every output is prefilled with NaN (an unwritten element fails) and
lies between two guard bands that must come back untouched (an out-of-bounds store fails without faulting).
"""
import math

import pytest
import torch

from helpers import rel_l2
from gpu_util import DEV

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 4096           # elements on either side of an output
NEW = "k_gemm1x1<bf16,256x128>"


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _guarded(shape, dtype):
    """A NaN-filled tensor of `shape` inside a larger allocation whose margins hold 1.5."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD,), 1.5, dtype=dtype, device=DEV)
    flat[GUARD:GUARD + n] = float("nan")
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _guards_intact(flat):
    return bool((flat[:GUARD] == 1.5).all()) and bool((flat[-GUARD:] == 1.5).all())


def _rand(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g) * scale
    return v.to(torch.bfloat16).float() if dtype == BF16 else v


def _case(ops, N, spatial, c1, cout, split=None, residual=False, stats=False, dtype=BF16, c2=0, prologue=False, seed=0):
    """Build one 1x1x1 launch and its CPU reference.  Returns a dict with the descriptor, the outputs and what to compare against."""
    split = cout if split is None else split
    D, H, W = spatial
    S, cin = D * H * W, c1 + c2
    x = _rand((N, S, cin), 100 + seed, dtype)
    w = _rand((cout, cin), 200 + seed, dtype, 1.0 / math.sqrt(cin))
    b = _rand((cout,), 300 + seed, F32, 0.1)
    res = _rand((N, S, split), 400 + seed, dtype) if residual else None
    pre = (1 + 0.3 * _rand((N, cin), 500 + seed, F32), 0.2 * _rand((N, cin), 600 + seed, F32)) if prologue else None
    xa = x
    if pre is not None:                  # the loader rounds the activated tile
        xa = torch.nn.functional.silu(pre[0][:, None, :] * x + pre[1][:, None, :])
        xa = xa.to(torch.bfloat16).float() if dtype == BF16 else xa
    ref = xa.reshape(-1, cin) @ w.t() + b                                   # fp32, [N * S, cout]
    ref = ref.reshape(N, S, cout)
    want_y = ref[:, :, :split] + (res if residual else 0)
    want_y2 = ref[:, :, split:].permute(0, 2, 1)                            # channel-major [N, cout - split, S]

    xd = x.to(DEV).to(dtype).reshape(N, D, H, W, cin)
    x1 = xd[..., :c1].contiguous()
    x2 = xd[..., c1:].contiguous() if c2 else None
    wp = ops.prep_conv_weight(w.reshape(cout, cin, 1, 1, 1).to(DEV), dtype)
    bp = b.to(DEV)
    yflat, y = _guarded((N, D, H, W, split), dtype) if split > 0 else (None, None)
    y2flat, y2 = _guarded((N, cout - split, S), dtype) if split < cout else (None, None)
    resd = res.to(DEV).to(dtype).reshape(N, D, H, W, split) if residual else None
    pa, pb = (pre[0].to(DEV), pre[1].to(DEV)) if pre else (None, None)
    d = ops.make_conv_desc(x1, x2, wp, bp, kernel=(1, 1, 1), cout=cout, split=split, y=y, y2=y2, res=resd, pre_a=pa, pre_b=pb,
                           pre_silu=prologue)
    sflat = sbuf = None
    tiles = 0
    if stats:
        tiles = ops.conv_stats_tiles(d)
        assert tiles == S // 256
        sflat, sbuf = _guarded((N, tiles, 2, split), F32)
        d.stats = sbuf.data_ptr()
    return dict(d=d, y=y, y2=y2, yflat=yflat, y2flat=y2flat, sbuf=sbuf, sflat=sflat, want_y=want_y, want_y2=want_y2,
                keep=(x1, x2, wp, bp, resd, pa, pb), N=N, S=S, split=split, cout=cout, tol=6e-3 if dtype == BF16 else 2e-5)


def _launch_and_check(ops, c):
    ops.conv_launch(c["d"])
    torch.cuda.synchronize()
    N, S, split, cout = c["N"], c["S"], c["split"], c["cout"]
    if c["y"] is not None:
        got = c["y"].float().cpu().reshape(N, S, split)
        assert torch.isfinite(got).all(), "unwritten or non-finite element in y"
        e = rel_l2(got, c["want_y"])
        print(f"y rel-L2 {e:.3e}")
        assert e < c["tol"], e
        assert _guards_intact(c["yflat"]), "store outside y"
    if c["y2"] is not None:
        got2 = c["y2"].float().cpu()
        assert torch.isfinite(got2).all(), "unwritten or non-finite element in y2"
        e2 = rel_l2(got2, c["want_y2"])
        print(f"y2 rel-L2 {e2:.3e}")
        assert e2 < c["tol"], e2
        assert _guards_intact(c["y2flat"]), "store outside y2"
    if c["sbuf"] is not None:
        st = c["sbuf"].cpu()
        assert torch.isfinite(st).all(), "unwritten statistics row"
        assert _guards_intact(c["sflat"]), "store outside the statistics buffer"
        yy = c["y"].float().cpu().reshape(N, S, split)                       # the values as stored
        tot = st.sum(1)                                                     # over the tiles of a sample: [N, 2, split]
        e_s, e_q = rel_l2(tot[:, 0], yy.sum(1)), rel_l2(tot[:, 1], (yy * yy).sum(1))
        print(f"stats rel-L2 sum {e_s:.3e} sumsq {e_q:.3e}")
        assert e_s < 1e-3 and e_q < 1e-3, (e_s, e_q)
        # ... and row by row: tile t of sample n covers positions [256 t, 256 t + 256)
        yt = yy.reshape(N, S // 256, 256, split)
        assert rel_l2(st[:, :, 0], yt.sum(2)) < 1e-3 and rel_l2(st[:, :, 1], (yt * yt).sum(2)) < 1e-3


# name -> keyword arguments of _case: the shapes of the issue (one tile and one K-step; eight K-steps, both epilogue orientations and
# the per-sample base of y2; an odd K-step count, an odd batch and a workgroup count that is no multiple of 8, with residual and
# statistics)
GEMM_CASES = {
    "one_tile_one_kstep": dict(N=1, spatial=(4, 8, 8), c1=64, cout=128),
    "split_both_orientations": dict(N=2, spatial=(8, 8, 8), c1=512, cout=384, split=256),
    "res_stats_odd": dict(N=3, spatial=(12, 8, 8), c1=192, cout=128, residual=True, stats=True),
    # two cout tiles in the channel-major region: the second one's rows start 128 channels into y2
    "two_y2_tiles": dict(N=2, spatial=(4, 8, 8), c1=64, cout=384, split=128),
}


@pytest.mark.parametrize("name", list(GEMM_CASES), ids=list(GEMM_CASES))
def test_gemm1x1_against_fp32_matmul(ops, name):
    c = _case(ops, seed=len(name), **GEMM_CASES[name])
    assert ops.conv_variant(c["d"]) == NEW
    _launch_and_check(ops, c)


@pytest.mark.parametrize("name", ["split_both_orientations", "res_stats_odd"])
def test_gemm1x1_same_launch_twice_is_bit_identical(ops, name):
    c = _case(ops, seed=7, **GEMM_CASES[name])
    assert ops.conv_variant(c["d"]) == NEW
    outs = [t for t in (c["y"], c["y2"], c["sbuf"]) if t is not None]
    ops.conv_launch(c["d"])
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    for t in outs:
        t.fill_(float("nan"))
    ops.conv_launch(c["d"])
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


FALLBACK_CASES = {
    "positions_105": dict(N=1, spatial=(3, 5, 7), c1=64, cout=128),
    "cin_96": dict(N=1, spatial=(4, 8, 8), c1=96, cout=128),
    "fp32": dict(N=1, spatial=(4, 8, 8), c1=64, cout=128, dtype=F32),
    "prologue": dict(N=1, spatial=(4, 8, 8), c1=64, cout=128, prologue=True),
    "second_input": dict(N=1, spatial=(4, 8, 8), c1=64, c2=64, cout=128),
    "small_grid": dict(N=1, spatial=(4, 8, 8), c1=128, cout=128),          # <= 128 workgroups and >= 4 chunks: k_conv's k-split range
}


@pytest.mark.parametrize("name", list(FALLBACK_CASES), ids=list(FALLBACK_CASES))
def test_launches_the_gemm_does_not_take_stay_on_k_conv(ops, name):
    c = _case(ops, seed=len(name), **FALLBACK_CASES[name])
    assert ops.conv_variant(c["d"]).startswith("k_conv<"), ops.conv_variant(c["d"])
    _launch_and_check(ops, c)


def test_switch_sends_everything_back_to_k_conv(ops, monkeypatch):
    c = _case(ops, seed=3, **GEMM_CASES["one_tile_one_kstep"])
    assert ops.conv_variant(c["d"]) == NEW
    monkeypatch.setenv("RHO_GEMM1X1", "0")
    assert ops.conv_variant(c["d"]).startswith("k_conv<")
    _launch_and_check(ops, c)
    monkeypatch.delenv("RHO_GEMM1X1")
    assert ops.conv_variant(c["d"]) == NEW


def test_misaligned_operand_stays_on_k_conv(ops):
    """The GEMM moves every operand in 16-byte pieces; an output that starts 8 bytes into a piece keeps k_conv's 8-byte path."""
    c = _case(ops, seed=5, **GEMM_CASES["one_tile_one_kstep"])
    assert ops.conv_variant(c["d"]) == NEW
    c["d"].y = c["y"].data_ptr() + 8
    assert ops.conv_variant(c["d"]).startswith("k_conv<")


def test_engine_plan_follows_the_switch(monkeypatch):
    """RHO_GEMM1X1 is part of the plan key: flipping it builds another plan instead of replaying the one built under the old value."""
    from helpers import UNET_CASES, case_inputs
    from rho_diffusion_amd.models import UNet
    from rho_diffusion_amd.engine.unet_engine import UNetEngine
    assert "RHO_GEMM1X1" in UNetEngine._PLAN_ENV and UNetEngine._plan_switches().gemm1x1
    kw, _, _ = UNET_CASES["tiny3d"]
    model = UNet(**dict(kw), compute_dtype="bf16").to(DEV).eval()
    _, x, t, _ = case_inputs("tiny3d")
    eng = model.engine()
    with torch.no_grad():
        a = model(x.to(DEV), t.to(DEV)).float()
        n0, sig0 = len(eng._plans), eng._plan_signature()
        monkeypatch.setenv("RHO_GEMM1X1", "0")
        assert not UNetEngine._plan_switches().gemm1x1 and eng._plan_signature() != sig0
        b = model(x.to(DEV), t.to(DEV)).float()
    assert len(eng._plans) == n0 + 1
    assert torch.isfinite(a).all() and rel_l2(b, a) < 3e-2          # (the whole-UNet bf16 bound; the same network either way)


def test_bench_geometry_runs_the_gemm(ops):
    """The headline's attention projections (c3: 512 channels at (64, 8, 8), batch 32; c5: 256 channels at (128, 16, 16)) dispatch to
    the new kernel.  Nothing is launched: the operands are one element broadcast to the shape."""
    def fake(*shape):
        return torch.zeros(1, dtype=BF16, device=DEV).expand(*shape)

    def variant(N, spatial, cin, cout, split, residual, stats=False):
        x = fake(N, *spatial, cin)
        w = fake(1, cout, cin)
        b = torch.zeros(cout, device=DEV)
        y = fake(N, *spatial, split)
        y2 = fake(N, cout - split, math.prod(spatial)) if split < cout else None
        d = ops.make_conv_desc(x, None, w, b, kernel=(1, 1, 1), cout=cout, split=split, y=y, y2=y2, res=y if residual else None)
        if stats:
            assert ops.conv_stats_tiles(d) == math.prod(spatial) // 256
            d.stats = b.data_ptr()
        return ops.conv_variant(d)

    assert variant(32, (64, 8, 8), 512, 1536, 1024, False) == NEW
    assert variant(32, (64, 8, 8), 512, 512, 512, True) == NEW
    assert variant(32, (64, 8, 8), 512, 512, 512, True, stats=True) == NEW
    assert variant(1, (64, 8, 8), 512, 1536, 1024, False) == NEW
    assert variant(1, (128, 16, 16), 256, 768, 512, False) == NEW
