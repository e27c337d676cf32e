"""-m gpu: the compile-time-geometry form of the bf16 3x3x3 k_conv variants (k_conv<..., GEO = 1>: whole 4 x 8 x 8 tiles of a stride-1
layer; csrc/conv.hip, Geo488), at the smallest shapes at which it can go wrong:

    N  D x H x W     tiles / sample
    1  4 x 8 x 8     1    every face of the one tile is padding
    2  8 x 16 x 16   8    the XCD range remap of the tile index; with 256 couts on the 128-cout tile the `cofast` order
    1  12 x 8 x 24   9    not a multiple of 8: the tail tile of the remap keeps its index; tile counts that are no powers of two

times the channel layers 32 -> 64 (one chunk), 64 -> 64, (64 + 32) -> 64 from two sources (a chunk crosses the concat boundary),
128 -> 128 and (128 + 64) -> 128 (the 8-wave variant) and one folded-skip layer per cout tile.

  * bit-exact against the fp64 reference on small-integer operands (the machinery of test_gpu_exact_conv.py), plain and with
    affine prologue + bias + residual + additive embedding + fused statistics; outputs and statistics are NaN-prefilled between
    guard bands;
  * byte-identical to the generic form (RHO_CONV_GEO=0) on random bf16 operands with a GroupNorm/FiLM-like affine + SiLU prologue,
    residual and statistics - two fresh child processes, one after the other, because the library latches the switch;
  * the path taken: rho_conv_variant reports "geo=1" behind the unchanged variant name for every case above and "geo=0" for a
    ragged twin (H = 12) and a 2-D twin, which still match the reference.
"""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [(1, (4, 8, 8)), (2, (8, 16, 16)), (1, (12, 8, 24))]
# (name, c1, c2, cout, skip)
LAYERS = [("32to64", 32, 0, 64, None), ("64to64", 64, 0, 64, None), ("64+32to64", 64, 32, 64, None), ("128to128", 128, 0, 128, None),
          ("128+64to128", 128, 64, 128, None), ("skip64", 64, 0, 64, (32, 32)), ("skip128", 128, 0, 128, (32, 32))]
EXTRA = [(2, (8, 16, 16), ("128to256", 128, 0, 256, None))]          # two 128-cout tiles on a grid of 8 position tiles: cofast


def _variant(cout, skip):
    bm = 128 if cout % 128 == 0 else 64
    return f"k_conv<bf16,3,3,3,BM={bm},MAXP={5 if bm == 128 else 10},NW={8 if bm == 128 else 4},M16=1>" + ("+skip" if skip else "")


def _w_scale(cin, full):
    """Weights are round(scale * z) clamped to +-1.  The scale keeps the standard deviation of an output near 10, so that every
    output stays an integer far below bf16's 256 (check_bf16_exact holds the reference to it): an input element has a mean square
    of about 0.64 (x in +-2), about 1.95 behind the integer affine prologue."""
    frac = min(0.3, 100.0 / (27 * cin * (1.95 if full else 0.64)))     # share of non-zero weights
    z = math.sqrt(2.0) * float(torch.erfinv(torch.tensor(1.0 - frac, dtype=torch.float64)))
    return 0.5 / z


def _case(N, spatial, layer, full, kernel=(3, 3, 3)):
    import exact_cases as X
    name, c1, c2, cout, skip = layer
    tag = f"geo_{name}_{N}x{'x'.join(map(str, spatial))}_{'full' if full else 'plain'}"
    # (fused statistics exist for 3-D kernels only: one sample per tile)
    return X._case(tag, N, spatial, c1, cout, kernel=kernel, c2=c2, pre=full, res=full, add=full, stats=full and kernel[0] == 3, skip=skip,
                   dtypes=(X.BF16,), w_scale=_w_scale(c1 + c2, full))


def _all():
    out = [(N, sp, layer) for N, sp in SHAPES for layer in LAYERS] + EXTRA
    return out


EXACT = [pytest.param(N, sp, layer, full, id=f"{layer[0]}-{N}x{'x'.join(map(str, sp))}-{'full' if full else 'plain'}")
         for N, sp, layer in _all() for full in (False, True)]


@pytest.fixture(scope="module")
def ops():
    from rho_diffusion_amd.engine import ops as o
    from rho_diffusion_amd import hip
    hip.load()
    return o


def _run_exact(ops, c, want_variant, want_detail):
    import exact_cases as X
    from exact_util import assert_bit_equal, check_bf16_exact, check_f32_exact, guarded, guards_intact
    from test_gpu_exact_conv import build_launch, check_outputs
    L = build_launch(ops, c, X.BF16)
    d = L["d"]
    sflat = sbuf = ids = None
    if c["stats"]:
        tiles = ops.conv_stats_tiles(d)
        assert tiles > 0
        sflat, sbuf = guarded((L["N"], tiles, 2, c["split"]), X.F32)
        d.stats = sbuf.data_ptr()
    variant, detail = ops.conv_variant(d), ops.conv_variant_detail(d)
    if want_variant is not None:
        assert variant == want_variant, variant
    assert detail == want_detail, (variant, detail)
    _, ref = X.fwd_reference(c, L["o"])
    check_bf16_exact(ref)
    if c["stats"]:
        ids = X.tile_ids(c, "k_conv")
        assert tiles == int(ids.max()) + 1, (tiles, int(ids.max()) + 1)
    ops.conv_launch(d)
    torch.cuda.synchronize()
    check_outputs(c, L, ref, f"{c['name']} {variant} {detail}")
    if c["stats"]:
        want = X.stats_reference(ref, ids)
        check_f32_exact(want, "statistics reference")
        assert_bit_equal(sbuf, want, f"{c['name']} {variant}: fused statistics [N, tile, (sum, sumsq), C]")
        assert guards_intact(sflat), "store outside the statistics buffer"


@pytest.mark.parametrize("N,spatial,layer,full", EXACT)
def test_geo_launch_is_bit_exact(ops, N, spatial, layer, full):
    _run_exact(ops, _case(N, spatial, layer, full), _variant(layer[3], layer[4]), "geo=1")


TWINS = [pytest.param(1, (4, 12, 8), (3, 3, 3), id="ragged-H12"), pytest.param(2, (8, 8), (1, 3, 3), id="2d")]


@pytest.mark.parametrize("N,spatial,kernel", TWINS)
@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_twins_outside_the_geometry_stay_generic_and_exact(ops, N, spatial, kernel, full):
    """H = 12 is no whole number of 8-row tiles, a 1x3x3 kernel is another instantiation: both keep the generic form."""
    _run_exact(ops, _case(N, spatial, LAYERS[1], full, kernel=kernel), None, "geo=0")


# ----------------------------------------------------------------------------- switch on / off: byte-identical
def _random_launches(ops):
    """Every (shape, layer) of this module on random bf16 operands: affine + SiLU prologue with real coefficients, residual,
    additive row, fused statistics.  Returns {name: (detail, y bytes, statistics bytes)}."""
    from detdata import det_normal, det_uniform
    bf = torch.bfloat16
    out = {}
    for N, sp, (name, c1, c2, cout, skip) in _all():
        D, H, W = sp
        tag = f"geor_{name}_{N}x{D}x{H}x{W}"
        cin = c1 + c2
        coutp = cout

        def clr(shape, t, s=1.0):
            return (det_normal(shape, t) * s).to(DEV).to(bf)

        x1 = clr((N, D, H, W, c1), tag + "x1")
        x2 = clr((N, D, H, W, c2), tag + "x2") if c2 else None
        w = ops.prep_conv_weight((det_normal((cout, cin, 3, 3, 3), tag + "w") / math.sqrt(27 * cin)).to(DEV), bf)
        b = det_normal((coutp,), tag + "b").to(DEV)
        pa = (1.0 + 0.3 * det_normal((N, cin), tag + "pa")).to(DEV)            # rstd * gamma * (1 + scale)
        pb = (0.3 * det_normal((N, cin), tag + "pb")).to(DEV)
        res = clr((N, D, H, W, cout), tag + "r")
        add = det_uniform((N, cout), tag + "add", -1.0, 1.0).to(DEV).contiguous()
        sk = None
        if skip:
            sx1, sx2 = clr((N, D, H, W, skip[0]), tag + "sx1"), clr((N, D, H, W, skip[1]), tag + "sx2")
            sw = ops.prep_conv_weight((det_normal((cout, sum(skip), 1, 1, 1), tag + "sw") / math.sqrt(sum(skip))).to(DEV), bf)
            sk = (sx1, sx2, sw, det_normal((coutp,), tag + "sb").to(DEV))
        y = torch.full((N, D, H, W, cout), float("nan"), dtype=bf, device=DEV)
        d = ops.make_conv_desc(x1, x2, w, b, kernel=(3, 3, 3), cout=cout, split=cout, y=y, y2=None, pre_a=pa, pre_b=pb, pre_silu=True,
                               res=res, res_add=add, res_add_stride=cout, skip=sk)
        tiles = ops.conv_stats_tiles(d)
        stats = torch.full((N, tiles, 2, cout), float("nan"), dtype=torch.float32, device=DEV)
        d.stats = stats.data_ptr()
        assert ops.conv_variant(d) == _variant(cout, skip)
        detail = ops.conv_variant_detail(d)
        ops.conv_launch(d)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(stats).all()), name
        out[tag] = (detail, y.cpu().view(torch.int16).clone(), stats.cpu().view(torch.int32).clone())
    return out


def _child_main(path):
    for p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from rho_diffusion_amd import hip
    from rho_diffusion_amd.engine import ops as o
    hip.load()
    torch.save(_random_launches(o), path)


def test_switch_off_gives_the_same_bytes(tmp_path):
    """RHO_CONV_GEO=1 against =0, each in a fresh process: the same outputs and statistics rows, byte for byte - the order of the
    MFMAs, of the statistics sums and of the prologue expressions is the generic form's."""
    got = {}
    for sw in ("1", "0"):
        path = str(tmp_path / f"geo{sw}.pt")
        env = dict(os.environ, RHO_CONV_GEO=sw, RHO_CONV_M16="1")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", path]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"RHO_CONV_GEO={sw}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        got[sw] = torch.load(path)
    assert set(got["1"]) == set(got["0"]) and len(got["1"]) == len(_all())
    for tag, (detail, y, stats) in got["1"].items():
        d0, y0, s0 = got["0"][tag]
        assert (detail, d0) == ("geo=1", "geo=0"), (tag, detail, d0)
        assert torch.equal(y, y0), f"{tag}: {int((y != y0).sum())} of {y.numel()} outputs differ between the two forms"
        assert torch.equal(stats, s0), f"{tag}: {int((stats != s0).sum())} of {stats.numel()} statistics differ between the two forms"


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child"
    _child_main(sys.argv[2])
