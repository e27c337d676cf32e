"""The conv launches of the c3 sampling plan (development aid): variant name, the form rho_conv_variant reports behind it (geo=1 = compile-time
4 x 8 x 8 tile geometry, geo=0 = generic), shape and HIP-event time of every launch, and the time the geo=1 launches cover.
usage (GPU box): python tools/conv_geo_forms.py"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch
import bench
from rho_diffusion_amd.engine import ops
args = argparse.Namespace(grid=64, dims=3, mc=64, dtype="bf16", labels=False, batch=32)
dev = "cuda:0"
ddpm, kw = bench.build_model(args, dev)
engine = ddpm.backbone.engine()
x = torch.randn(32, 1, 64, 64, 64, device=dev)
t_dev = torch.full((1,), 999, dtype=torch.int32, device=dev)
with torch.no_grad():
    engine.forward(x, None, None, t_scalar_dev=t_dev)
torch.cuda.synchronize()
plan = next(iter(engine._plans.values()))
prof = plan.profile(repeats=3)
convs = [p for p in prof if p["kind"] in ("conv3", "conv1")]
descs = plan.fwd_descs
print("launches in profile (conv3 + conv1):", len(convs), " descriptors:", len(descs))
tot = sum(p["ms"] for p in prof)
rows = []
for i, d in enumerate(descs):
    v, det = ops.conv_variant(d), ops.conv_variant_detail(d)
    rows.append((v, det, d.c1 + d.c2, d.cout, (d.kd, d.kh, d.kw), (d.n, d.d, d.h, d.w_), (d.sh, d.sw), (d.up_h, d.up_w), (d.ph_h, d.ph_w), (d.phd_h, d.phd_w)))
if len(convs) == len(descs):
    for r, p in zip(rows, convs):
        print(f"{p['kind']:6s} ms={p['ms']:7.3f} share={100 * p['ms'] / tot:5.2f}% {r[1]} {r[0]:55s} cin={r[2]} cout={r[3]} k={r[4]} ndhw={r[5]} s={r[6]} up={r[7]} ph={r[8]} phd={r[9]}")
    g1 = sum(p["ms"] for r, p in zip(rows, convs) if r[1] == "geo=1")
    c3 = sum(p["ms"] for p in convs if p["kind"] == "conv3")
    print(f"all kernels {tot:.3f} ms; conv3 {c3:.3f} ms; geo=1 launches {sum(r[1] == 'geo=1' for r in rows)} with {g1:.3f} ms")
else:
    for r in rows:
        print(r)
