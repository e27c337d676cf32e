"""Same-box A/B of rho_attention_fwd / rho_attention_bwd in bf16 (not a product path): tools/probe/librho_head.so (AB_REF overrides; a
build of the committed tree) vs the in-tree library (AB_NEW overrides: a second copy of the reference build there measures the
spread of the timing itself).

Bit identity: per shape and direction, whether out, lse (forward) and dqkv (backward) are equal bit for bit between the two
libraries, on the same random operands - the c3 (T = 4096, ch = 128, B = 32) and c5 (T = 32768, ch = 64, B = 2) bench shapes and the
small shapes of tests/attn_cases.py::CASES and tests/exact_cases.py::ATTN_CASES (ragged tiles, T % 8 != 0, every head width).
Timing: the two bench shapes, the libraries alternated window by window, forward and backward; median over the windows.
RHO_ATTN_DKV_SPLIT=1 in the environment puts both libraries on the dK / dV pair at ch = 64 instead of the fused kernel.
Exit status 1 if any output differs.  usage: python tools/ab_attn.py"""
import ctypes as C, os, statistics, sys, time
R0 = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R0)
sys.path[:0] = [os.path.join(R0, "tests"), os.path.join(R0, "tests", "golden")]      # the case lists and what they import
import torch
from rho_diffusion_amd import hip  # noqa: F401
from rho_diffusion_amd.hip import check_abi
from attn_cases import CASES
from exact_cases import ATTN_CASES

dev = "cuda"
vp = C.c_void_p
libs = {"ref": C.CDLL(os.path.join(R0, os.environ.get("AB_REF", "tools/probe/librho_head.so"))),
        "new": C.CDLL(os.path.join(R0, os.environ.get("AB_NEW", "rho_diffusion_amd/librho_hip.so")))}
for _n, _l in libs.items():
    check_abi(_l, _n)      # a probe build with older signatures would be called with shifted arguments
    _l.rho_attention_fwd.restype = _l.rho_attention_bwd.restype = C.c_int
    _l.rho_attention_fwd.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
    _l.rho_attention_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, vp]
BENCH = [(32, 4096, 4, 128), (2, 32768, 4, 64)]
WINDOWS, WINDOW_S = 7, 0.25


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


all_equal = True
for (B, T, heads, ch) in BENCH + CASES + ATTN_CASES:
    Cc = heads * ch
    g = torch.Generator(device=dev).manual_seed(1000 * T + ch)
    qk = (torch.randn(B, T, 2 * Cc, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    vt = (torch.randn(B, Cc, T, device=dev, generator=g) * 0.5).to(torch.bfloat16)
    dout = (torch.randn(B, T, Cc, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    fns, bufs = {}, {}
    for k, lib in libs.items():
        out = torch.zeros(B, T, Cc, device=dev, dtype=torch.bfloat16)
        lse = torch.zeros(B, heads, T, device=dev)
        delta = torch.zeros(B, heads, T, device=dev)
        dqkv = torch.zeros(B, T, 3 * Cc, device=dev, dtype=torch.bfloat16)
        bufs[k] = (out, lse, dqkv, delta)

        def fwd(lib=lib, out=out, lse=lse):
            return lib.rho_attention_fwd(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, B, T, heads, ch, st)

        def bwd(lib=lib, out=out, lse=lse, delta=delta, dqkv=dqkv):
            return lib.rho_attention_bwd(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(),
                                         dqkv.data_ptr(), 3 * Cc, dqkv.data_ptr() + 2 * Cc * 2, 3 * Cc, 1, B, T, heads, ch, st)
        fns[k] = {"fwd": fwd, "bwd": bwd}
        assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    eq = {"out": torch.equal(bits(bufs["ref"][0]), bits(bufs["new"][0])), "lse": torch.equal(bits(bufs["ref"][1]), bits(bufs["new"][1])),
          "dqkv": torch.equal(bits(bufs["ref"][2]), bits(bufs["new"][2]))}
    all_equal = all_equal and all(eq.values())
    print(f"B={B} T={T} heads={heads} ch={ch}  fwd: out {'equal' if eq['out'] else 'DIFFERS'}, lse {'equal' if eq['lse'] else 'DIFFERS'}"
          f"  bwd: dqkv {'equal' if eq['dqkv'] else 'DIFFERS'}", flush=True)
    if (B, T, heads, ch) not in BENCH:
        continue
    fl_f = 4.0 * B * heads * T * T * ch
    for name, fl in (("fwd", fl_f), ("bwd", 3.5 * fl_f)):
        t0 = time.perf_counter(); fns["ref"][name](); torch.cuda.synchronize(); one = time.perf_counter() - t0
        reps = max(3, int(WINDOW_S / one))
        ms = {k: [] for k in libs}
        for _ in range(WINDOWS):
            for k in libs:                           # ref, new, ref, new, ...
                t0 = time.perf_counter()
                for _ in range(reps):
                    fns[k][name]()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / reps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(f"   {name}: ref {med['ref']:.3f} ms ({fl / med['ref'] / 1e9:.0f} TF/s, windows {min(ms['ref']):.3f} - {max(ms['ref']):.3f})"
              f"  new {med['new']:.3f} ms ({fl / med['new'] / 1e9:.0f} TF/s, windows {min(ms['new']):.3f} - {max(ms['new']):.3f})"
              f"  new/ref {med['new'] / med['ref'] - 1:+.2%}", flush=True)
print("bit identity:", "equal everywhere" if all_equal else "DIFFERENCES (see above)", flush=True)
sys.exit(0 if all_equal else 1)
