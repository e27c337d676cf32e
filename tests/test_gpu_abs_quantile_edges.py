"""-m gpu: the radix select of csrc/select.hip (rho_abs_quantile / _strided) at the inputs that force its paths: rows built from bit
patterns whose two ranks part at a chosen pass (the ``same`` flag and the second histogram of k_sel_hist), all-equal rows, +-0 with
denormals, N = 1 and 2, q = 0 and 1, a per-block span that is no multiple of 4 (scalar loop although N % 4 == 0), strided rows whose
other halves must not be counted, and a base one float off 16 bytes (scalar loop; same bits as the aligned call).

Reference: a float32 sort on the CPU.  torch.quantile's ranks: rank = float32(q) * float32(N - 1), lo = floor, hi = ceil, weight =
rank - lo.  Where the weight is 0 the result is the order statistic itself, bit for bit; elsewhere it lies between the two order
statistics and within 1 ulp (rtol 2.5e-7, the bar of test_abs_quantile_matches_torch) of torch.quantile.  Every call runs with sentinels
around ``out`` and around the workspace."""
import numpy as np
import pytest
import torch

from helpers import det_normal, det_uniform
from gpu_util import DEV, Guarded, bits, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32


def _run(x: torch.Tensor, q: float, shift: int = 0, stride=None):
    """x: CPU float32 [B, N] (or [B, stride] with ``stride``: the first N = stride // 2 of each row are the sample) -> out [B] CPU"""
    from rho_diffusion_amd import hip
    L = hip.lib()
    B = x.shape[0]
    N = x.shape[1] if stride is None else stride // 2
    xg = Guarded(x.reshape(-1).contiguous(), shift=shift)
    out = Guarded(B)
    ws = Guarded(torch.zeros(L.rho_abs_quantile_workspace_bytes(B) // 4, dtype=torch.int32))
    if stride is None:
        rc = L.rho_abs_quantile(xg.ptr, B, N, float(q), ws.ptr, out.ptr, hip.stream())
    else:
        rc = L.rho_abs_quantile_strided(xg.ptr, B, N, stride, float(q), ws.ptr, out.ptr, hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and xg.intact() and torch.equal(xg.cpu(), x.reshape(-1))
    return out.cpu()


def _check(got: torch.Tensor, rows: torch.Tensor, q: float):
    """rows: CPU float32 [B, N], the samples themselves"""
    N = rows.shape[1]
    srt = rows.abs().sort(dim=-1).values
    rank = f32(q) * f32(N - 1)
    lo, hi = int(np.floor(rank)), min(int(np.ceil(rank)), N - 1)
    if rank - f32(lo) == 0:
        assert same_bits(got, srt[:, lo]), (got, srt[:, lo])
        return
    assert torch.all(got >= srt[:, lo]) and torch.all(got <= srt[:, hi]), (got, srt[:, lo], srt[:, hi])
    assert torch.allclose(got, torch.quantile(rows.abs(), q, dim=-1), rtol=2.5e-7, atol=0.0)


def _q_for_rank(r: int, N: int) -> float:
    """a q (exact in float32, as the library casts it) whose rank float32(q) * float32(N - 1) is the integer r, so the weight is 0"""
    q = f32(r) / f32(N - 1)
    for c in (q, np.nextafter(q, f32(2)), np.nextafter(q, f32(-1))):
        if f32(c) * f32(N - 1) == f32(r):
            return float(c)
    raise AssertionError(f"no float32 q gives the rank {r} of {N}")


def _from_bits(v):
    return torch.from_numpy(np.asarray(v, dtype=np.uint32).view(np.float32).copy())


# the two middle order statistics A < B first differ in byte ``p`` (from the top), and A's lower bytes are smaller digits than B's: a
# second-rank histogram that also counted elements outside B's prefix bucket would meet A's digits first
SPLITS = {0: (0x3F101010, 0x40808080), 1: (0x3F7F1010, 0x3F808080), 2: (0x3F807F10, 0x3F808080), 3: (0x3F80807F, 0x3F808080)}


@pytest.mark.parametrize("p", sorted(SPLITS))
def test_ranks_part_at_a_chosen_pass(p):
    a, b = SPLITS[p]
    h, k = 300, 212                                              # N = 1024: rank 511.5, lo the last A, hi the first B
    rows = []
    for r in range(2):
        small = det_uniform((k,), f"qsplit_s{p}{r}", 0.0, 0.4)
        large = det_uniform((k,), f"qsplit_l{p}{r}", 5.0, 100.0)
        row = torch.cat([small, _from_bits([a] * h), _from_bits([b] * h), large])
        sign = torch.where(det_uniform((row.numel(),), f"qsplit_g{p}{r}") < 0, -1.0, 1.0)
        perm = torch.from_numpy(np.argsort(det_uniform((row.numel(),), f"qsplit_p{p}{r}").numpy(), kind="stable"))
        rows.append((row * sign)[perm])
    x = torch.stack(rows)
    srt = x.abs().sort(dim=-1).values
    assert same_bits(srt[:, 511], _from_bits([a, a])) and same_bits(srt[:, 512], _from_bits([b, b]))
    _check(_run(x, 0.5), x, 0.5)
    # weight 0 on either side of the boundary: the order statistics themselves
    for r, want in ((511, a), (512, b)):
        assert same_bits(_run(x, _q_for_rank(r, 1024)), _from_bits([want, want])), (p, r)


def test_all_equal_rows_zeros_denormals_and_tiny_rows():
    x = torch.full((2, 777), 1.25)
    x[1] = -3.0e-5
    for q in (0.0, 0.3, 0.9, 1.0):
        assert same_bits(_run(x, q), torch.tensor([1.25, 3.0e-5])), q
    # +0 / -0 with a few denormals: the masked keys order them, the result keeps the denormal's bits
    z = torch.zeros(1025)
    z[::2] = -0.0
    den = _from_bits([1, 2, 3, 0x7FFFFF, 0x400000, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94, 95, 96])
    z[100:125] = den * torch.tensor([1.0, -1.0] * 12 + [1.0])
    x = z[None]
    assert same_bits(_run(x, 0.5), torch.zeros(1))              # rank 512, weight 0: +0.0 whatever the sign bits were
    assert same_bits(_run(x, 1.0), _from_bits([0x7FFFFF]))
    assert same_bits(_run(x, 1023.0 / 1024.0), _from_bits([0x400000]))
    assert int(bits(_run(x, 0.99))) in (87, 88)                 # rank 1013.76: between the denormals with the bits 87 and 88
    for v in (-2.5, 0.0, 7.0):
        for q in (0.0, 0.5, 1.0):
            assert same_bits(_run(torch.tensor([[v]]), q), torch.tensor([abs(v)])), (v, q)
    x = torch.tensor([[3.0, -1.0], [-0.5, 0.25]])
    assert same_bits(_run(x, 0.5), torch.tensor([2.0, 0.375]))
    assert same_bits(_run(x, 0.0), torch.tensor([1.0, 0.25])) and same_bits(_run(x, 1.0), torch.tensor([3.0, 0.5]))


@pytest.mark.parametrize("q", [0.0, 1.0, 0.9])
def test_q_ends_on_a_plain_row(q):
    x = det_normal((3, 1000), "qends") * 3.0
    _check(_run(x, q), x, q)


def test_scalar_loop_when_the_block_span_is_no_multiple_of_4():
    """N = 524 292 = 4 * 131 073: 128 blocks of 4097 elements each, so the 16-byte path is off although N % 4 == 0"""
    x = det_normal((2, 524292), "qspan") * 2.0
    x[1] = x[1].abs() * 1e-3
    for q in (0.9, 0.5):
        _check(_run(x, q), x, q)


def test_strided_rows_skip_the_other_halves_and_misaligned_bases_give_the_same_bits():
    from rho_diffusion_amd.engine import ops
    N, B = 1028, 3
    rows = det_normal((B, N), "qstride") * 3.0
    x = torch.full((B, 2 * N), 1e30)
    x[:, :N] = rows
    for q in (0.9, 1.0):
        got = _run(x, q, stride=2 * N)
        _check(got, rows, q)
        assert same_bits(got, _run(rows, q))
        # one float off 16 bytes: the scalar loop, same bits (strided and contiguous)
        assert same_bits(got, _run(x, q, shift=1, stride=2 * N)) and same_bits(got, _run(rows, q, shift=3))
        # through the wrapper: the mean half of a [B, 2C, ...] tensor read in place, aligned and as a view at an odd storage offset
        xd = x.to(DEV).view(B, 2, N)
        assert same_bits(ops.abs_quantile(xd[:, :1], q), got)
        buf = torch.full((B * 2 * N + 1,), 1e30, device=DEV)
        buf[1:].copy_(x.reshape(-1))
        off = buf[1:].view(B, 2, N)
        assert off.data_ptr() % 16 == 4
        assert same_bits(ops.abs_quantile(off[:, :1], q), got)
    one = det_normal((1, N), "qstride1")
    assert same_bits(_run(one, 0.9), _run(one, 0.9, shift=1))
