// The wide 1x1x1 convolutions (attention qkv / proj_out, un-folded skips, their data gradients) as a plain bf16 GEMM
//
//     Y[pos][cout] = sum_k X[pos][k] * W[cout][k] + bias[cout] (+ res[pos][cout])
//
// with both operands K-contiguous (channels-last activations, prepared weights [cout][cin]).  k_conv<.,1,1,1,...> ran these
// through its halo-tile machinery degenerated to one tap: a 64-byte K chunk and 16 MFMAs per wave between barriers, a per-thread
// halo-slot decode, and an fp32 LDS transpose in the epilogue.  Here:
//
//   * Tile: 256 positions x 128 couts per workgroup, BK = 64 (128-byte rows), 8 waves as 4 (positions) x 2 (couts), 64 x 64 per
//     wave = 4 x 4 accumulators of v_mfma_f32_16x16x32_bf16 (64 accumulator registers).  The 256 positions are one row of the
//     fused GroupNorm statistics buffer [N][S / 256][2][cout], which is what rho_conv_stats_tiles reports for 1x1x1 launches.
//   * Staging: LDS-DMA (global_load_lds_dwordx4, the inline-asm statement of wgrad.hip) into a ring of THREE buffers of
//     (256 + 128) rows x 128 B = 48 KiB (144 KiB, one workgroup per CU, two waves per SIMD).  Per K-step a wave issues 6 DMAs of
//     1 KiB; K-step k + 2 is issued while K-step k computes, `s_waitcnt vmcnt(6)` (vmcnt(0) at the last step) retires K-step k
//     and ONE barrier per K-step both publishes it and frees the buffer K-step k - 1 was read from (the ring slot of k + 2).
//     All LDS is one array.  The barrier is __syncthreads(): the compiler does not see the inline-asm DMAs, so it emits a bare
//     s_barrier there (no vmcnt(0) that would drain the ring) - checked in the gfx950 disassembly of the loop: the only vmcnt
//     waits inside it are the two written here.
//   * LDS image: rows are linear (the DMA writes wave base + 16 B x lane), the 16-byte pieces of row R are stored at piece
//     p ^ ((R >> 1) & 7) by permuting the per-lane SOURCE address; the fragment reads apply the same XOR.  A ds_read_b128 is served
//     in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32); a lane reads row i = lane & 15 of a 16-row fragment at
//     K piece q + (lane >> 4).  Slot (16-byte bank group) = 8 * (R & 1) + (piece ^ ((R >> 1) & 7)): within a group the eight rows
//     at piece q and the eight at piece q ^ 1 give (R >> 1) ^ q = all eight values, each for both parities of R - 16 distinct
//     slots, conflict-free.
//   * No transpose in the epilogue: a workgroup's cout tile lies wholly below `split` (channels-last y) or wholly above it
//     (channel-major y2, the attention's V^T), so the MFMA operand order is chosen by that block-uniform fact.  Weights as A
//     leaves a lane 4 couts of one position, activations as A leaves it 4 positions of one cout.  The rows of a fragment are
//     dealt so that the four fragments of a wave give a lane 16 CONSECUTIVE couts (positions): MFMA row r of fragment f is
//     cout (position) 16 * (r >> 2) + 4 * f + (r & 3) of the wave's 64 - a permutation of the DMA's source rows, free.  Stores
//     and residual loads are 16-byte pieces, and the four lanes that share a position (cout) cover one 128-byte line.
//   * Statistics: the values as stored (rounded, residual included), summed per lane over its 4 positions per fragment, over the
//     16 position lanes by an xor butterfly, and over the four position waves through LDS in wave order: fixed order, no atomics.
//   * XCD placement: the launch is one linear grid; slot L / 8 of XCD label L % 8 maps to consecutive tiles of that label's range
//     (bijective for every grid size), and the cout tiles of a position tile are consecutive, so the 256 x cin activation tile
//     comes from HBM once and from that L2 afterwards.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "conv_common.h"

#define G1_BN 128                          // couts per workgroup
#define G1_ROWS (256 + G1_BN)              // LDS rows per K-step: activations, then weights
#define G1_BUF (G1_ROWS * 128)             // bytes per ring slot
#define G1_NBUF 3
#define G1_DMA (G1_ROWS / 64)              // DMAs per wave and K-step (8 waves x 8 rows each)

struct Gemm1K {
    const char* x;
    const char* w;
    const float* bias;
    const char* res;
    char* y;
    char* y2;
    float* stats;
    int cin, cout, split;
    int ctiles;            // cout tiles
    int tps;               // position tiles per sample (S / 256) where the launch needs the sample of a tile, else 1
    long long S;           // positions per sample
};

__device__ __forceinline__ void g1_unpack8(const uint4& r, float* v) {
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
    v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xFFFF0000u);
    v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xFFFF0000u);
}

__global__ __launch_bounds__(512) void k_gemm1x1(const Gemm1K p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wp = wave & 3;               // position quarter of this wave
    const int wc = wave >> 2;              // cout half
    const int fi = lane & 15;              // fragment row / column of this lane
    const int fg = lane >> 4;              // its K piece within a 32-deep MFMA step, its 4-row group in the accumulator

    // ---- tile of this workgroup
    int wg;
    {
        const int nwg = (int)gridDim.x, L = (int)blockIdx.x;
        const int xcd = L & 7, q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    }
    const int ct = wg % p.ctiles, bt = wg / p.ctiles;
    const int co0 = ct * G1_BN;
    const long long pos0 = (long long)bt * 256;

    // ---- DMA sources: LDS row R = 64 * j + 8 * wave + (lane >> 3), physical piece lane & 7
    const char* src[G1_DMA];
#pragma unroll
    for (int j = 0; j < G1_DMA; ++j) {
        const int R = j * 64 + wave * 8 + (lane >> 3);
        const int lp = (lane & 7) ^ ((R >> 1) & 7);                        // the logical K piece stored there
        const int r = R & 15, f = (R >> 4) & 3, w64 = (R >> 6) & 3;        // MFMA row, fragment, wave chunk
        const int m = w64 * 64 + (r >> 2) * 16 + f * 4 + (r & 3);          // position / cout of that row
        if (j < 4) src[j] = p.x + (size_t)(pos0 + m) * (size_t)p.cin * 2 + lp * 16;
        else src[j] = p.w + (size_t)(co0 + (m & (G1_BN - 1))) * (size_t)p.cin * 2 + lp * 16;
    }
    const unsigned ldsw = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)wave * 1024u);
    // (M0 is left as set, see wgrad.hip; tests/test_cabi.py checks the disassembly)
    auto glds16 = [&](const char* gsrc, unsigned lds_dst) {               // wave-uniform LDS base + 16 bytes x lane
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(lds_dst) : "memory");
    };
    auto issue = [&](int buf) {                                           // the next K-step of every source row
#pragma unroll
        for (int j = 0; j < G1_DMA; ++j) {
            glds16(src[j], ldsw + (unsigned)buf * G1_BUF + (unsigned)j * 8192u);
            src[j] += 128;
        }
    };

    // ---- fragment reads: row fi of fragment f at (wave chunk * 64 + 16 f + fi) * 128, piece (4 kk + fg) ^ (fi >> 1)
    const int offk0 = ((fg) ^ (fi >> 1)) * 16, offk1 = ((4 + fg) ^ (fi >> 1)) * 16;
    const int offp = (wp * 64 + fi) * 128;
    const int offc = (256 + wc * 64 + fi) * 128;

    f32x4_t acc[4][4];                      // [cout fragment][position fragment]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};

    const int nk = p.cin >> 6;
    const bool yreg = co0 < p.split;        // block-uniform: channels-last region
    auto kloop = [&](auto YREG) {
        constexpr bool W_IS_A = decltype(YREG)::value;
        issue(0);
        if (nk > 1) issue(1);
        int cur = 0, nxt = 2;               // ring slots of K-step k and k + 2
        for (int k = 0; k < nk; ++k) {
            if (k + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(G1_DMA) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (k + 2 < nk) issue(nxt);
            const char* const base = smem + cur * G1_BUF;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int ok = kk ? offk1 : offk0;
                bf16x8_t fp[4], fc[4];
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    fp[f] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(base + offp + f * 2048 + ok));
                    fc[f] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(base + offc + f * 2048 + ok));
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        if constexpr (W_IS_A) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fc[a], fp[b], acc[a][b], 0, 0, 0);
                        else acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fp[b], fc[a], acc[a][b], 0, 0, 0);
                    }
            }
            cur = cur == G1_NBUF - 1 ? 0 : cur + 1;
            nxt = nxt == G1_NBUF - 1 ? 0 : nxt + 1;
        }
    };
    if (yreg) kloop(std::true_type{});
    else kloop(std::false_type{});

    if (yreg) {
        // ---- channels-last: acc[a][b][j] = cout cl + 4 a + j of position column fi of position fragment b
        const int cl = co0 + wc * 64 + fg * 16;
        float bia[16];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float4 b4 = *reinterpret_cast<const float4*>(p.bias + cl + a * 4);
            bia[a * 4 + 0] = b4.x; bia[a * 4 + 1] = b4.y; bia[a * 4 + 2] = b4.z; bia[a * 4 + 3] = b4.w;
        }
        size_t eo[4];
        uint4 rr[4][2];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long long P = pos0 + wp * 64 + (fi >> 2) * 16 + b * 4 + (fi & 3);
            eo[b] = ((size_t)P * (size_t)p.split + (size_t)cl) * 2;
            rr[b][0] = rr[b][1] = make_uint4(0u, 0u, 0u, 0u);
            if (p.res != nullptr) {
                rr[b][0] = *reinterpret_cast<const uint4*>(p.res + eo[b]);
                rr[b][1] = *reinterpret_cast<const uint4*>(p.res + eo[b] + 16);
            }
        }
        float ssum[16], ssq[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) ssum[e] = ssq[e] = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float v[16];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[a * 4 + j] = acc[a][b][j] + bia[a * 4 + j];
            if (p.res != nullptr) {
                float rv[16];
                g1_unpack8(rr[b][0], rv);
                g1_unpack8(rr[b][1], rv + 8);
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] += rv[e];
            }
            typedef unsigned int u32x4_nt __attribute__((ext_vector_type(4)));
            const u32x4_nt o0 = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
            const u32x4_nt o1 = {pack_bf16x2(v[8], v[9]), pack_bf16x2(v[10], v[11]), pack_bf16x2(v[12], v[13]), pack_bf16x2(v[14], v[15])};
            __builtin_nontemporal_store(o0, reinterpret_cast<u32x4_nt*>(p.y + eo[b]));
            __builtin_nontemporal_store(o1, reinterpret_cast<u32x4_nt*>(p.y + eo[b] + 16));
            if (p.stats != nullptr) {       // statistics of the values as stored (what a reader would see)
                float sv[16];
                g1_unpack8(make_uint4(o0.x, o0.y, o0.z, o0.w), sv);
                g1_unpack8(make_uint4(o1.x, o1.y, o1.z, o1.w), sv + 8);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    ssum[e] += sv[e];
                    ssq[e] = fmaf(sv[e], sv[e], ssq[e]);
                }
            }
        }
        if (p.stats != nullptr) {
            // the 16 position lanes of a cout group (xor butterfly: every lane ends with the same sum), then the four position waves
            // through LDS in wave order
#pragma unroll
            for (int e = 0; e < 16; ++e) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    ssum[e] += __shfl_xor(ssum[e], o, 64);
                    ssq[e] += __shfl_xor(ssq[e], o, 64);
                }
            }
            __syncthreads();                // every wave is done with the last K-step's buffer
            float* const red = reinterpret_cast<float*>(smem);             // [4 position waves][2][G1_BN]
            if (fi == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    red[(wp * 2 + 0) * G1_BN + wc * 64 + fg * 16 + e] = ssum[e];
                    red[(wp * 2 + 1) * G1_BN + wc * 64 + fg * 16 + e] = ssq[e];
                }
            }
            __syncthreads();
            if (tid < 2 * G1_BN) {
                const int stat = tid / G1_BN, ch = tid % G1_BN;
                float a = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) a += red[(q * 2 + stat) * G1_BN + ch];
                // row (sample, tile of the sample) of [N][S / 256][2][split] = the launch's position tile
                p.stats[((size_t)bt * 2 + stat) * (size_t)p.split + co0 + ch] = a;
            }
        }
        return;
    }
    // ---- channel-major y2 [N][cout - split][S]: acc[a][b][j] = position 16 fg + 4 b + j of the wave's 64, cout column fi of fragment a
    const int ns = bt / p.tps;
    const long long ps = (long long)(bt % p.tps) * 256 + wp * 64 + fg * 16;
    const int w2 = p.cout - p.split;
    float bia[4];                           // (all four ahead of the stores: a load between them waits for the stores in front of it)
#pragma unroll
    for (int a = 0; a < 4; ++a) bia[a] = p.bias[co0 + wc * 64 + (fi >> 2) * 16 + a * 4 + (fi & 3)];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int co = co0 + wc * 64 + (fi >> 2) * 16 + a * 4 + (fi & 3);
        const float bv = bia[a];
        char* const dst = p.y2 + (((size_t)ns * (size_t)w2 + (size_t)(co - p.split)) * (size_t)p.S + (size_t)ps) * 2;
        float v[16];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[b * 4 + j] = acc[a][b][j] + bv;
        *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
        *reinterpret_cast<uint4*>(dst + 16) =
            make_uint4(pack_bf16x2(v[8], v[9]), pack_bf16x2(v[10], v[11]), pack_bf16x2(v[12], v[13]), pack_bf16x2(v[14], v[15]));
    }
}

// ------------------------------------------------------------------------------------------ host
// Read at every call (a getenv, no static): the switch takes effect for the next plan, and the engine keys its plans on it.
static bool gemm1x1_on() {
    const char* e = getenv("RHO_GEMM1X1");
    return !(e && atoi(e) == 0);
}

static bool gemm1x1_applies(const rho_conv_desc& d) {
    if (!gemm1x1_on()) return false;
    if (d.dtype != RHO_BF16 || d.kd != 1 || d.kh != 1 || d.kw != 1 || d.sh != 1 || d.sw != 1 || d.up_h || d.up_w) return false;
    if (d.x2 || d.pre_a || d.pre_b || d.res_add || d.y2_f32 || d.y2_cl || d.res2 || d.gnb_x1 || d.gna_g || d.sk_w) return false;
    if (d.zs_h || d.zs_w || d.ph_h || d.ph_w || d.phd_h || d.phd_w) return false;
    if (d.c1 % 64 || d.coutp != d.cout || d.cout % G1_BN || d.split % G1_BN) return false;
    if ((d.split > 0 && !d.y) || (d.split < d.cout && !d.y2) || (d.stats && d.split != d.cout)) return false;   // (k_conv reports these)
    // every operand moves in 16-byte pieces (DMA, float4 bias, residual loads, stores)
    const uintptr_t al = (uintptr_t)d.x1 | (uintptr_t)d.w | (uintptr_t)d.bias | (uintptr_t)d.y | (uintptr_t)d.y2 | (uintptr_t)d.res;
    if (al & 15) return false;
    const long long S = (long long)d.d * d.h * d.w_, total = S * d.n;
    if (total % 256 || total >= (1LL << 31)) return false;
    if ((d.stats || d.split < d.cout) && S % 256) return false;           // such tiles must lie in one sample
    const long long wgs = total / 256 * (d.cout / G1_BN);
    if (wgs > 0x7FFFFFFFLL) return false;
    // grids that leave half the chip idle and that k_conv may split over K (rho_conv_desc.ws) stay there
    if (d.split == d.cout && !d.stats && wgs <= 128 && d.c1 / 32 >= 4) return false;
    return true;
}
// statistics rows per sample: one per 256 positions, as k_conv's 1x1x1 launches
static int64_t gemm1x1_stats_tiles(const rho_conv_desc& d) {
    const long long S = (long long)d.d * d.h * d.w_;
    return (d.split == d.cout && S % 256 == 0) ? S / 256 : 0;
}
static int launch_gemm1x1(const rho_conv_desc& d, hipStream_t st) {
    Gemm1K k{};
    k.x = (const char*)d.x1; k.w = (const char*)d.w; k.bias = d.bias; k.res = (const char*)d.res;
    k.y = (char*)d.y; k.y2 = (char*)d.y2; k.stats = d.stats;
    k.cin = d.c1; k.cout = d.cout; k.split = d.split;
    k.ctiles = d.cout / G1_BN;
    k.S = (long long)d.d * d.h * d.w_;
    k.tps = (k.S % 256 == 0) ? (int)(k.S / 256) : 1;
    const long long wgs = k.S * d.n / 256 * k.ctiles;
    const size_t lds = (size_t)G1_NBUF * G1_BUF;
    // (once per process, not per launch: the attribute belongs to the function)
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gemm1x1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (attr != hipSuccess) return (int)attr;
    hipError_t e;
    hipLaunchKernelGGL(k_gemm1x1, dim3((unsigned)wgs), dim3(512), lds, st, k);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
