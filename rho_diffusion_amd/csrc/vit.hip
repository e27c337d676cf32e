// VisionTransformer backbone (rho_diffusion/models/vit.py:32-372): the kernels the conv / attention engine does not already have.
//   LayerNorm over the embedding axis of token rows [R, E] (nn.LayerNorm(embed_dim), vit.py:145-146,178,182) with the broadcast add
//   of the time embedding (vit.py:175-176) fused into the load, forward and backward;
//   the patch gather / scatter between [B, C, *spatial] float32 and token rows [B, N, Kp] (the kernel = stride = p convolutions of
//   vit.py:73-78 and :282-288 are a GEMM over these rows);
//   activation forward / backward over rows for all six activation codes (vit.py:157-164,167-171,291-295);
//   the positional-embedding add over the batch and its gradient (vit.py:351-353).
// All of them are HBM-bound: 16-byte accesses, statistics and reductions in float32, no atomics, fixed summation orders.
#include <math.h>

#include "common.h"

namespace {

constexpr int LN_MAX_E = 2048;          // rows are held in registers: 8 (f32) / 4 (bf16) 16-byte vectors per lane of a full wave
constexpr float LN_EPS = 1e-5f;

template <typename T> struct V16;
template <> struct V16<float> {
    static constexpr int PE = 4;
    static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
        const float4 r = *reinterpret_cast<const float4*>(p);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
    static __device__ __forceinline__ void st(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <> struct V16<bf16_raw> {
    static constexpr int PE = 8;
    static __device__ __forceinline__ void ld(const bf16_raw* p, float (&v)[8]) {
        const uint4 r = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(w[j] << 16);
            v[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
        }
    }
    static __device__ __forceinline__ void st(bf16_raw* p, const float (&v)[8]) {
        uint4 o;
        o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]); o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4*>(p) = o;
    }
};

// sum over the G lanes (a power of two <= 64, aligned inside the wave) that share a row
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float act_any(float u, int act) { return act == 1 ? silu_f(u) : act_other_f(u, act); }
__device__ __forceinline__ float dact_any(float u, int act) { return act == 1 ? dsilu_f(u) : dact_other_f(u, act); }

// Row geometry shared by the two LayerNorm kernels: G lanes per row (a fixed fraction of a wave), NV vectors per lane.
struct LnGeom { int G, lgG, NV, rpb; };
inline LnGeom ln_geom(int64_t e, int pe) {
    const int nvec = (int)(e / pe);
    LnGeom g{};
    g.G = 4; g.lgG = 2;
    while (g.G < nvec && g.G < 64) { g.G <<= 1; ++g.lgG; }
    const int per = (nvec + g.G - 1) / g.G;
    g.NV = 1;
    while (g.NV < per) g.NV <<= 1;
    g.rpb = 256 / g.G;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm forward
// y[r, :] = (x'[r, :] - mean) * rstd * gamma + beta with x' = x[r, :] + add[r / rps, :]; two passes over the registers that hold the row.
template <typename T, int NV>
__global__ __launch_bounds__(256) void k_ln_fwd(const T* __restrict__ x, const float* __restrict__ add, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, T* __restrict__ y, float* __restrict__ stats,
                                                int64_t rows, int64_t rps, int e, int G, int lgG) {
    constexpr int PE = V16<T>::PE;
    const int g = threadIdx.x & (G - 1), slot = threadIdx.x >> lgG;
    const int64_t r = (int64_t)blockIdx.x * (256 >> lgG) + slot;
    const bool live = r < rows;
    const int nvec = e / PE;
    const float* ad = (add != nullptr && live) ? add + (r / rps) * e : nullptr;
    float v[NV][PE];
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int vi = j * G + g;
        if (live && vi < nvec) {
            V16<T>::ld(x + r * e + vi * PE, v[j]);
            if (ad) {
#pragma unroll
                for (int q = 0; q < PE; ++q) v[j][q] += ad[vi * PE + q];
            }
        } else {
#pragma unroll
            for (int q = 0; q < PE; ++q) v[j][q] = 0.0f;
        }
#pragma unroll
        for (int q = 0; q < PE; ++q) s += v[j][q];
    }
    const float mean = group_sum(s, G) / (float)e;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (j * G + g < nvec) {
#pragma unroll
            for (int q = 0; q < PE; ++q) { const float d = v[j][q] - mean; sq = fmaf(d, d, sq); }
        }
    }
    const float var = group_sum(sq, G) / (float)e;
    const float rstd = 1.0f / sqrtf(var + LN_EPS);
    if (!live) return;
    if (g == 0) { stats[2 * r] = mean; stats[2 * r + 1] = rstd; }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int vi = j * G + g;
        if (vi < nvec) {
            float o[PE];
#pragma unroll
            for (int q = 0; q < PE; ++q) o[q] = fmaf((v[j][q] - mean) * rstd, gamma[vi * PE + q], beta[vi * PE + q]);
            V16<T>::st(y + r * e + vi * PE, o);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- LayerNorm backward
// Block (k, b) walks the rows k * rpb + slot, + bps * rpb, ... of sample b:  g = dy * gamma,
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat))   (written, or added to what dx holds)
// and keeps per-lane column sums of dy * xhat, dy and dx over its rows; the row slots of the block are then added in slot order through
// LDS into partials [b][k][3][e] which k_ln_bwd_fin adds in (b, k) order: every sum has one fixed order.
template <typename T, int NV, bool HAS_ADD>
__global__ __launch_bounds__(256) void k_ln_bwd(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ add,
                                                const float* __restrict__ stats, const float* __restrict__ gamma, T* __restrict__ dx,
                                                int acc_dx, float* __restrict__ part, int64_t rps, int e, int G, int lgG) {
    constexpr int PE = V16<T>::PE;
    __shared__ __attribute__((aligned(16))) float sh[8192];
    const int g = threadIdx.x & (G - 1), slot = threadIdx.x >> lgG;
    const int rpb = 256 >> lgG;
    const int k = blockIdx.x, bps = gridDim.x;
    const int64_t b = blockIdx.y;
    const int nvec = e / PE;
    const float inv_e = 1.0f / (float)e;
    float ga[NV][PE], sg[NV][PE], sb[NV][PE], sa[HAS_ADD ? NV : 1][PE];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int vi = j * G + g;
#pragma unroll
        for (int q = 0; q < PE; ++q) {
            ga[j][q] = vi < nvec ? gamma[vi * PE + q] : 0.0f;
            sg[j][q] = 0.0f; sb[j][q] = 0.0f;
            if (HAS_ADD) sa[j][q] = 0.0f;
        }
    }
    for (int64_t base = (int64_t)k * rpb; base < rps; base += (int64_t)bps * rpb) {
        const int64_t rl = base + slot;
        const bool live = rl < rps;
        const int64_t r = b * rps + rl;
        float xh[NV][PE], gy[NV][PE];
        float mean = 0.0f, rstd = 0.0f;
        if (live) { mean = stats[2 * r]; rstd = stats[2 * r + 1]; }
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int vi = j * G + g;
            if (live && vi < nvec) {
                V16<T>::ld(x + r * e + vi * PE, xh[j]);
                V16<T>::ld(dy + r * e + vi * PE, gy[j]);
#pragma unroll
                for (int q = 0; q < PE; ++q) {
                    float xv = xh[j][q];
                    if (HAS_ADD) xv += add[b * e + vi * PE + q];
                    xh[j][q] = (xv - mean) * rstd;
                    const float d = gy[j][q];
                    sb[j][q] += d;
                    sg[j][q] = fmaf(d, xh[j][q], sg[j][q]);
                    gy[j][q] = d * ga[j][q];
                    s1 += gy[j][q];
                    s2 = fmaf(gy[j][q], xh[j][q], s2);
                }
            } else {
#pragma unroll
                for (int q = 0; q < PE; ++q) { xh[j][q] = 0.0f; gy[j][q] = 0.0f; }
            }
        }
        const float m1 = group_sum(s1, G) * inv_e, m2 = group_sum(s2, G) * inv_e;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int vi = j * G + g;
            if (live && vi < nvec) {
                float o[PE];
#pragma unroll
                for (int q = 0; q < PE; ++q) {
                    o[q] = rstd * (gy[j][q] - m1 - xh[j][q] * m2);
                    if (HAS_ADD) sa[j][q] += o[q];
                }
                if (acc_dx) {
                    float old[PE];
                    V16<T>::ld(dx + r * e + vi * PE, old);
#pragma unroll
                    for (int q = 0; q < PE; ++q) o[q] += old[q];
                }
                V16<T>::st(dx + r * e + vi * PE, o);
            }
        }
    }
    // row slots -> one partial row per block, slot order
    float* pb = part + ((b * bps + k) * 3) * (int64_t)e;
    constexpr int NCOMP = HAS_ADD ? 3 : 2;
#pragma unroll
    for (int comp = 0; comp < NCOMP; ++comp) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int vi = j * G + g;
            if (vi < nvec) {
#pragma unroll
                for (int q = 0; q < PE; ++q)
                    sh[slot * e + vi * PE + q] = comp == 0 ? sg[j][q] : comp == 1 ? sb[j][q] : sa[HAS_ADD ? j : 0][q];
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < e; c += 256) {
            float t = 0.0f;
            for (int s = 0; s < rpb; ++s) t += sh[s * e + c];
            pb[(int64_t)comp * e + c] = t;
        }
        __syncthreads();
    }
}

// Second level of the row reductions: 32 columns x 8 row lanes per block; row lane g adds partial rows g, g + 8, ... in order, the 8
// lane sums are then added in lane order.  mode 0: dadd[y, :] = sum over the nrows partials of sample y, component 2;
// mode 1: y = 0 / 1 -> dgamma / dbeta (+)= sum over all nrows partials of component y.
__global__ __launch_bounds__(256) void k_ln_bwd_fin(const float* __restrict__ part, int64_t nrows, int e, int mode, float* __restrict__ o0,
                                                    float* __restrict__ o1, int acc) {
    __shared__ float sh[8][32];
    const int cx = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;                     // e % 32 == 0: always inside the row
    const int64_t y = blockIdx.y;
    const int comp = mode == 0 ? 2 : (int)y;
    const int64_t base = mode == 0 ? y * nrows : 0;
    float t = 0.0f;
    for (int64_t i = rg; i < nrows; i += 8) t += part[((base + i) * 3 + comp) * e + c];
    sh[rg][cx] = t;
    __syncthreads();
    if (rg != 0) return;
    float tot = 0.0f;
#pragma unroll
    for (int g = 0; g < 8; ++g) tot += sh[g][cx];
    float* out = mode == 0 ? o0 + y * e : (y == 0 ? o0 : o1);
    out[c] = acc ? out[c] + tot : tot;
}

inline int ln_bps(int64_t nb, int64_t rps, int rpb) {
    int64_t want = (rps + rpb - 1) / rpb;
    int64_t cap = 1024 / nb;
    if (cap < 1) cap = 1;
    return (int)(want < cap ? want : cap);
}

// ------------------------------------------------------------------------------------------------------------------- patch gather
struct PatchGeo {
    int64_t B, C, S0, S1, S2, G0, G1, G2, K, Kp;
    int p0, p1, p2;
};

// thread per (token, 8 consecutive k): k = ((c * p0 + i0) * p1 + i1) * p2 + i2, token n = (g0 * G1 + g1) * G2 + g2 (vit.py:99-107)
template <typename T, bool TO_TOKENS>
__global__ __launch_bounds__(256) void k_patch(const float* __restrict__ img_in, float* __restrict__ img_out, const T* __restrict__ tok_in,
                                               T* __restrict__ tok_out, const float* __restrict__ bias, PatchGeo ge, int64_t total) {
    const int64_t ppr = ge.Kp / 8;
    const int pv = ge.p0 * ge.p1 * ge.p2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t piece = i % ppr, t = i / ppr;
        const int64_t n = t % (ge.G0 * ge.G1 * ge.G2), b = t / (ge.G0 * ge.G1 * ge.G2);
        const int64_t g2 = n % ge.G2, g1 = (n / ge.G2) % ge.G1, g0 = n / (ge.G2 * ge.G1);
        float v[8];
        if (!TO_TOKENS) {
            if (sizeof(T) == 2) {
                V16<bf16_raw>::ld(reinterpret_cast<const bf16_raw*>(tok_in) + t * ge.Kp + piece * 8, v);
            } else {
                float lo[4], hi[4];
                V16<float>::ld(reinterpret_cast<const float*>(tok_in) + t * ge.Kp + piece * 8, lo);
                V16<float>::ld(reinterpret_cast<const float*>(tok_in) + t * ge.Kp + piece * 8 + 4, hi);
#pragma unroll
                for (int q = 0; q < 4; ++q) { v[q] = lo[q]; v[4 + q] = hi[q]; }
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int64_t k = piece * 8 + q;
            if (k < ge.K) {
                const int c = (int)(k / pv), o = (int)(k % pv);
                const int i2 = o % ge.p2, i1 = (o / ge.p2) % ge.p1, i0 = o / (ge.p2 * ge.p1);
                const int64_t src = (((b * ge.C + c) * ge.S0 + g0 * ge.p0 + i0) * ge.S1 + g1 * ge.p1 + i1) * ge.S2 + g2 * ge.p2 + i2;
                if (TO_TOKENS) v[q] = img_in[src];
                else img_out[src] = bias ? v[q] + bias[c] : v[q];
            } else if (TO_TOKENS) {
                v[q] = 0.0f;
            }
        }
        if (TO_TOKENS) {
            if (sizeof(T) == 2) {
                V16<bf16_raw>::st(reinterpret_cast<bf16_raw*>(tok_out) + t * ge.Kp + piece * 8, v);
            } else {
                const float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
                V16<float>::st(reinterpret_cast<float*>(tok_out) + t * ge.Kp + piece * 8, lo);
                V16<float>::st(reinterpret_cast<float*>(tok_out) + t * ge.Kp + piece * 8 + 4, hi);
            }
        }
    }
}

// dbias[c] (+)= sum over (b, s) of x[b, c, s], two levels: block (j, c) walks the 256-element tiles j, j + nblk, ... of channel c's B
// contiguous rows (one division per tile, none per element), reduces them through a fixed LDS tree into ws[c][j]; the second kernel
// adds the nblk partials of a channel in order.
constexpr int CS_MAX_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_chan_sum_nchw(const float* __restrict__ x, float* __restrict__ ws, int64_t B, int64_t C, int64_t S) {
    __shared__ float sh[256];
    const int64_t c = blockIdx.y;
    const int64_t tps = (S + 255) / 256, tiles = B * tps;
    float t = 0.0f;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t b = tile / tps, s = (tile - b * tps) * 256 + threadIdx.x;
        if (s < S) t += x[(b * C + c) * S + s];
    }
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) ws[c * gridDim.x + blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(64) void k_chan_sum_fin(const float* __restrict__ ws, float* __restrict__ out, int64_t C, int nblk, int accumulate) {
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    float t = 0.0f;
    for (int j = 0; j < nblk; ++j) t += ws[c * nblk + j];
    out[c] = accumulate ? out[c] + t : t;
}
inline int chan_sum_blocks(int64_t batch, int64_t s) {
    const int64_t tiles = batch * ((s + 255) / 256);
    return (int)(tiles < CS_MAX_BLOCKS ? tiles : CS_MAX_BLOCKS);
}

bool patch_geo(PatchGeo& ge, int64_t batch, int64_t c, int dims, int64_t s0, int64_t s1, int64_t s2, int64_t p, int64_t kp) {
    if (batch <= 0 || c <= 0 || dims < 1 || dims > 3 || p <= 0 || s0 <= 0 || s1 <= 0 || s2 <= 0) return false;
    if ((dims < 3 && s0 != 1) || (dims < 2 && s1 != 1)) return false;
    ge.B = batch; ge.C = c; ge.S0 = s0; ge.S1 = s1; ge.S2 = s2;
    ge.p0 = dims >= 3 ? (int)p : 1; ge.p1 = dims >= 2 ? (int)p : 1; ge.p2 = (int)p;
    if (s0 % ge.p0 || s1 % ge.p1 || s2 % ge.p2) return false;
    ge.G0 = s0 / ge.p0; ge.G1 = s1 / ge.p1; ge.G2 = s2 / ge.p2;
    ge.K = c * ge.p0 * ge.p1 * ge.p2;
    ge.Kp = kp;
    return kp >= ge.K && kp % 32 == 0 && p <= 1024 && ge.K < (1LL << 31);
}

inline unsigned grid1d(int64_t total) {
    int64_t g = (total + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 262144 ? 262144 : g));
}

// ----------------------------------------------------------------------------------------------------------------- element-wise
// y = act(x + bias[c]) over rows of `cols` elements, 16 bytes per thread
template <typename T>
__global__ __launch_bounds__(256) void k_bias_act(const T* __restrict__ x, const float* __restrict__ bias, T* __restrict__ y, int64_t nvec,
                                                  int cols, int act) {
    constexpr int PE = V16<T>::PE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float v[PE];
        V16<T>::ld(x + i * PE, v);
        const int c0 = (int)((i * PE) % cols);
#pragma unroll
        for (int q = 0; q < PE; ++q) v[q] = act_any(bias ? v[q] + bias[c0 + q] : v[q], act);
        V16<T>::st(y + i * PE, v);
    }
}

// dx = dy * act'(x + bias[c])
template <typename T>
__global__ __launch_bounds__(256) void k_bias_act_bwd(const T* __restrict__ x, const float* __restrict__ bias, const T* __restrict__ dy,
                                                      T* __restrict__ dx, int64_t nvec, int cols, int act) {
    constexpr int PE = V16<T>::PE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float v[PE], d[PE];
        V16<T>::ld(x + i * PE, v);
        V16<T>::ld(dy + i * PE, d);
        const int c0 = (int)((i * PE) % cols);
#pragma unroll
        for (int q = 0; q < PE; ++q) d[q] *= dact_any(bias ? v[q] + bias[c0 + q] : v[q], act);
        V16<T>::st(dx + i * PE, d);
    }
}

// x[b, j] += pos[j]
template <typename T>
__global__ __launch_bounds__(256) void k_pos_add(T* __restrict__ x, const float* __restrict__ pos, int64_t nvec, int64_t mvec) {
    constexpr int PE = V16<T>::PE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float v[PE];
        V16<T>::ld(x + i * PE, v);
        const float* p = pos + (i % mvec) * PE;
#pragma unroll
        for (int q = 0; q < PE; ++q) v[q] += p[q];
        V16<T>::st(x + i * PE, v);
    }
}

// dpos[j] = sum_b dx[b, j], b ascending
template <typename T>
__global__ __launch_bounds__(256) void k_pos_add_bwd(const T* __restrict__ dx, float* __restrict__ dpos, int64_t batch, int64_t mvec) {
    constexpr int PE = V16<T>::PE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mvec; i += (int64_t)gridDim.x * blockDim.x) {
        float t[PE];
#pragma unroll
        for (int q = 0; q < PE; ++q) t[q] = 0.0f;
        for (int64_t b = 0; b < batch; ++b) {
            float v[PE];
            V16<T>::ld(dx + (b * mvec + i) * PE, v);
#pragma unroll
            for (int q = 0; q < PE; ++q) t[q] += v[q];
        }
#pragma unroll
        for (int q = 0; q < PE; ++q) dpos[i * PE + q] = t[q];
    }
}

bool ln_args_ok(int64_t rows, int64_t rps, int64_t e, bool has_add) {
    if (rows <= 0 || e < 32 || e > LN_MAX_E || e % 32 != 0) return false;
    if (has_add && (rps <= 0 || rows % rps != 0)) return false;
    return true;
}

template <typename T, int NV>
void launch_ln_fwd(const void* x, const float* add, const float* gamma, const float* beta, void* y, float* stats, int64_t rows, int64_t rps,
                   int e, const LnGeom& g, hipStream_t st) {
    const int64_t blocks = (rows + g.rpb - 1) / g.rpb;
    hipLaunchKernelGGL((k_ln_fwd<T, NV>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)x, add, gamma, beta, (T*)y, stats, rows, rps, e,
                       g.G, g.lgG);
}

template <typename T, int NV>
void launch_ln_bwd(const void* dy, const void* x, const float* add, const float* stats, const float* gamma, void* dx, int acc_dx, float* part,
                   int64_t nb, int bps, int64_t rps, int e, const LnGeom& g, hipStream_t st) {
    const dim3 grid((unsigned)bps, (unsigned)nb);
    if (add)
        hipLaunchKernelGGL((k_ln_bwd<T, NV, true>), grid, dim3(256), 0, st, (const T*)dy, (const T*)x, add, stats, gamma, (T*)dx, acc_dx, part,
                           rps, e, g.G, g.lgG);
    else
        hipLaunchKernelGGL((k_ln_bwd<T, NV, false>), grid, dim3(256), 0, st, (const T*)dy, (const T*)x, add, stats, gamma, (T*)dx, acc_dx,
                           part, rps, e, g.G, g.lgG);
}

}  // namespace

extern "C" int64_t rho_layernorm_max_dim(void) { return LN_MAX_E; }

extern "C" int rho_layernorm_fwd(const void* x, const float* add, const float* gamma, const float* beta, void* y, float* stats, int dtype,
                                 int64_t rows, int64_t rows_per_sample, int64_t e, void* stream) {
    if (!x || !gamma || !beta || !y || !stats) return RHO_E_ARG;
    if (dtype != RHO_F32 && dtype != RHO_BF16) return RHO_E_ARG;
    if (!ln_args_ok(rows, rows_per_sample, e, add != nullptr)) return RHO_E_SHAPE;
    const int64_t rps = add ? rows_per_sample : rows;
    const LnGeom g = ln_geom(e, dtype == RHO_BF16 ? 8 : 4);
    if ((rows + g.rpb - 1) / g.rpb > 0x7FFFFFFFLL) return RHO_E_SHAPE;
    hipStream_t st = as_stream(stream);
#define RHO_LN_CASE(NVV)                                                                                                          \
    case NVV:                                                                                                                     \
        if (dtype == RHO_F32) launch_ln_fwd<float, NVV>(x, add, gamma, beta, y, stats, rows, rps, (int)e, g, st);                 \
        else launch_ln_fwd<bf16_raw, NVV>(x, add, gamma, beta, y, stats, rows, rps, (int)e, g, st);                               \
        break;
    switch (g.NV) {
        RHO_LN_CASE(1)
        RHO_LN_CASE(2)
        RHO_LN_CASE(4)
        RHO_LN_CASE(8)
        default: return RHO_E_SHAPE;
    }
#undef RHO_LN_CASE
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t rho_layernorm_bwd_workspace_bytes(int64_t rows, int64_t rows_per_sample, int64_t e, int dtype, int has_add) {
    if ((dtype != RHO_F32 && dtype != RHO_BF16) || !ln_args_ok(rows, rows_per_sample, e, has_add != 0)) return 0;
    const int64_t rps = has_add ? rows_per_sample : rows, nb = rows / rps;
    const LnGeom g = ln_geom(e, dtype == RHO_BF16 ? 8 : 4);
    return nb * ln_bps(nb, rps, g.rpb) * 3 * e * (int64_t)sizeof(float);
}

extern "C" int rho_layernorm_bwd(const void* dy, const void* x, const float* add, const float* stats, const float* gamma, void* dx, int acc_dx,
                                 float* dadd, float* dgamma, float* dbeta, int acc_params, void* workspace, int64_t workspace_bytes,
                                 int dtype, int64_t rows, int64_t rows_per_sample, int64_t e, void* stream) {
    if (!dy || !x || !stats || !gamma || !dx || !dgamma || !dbeta || !workspace) return RHO_E_ARG;
    if (dtype != RHO_F32 && dtype != RHO_BF16) return RHO_E_ARG;
    if (dadd && !add) return RHO_E_ARG;
    if (!ln_args_ok(rows, rows_per_sample, e, add != nullptr)) return RHO_E_SHAPE;
    const int64_t rps = add ? rows_per_sample : rows, nb = rows / rps;
    if (nb > 65535) return RHO_E_SHAPE;
    const LnGeom g = ln_geom(e, dtype == RHO_BF16 ? 8 : 4);
    const int bps = ln_bps(nb, rps, g.rpb);
    if (workspace_bytes < nb * bps * 3 * e * (int64_t)sizeof(float)) return RHO_E_ARG;
    if ((int64_t)g.rpb * e > 8192) return RHO_E_SHAPE;
    float* part = (float*)workspace;
    hipStream_t st = as_stream(stream);
#define RHO_LN_CASE(NVV)                                                                                                          \
    case NVV:                                                                                                                     \
        if (dtype == RHO_F32) launch_ln_bwd<float, NVV>(dy, x, add, stats, gamma, dx, acc_dx, part, nb, bps, rps, (int)e, g, st); \
        else launch_ln_bwd<bf16_raw, NVV>(dy, x, add, stats, gamma, dx, acc_dx, part, nb, bps, rps, (int)e, g, st);               \
        break;
    switch (g.NV) {
        RHO_LN_CASE(1)
        RHO_LN_CASE(2)
        RHO_LN_CASE(4)
        RHO_LN_CASE(8)
        default: return RHO_E_SHAPE;
    }
#undef RHO_LN_CASE
    RHO_LAUNCH_CHECK();
    if (dadd) {
        hipLaunchKernelGGL(k_ln_bwd_fin, dim3((unsigned)(e / 32), (unsigned)nb), dim3(256), 0, st, part, (int64_t)bps, (int)e, 0, dadd,
                           (float*)nullptr, 0);
        RHO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ln_bwd_fin, dim3((unsigned)(e / 32), 2u), dim3(256), 0, st, part, nb * (int64_t)bps, (int)e, 1, dgamma, dbeta,
                       acc_params);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t rho_patchify_dbias_workspace_bytes(int64_t c) { return c > 0 ? c * CS_MAX_BLOCKS * (int64_t)sizeof(float) : 0; }

extern "C" int rho_patchify(const float* x, void* tokens, int dtype, int64_t batch, int64_t c, int dims, int64_t s0, int64_t s1, int64_t s2,
                            int64_t p, int64_t kp, float* dbias, int acc_dbias, float* dbias_ws, void* stream) {
    PatchGeo ge{};
    if (!x || !tokens || (dtype != RHO_F32 && dtype != RHO_BF16) || (dbias && !dbias_ws)) return RHO_E_ARG;
    if (dbias && c > 65535) return RHO_E_SHAPE;
    if (!patch_geo(ge, batch, c, dims, s0, s1, s2, p, kp)) return RHO_E_SHAPE;
    const int64_t total = batch * ge.G0 * ge.G1 * ge.G2 * (kp / 8);
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32)
        hipLaunchKernelGGL((k_patch<float, true>), dim3(grid1d(total)), dim3(256), 0, st, x, (float*)nullptr, (const float*)nullptr,
                           (float*)tokens, (const float*)nullptr, ge, total);
    else
        hipLaunchKernelGGL((k_patch<bf16_raw, true>), dim3(grid1d(total)), dim3(256), 0, st, x, (float*)nullptr, (const bf16_raw*)nullptr,
                           (bf16_raw*)tokens, (const float*)nullptr, ge, total);
    RHO_LAUNCH_CHECK();
    if (dbias) {
        const int nblk = chan_sum_blocks(batch, s0 * s1 * s2);
        hipLaunchKernelGGL(k_chan_sum_nchw, dim3((unsigned)nblk, (unsigned)c), dim3(256), 0, st, x, dbias_ws, batch, c, s0 * s1 * s2);
        RHO_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_chan_sum_fin, dim3((unsigned)((c + 63) / 64)), dim3(64), 0, st, dbias_ws, dbias, c, nblk, acc_dbias);
        RHO_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int rho_unpatchify(const void* tokens, const float* bias, float* out, int dtype, int64_t batch, int64_t c, int dims, int64_t s0,
                              int64_t s1, int64_t s2, int64_t p, int64_t kp, void* stream) {
    PatchGeo ge{};
    if (!tokens || !out || (dtype != RHO_F32 && dtype != RHO_BF16)) return RHO_E_ARG;
    if (!patch_geo(ge, batch, c, dims, s0, s1, s2, p, kp)) return RHO_E_SHAPE;
    const int64_t total = batch * ge.G0 * ge.G1 * ge.G2 * (kp / 8);
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32)
        hipLaunchKernelGGL((k_patch<float, false>), dim3(grid1d(total)), dim3(256), 0, st, (const float*)nullptr, out, (const float*)tokens,
                           (float*)nullptr, bias, ge, total);
    else
        hipLaunchKernelGGL((k_patch<bf16_raw, false>), dim3(grid1d(total)), dim3(256), 0, st, (const float*)nullptr, out,
                           (const bf16_raw*)tokens, (bf16_raw*)nullptr, bias, ge, total);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_bias_act(const void* x, const float* bias, void* y, int dtype, int64_t rows, int64_t cols, int act, void* stream) {
    if (!x || !y || rows <= 0 || cols <= 0 || cols % 8 != 0 || cols >= (1LL << 31) || act < 0 || act > 6) return RHO_E_ARG;
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32) {
        const int64_t nvec = rows * cols / 4;
        hipLaunchKernelGGL(k_bias_act<float>, dim3(grid1d(nvec)), dim3(256), 0, st, (const float*)x, bias, (float*)y, nvec, (int)cols, act);
    } else if (dtype == RHO_BF16) {
        const int64_t nvec = rows * cols / 8;
        hipLaunchKernelGGL(k_bias_act<bf16_raw>, dim3(grid1d(nvec)), dim3(256), 0, st, (const bf16_raw*)x, bias, (bf16_raw*)y, nvec, (int)cols,
                           act);
    } else {
        return RHO_E_ARG;
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_bias_act_bwd(const void* x, const float* bias, const void* dy, void* dx, int dtype, int64_t rows, int64_t cols, int act,
                                void* stream) {
    if (!x || !dy || !dx || rows <= 0 || cols <= 0 || cols % 8 != 0 || cols >= (1LL << 31) || act < 0 || act > 6) return RHO_E_ARG;
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32) {
        const int64_t nvec = rows * cols / 4;
        hipLaunchKernelGGL(k_bias_act_bwd<float>, dim3(grid1d(nvec)), dim3(256), 0, st, (const float*)x, bias, (const float*)dy, (float*)dx,
                           nvec, (int)cols, act);
    } else if (dtype == RHO_BF16) {
        const int64_t nvec = rows * cols / 8;
        hipLaunchKernelGGL(k_bias_act_bwd<bf16_raw>, dim3(grid1d(nvec)), dim3(256), 0, st, (const bf16_raw*)x, bias, (const bf16_raw*)dy,
                           (bf16_raw*)dx, nvec, (int)cols, act);
    } else {
        return RHO_E_ARG;
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_pos_add(void* x, const float* pos, int dtype, int64_t batch, int64_t m, void* stream) {
    if (!x || !pos || batch <= 0 || m <= 0 || m % 8 != 0) return RHO_E_ARG;
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32)
        hipLaunchKernelGGL(k_pos_add<float>, dim3(grid1d(batch * m / 4)), dim3(256), 0, st, (float*)x, pos, batch * m / 4, m / 4);
    else if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_pos_add<bf16_raw>, dim3(grid1d(batch * m / 8)), dim3(256), 0, st, (bf16_raw*)x, pos, batch * m / 8, m / 8);
    else
        return RHO_E_ARG;
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_pos_add_bwd(const void* dx, float* dpos, int dtype, int64_t batch, int64_t m, void* stream) {
    if (!dx || !dpos || batch <= 0 || m <= 0 || m % 8 != 0) return RHO_E_ARG;
    hipStream_t st = as_stream(stream);
    if (dtype == RHO_F32)
        hipLaunchKernelGGL(k_pos_add_bwd<float>, dim3(grid1d(m / 4)), dim3(256), 0, st, (const float*)dx, dpos, batch, m / 4);
    else if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_pos_add_bwd<bf16_raw>, dim3(grid1d(m / 8)), dim3(256), 0, st, (const bf16_raw*)dx, dpos, batch, m / 8);
    else
        return RHO_E_ARG;
    RHO_LAUNCH_CHECK();
    return 0;
}
