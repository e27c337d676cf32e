// Gaussian line profiles of the reference's SpectroscopyDataset for a whole batch (rho_diffusion/data/spectroscopy.py:111-189:
// simulate_lineprofile :142-189 = sum over the lines inside the grid's range of I * exp(-(f - c)^2 / (2 w^2)), and :130 the division
// by the row maximum).  The reference builds a float64 [lines, grid] temporary per item on the host; a line of width ~1 MHz reaches
// a few dozen of the default grid's 50 000 points, so almost every exp of that temporary is zero.
//
// The lines of all items are resident in CSR form (centers / intensity [total], offsets [N + 1]), sorted by centre inside an item.  A
// workgroup owns one item and one tile of LP_TILE consecutive grid points.  It finds the sub-range of the item's lines whose centres
// lie within R of the tile by binary search, stages (c, I, -log2e / (2 w^2)) chunks of it in LDS, and every wave walks the chunk for
// its own LP_WAVE_PTS consecutive points (LP_ACC per lane in registers), skipping the lines out of its own reach.  A line is out
// of reach only where its exponent is below -87 at every point: its term there is under 1.7e-38 * I, and I <= 1e-2.
// R = 13.25 w >= w * sqrt(2 * 87) with the item's largest width.
//
// Float32 throughout: d = f - c, d * d, one multiply by the per-line constant, v_exp_f32, one multiply-add.  v_exp_f32 issues in 8
// cycles, the other four in 4 each: 24 cycles per (line, 64 points), a third of it the exponential - the reach test is what pays.
//
// The row maximum is folded by the same launch: a non-negative float's bit pattern orders as an unsigned integer, so each workgroup
// ends with one atomicMax on the bits (a NaN sum has the largest pattern and wins, as numpy's max propagates it).  A second,
// bandwidth-bound launch divides.  Nothing waits for another workgroup.
#include "common.h"

#include <cmath>

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_ACC = 4;                                   // grid points per lane
constexpr int LP_WAVE_PTS = 64 * LP_ACC;                    // consecutive grid points per wave
constexpr int LP_TILE = LP_WAVES * LP_WAVE_PTS;             // grid points per workgroup (1024)
constexpr int LP_CHUNK = 512;                               // lines staged per pass (8 KB of LDS)
constexpr float LP_REACH = 13.25f;                          // > sqrt(2 * 87) = 13.191: exponent < -87 beyond REACH * w
constexpr float LP_NLOG2E_HALF = -0.72134752044448170f;     // -log2(e) / 2

struct LineK {
    const float* grid;
    const float* centers;
    const float* intensity;
    const float* line_width;    // optional [total]
    const int64_t* offsets;
    const int64_t* index;
    const float* widths;        // [batch]
    float* out;
    unsigned int* rowmax;       // optional [batch]: bits of the row maximum
    int32_t* err_flag;
    int64_t n, total, g;
};

// first line of [lo, hi) whose centre is >= x (NaN centres sort last and count as +inf)
__device__ __forceinline__ int64_t lower_line(const float* __restrict__ c, int64_t lo, int64_t hi, float x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (c[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// first line of [lo, hi) whose centre is > x
__device__ __forceinline__ int64_t upper_line(const float* __restrict__ c, int64_t lo, int64_t hi, float x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (c[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// item of batch row b and its line range, or false (flag set) when the index or the offsets are out of range: uniform per workgroup
__device__ __forceinline__ bool item_range(const LineK& p, int b, int64_t& lo, int64_t& hi) {
    const int64_t item = p.index[b];
    if (item < 0 || item >= p.n) {
        if (threadIdx.x == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 4);
        return false;
    }
    lo = p.offsets[item];
    hi = p.offsets[item + 1];
    if (lo < 0 || hi < lo || hi > p.total) {
        if (threadIdx.x == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 8);
        return false;
    }
    return true;
}

__global__ __launch_bounds__(LP_THREADS) void k_line_profile(const LineK p) {
    __shared__ float4 stage[LP_CHUNK];                      // (c, I, -log2e / (2 w^2), unused)
    __shared__ float red[LP_WAVES];
    const int b = blockIdx.y;
    int64_t lo, hi;
    if (!item_range(p, b, lo, hi)) return;                  // before any barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t G = p.g;
    const int64_t t0 = (int64_t)blockIdx.x * LP_TILE, t1 = min(t0 + LP_TILE, G) - 1;          // the tile's points, inclusive
    const float ga = p.grid[0], gb = p.grid[G - 1];
    const float gmin = fminf(ga, gb), gmax = fmaxf(ga, gb);                                   // the grid is monotone
    const float ta = p.grid[t0], tb = p.grid[t1];

    // the window's width: the item's width, or its largest line width
    float wmax = p.widths[b];
    if (p.line_width != nullptr) {
        float m = 0.0f;
        for (int64_t k = lo + threadIdx.x; k < hi; k += LP_THREADS) m = fmaxf(m, fabsf(p.line_width[k]));
        m = wave_max(m);
        if (lane == 0) red[wave] = m;
        __syncthreads();
        wmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
    wmax = fabsf(wmax);
    const float wi = p.widths[b];
    const float k2_item = LP_NLOG2E_HALF / (wi * wi);
    const float R = LP_REACH * wmax;
    // lines inside the grid's range (inclusive, spectroscopy.py:179-181) and within R of the tile.  tlo / thi round to nearest: two
    // ulps outwards keep the reach; LP_REACH's margin over sqrt(174) covers the rest.
    float tlo = fminf(ta, tb) - R, thi = fmaxf(ta, tb) + R;
    tlo -= fabsf(tlo) * 2.4e-7f;
    thi += fabsf(thi) * 2.4e-7f;
    const int64_t k0 = lower_line(p.centers, lo, hi, fmaxf(tlo, gmin));
    const int64_t k1 = upper_line(p.centers, k0, hi, fminf(thi, gmax));

    // this wave's points: w0 + j * 64 + lane
    const int64_t w0 = t0 + (int64_t)wave * LP_WAVE_PTS;
    const bool live = w0 < G;
    float f[LP_ACC], acc[LP_ACC];
#pragma unroll
    for (int j = 0; j < LP_ACC; ++j) {
        f[j] = p.grid[min(w0 + j * 64 + lane, G - 1)];
        acc[j] = 0.0f;
    }
    float wlo = 0.0f, whi = 0.0f;
    if (live) {
        const float wa = p.grid[w0], wb = p.grid[min(w0 + LP_WAVE_PTS, G) - 1];
        wlo = fminf(wa, wb) - R;
        whi = fmaxf(wa, wb) + R;
        wlo -= fabsf(wlo) * 2.4e-7f;
        whi += fabsf(whi) * 2.4e-7f;
    }

    for (int64_t c0 = k0; c0 < k1; c0 += LP_CHUNK) {
        const int nl = (int)min((int64_t)LP_CHUNK, k1 - c0);
        __syncthreads();                                    // the previous chunk (and red[]) has been read
        for (int i = threadIdx.x; i < nl; i += LP_THREADS) {
            float k2 = k2_item;
            if (p.line_width != nullptr) {
                const float w = p.line_width[c0 + i];
                k2 = LP_NLOG2E_HALF / (w * w);
            }
            stage[i] = make_float4(p.centers[c0 + i], p.intensity[c0 + i], k2, 0.0f);
        }
        __syncthreads();
        if (live) {
            for (int i = 0; i < nl; ++i) {
                const float4 l = stage[i];                  // one address per wave: a broadcast read
                if (l.x < wlo || l.x > whi) continue;       // uniform over the wave
#pragma unroll
                for (int j = 0; j < LP_ACC; ++j) {
                    const float d = f[j] - l.x;
                    acc[j] = fmaf(l.y, __builtin_amdgcn_exp2f(d * d * l.z), acc[j]);
                }
            }
        }
    }

    unsigned int mbits = 0u;
#pragma unroll
    for (int j = 0; j < LP_ACC; ++j) {
        const int64_t g = w0 + j * 64 + lane;
        if (g < G) {
            p.out[(int64_t)b * G + g] = acc[j];
            mbits = max(mbits, __float_as_uint(acc[j]));
        }
    }
    if (p.rowmax != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mbits = max(mbits, (unsigned int)__shfl_xor((int)mbits, o, 64));
        __syncthreads();                                    // red[] may still be read by a slower wave
        if (lane == 0) red[wave] = __uint_as_float(mbits);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int m = __float_as_uint(red[0]);
#pragma unroll
            for (int k = 1; k < LP_WAVES; ++k) m = max(m, __float_as_uint(red[k]));
            atomicMax(p.rowmax + b, m);
        }
    }
}

// out[b, :] /= rowmax[b] (spectroscopy.py:130).  IEEE division: the maximum itself becomes exactly 1, an all-zero row 0 / 0 = NaN.
__global__ __launch_bounds__(LP_THREADS) void k_line_profile_normalise(const LineK p) {
    const int b = blockIdx.y;
    const int64_t item = p.index[b];
    if (item < 0 || item >= p.n) return;                    // the profile launch has set the flag and written nothing
    const float m = __uint_as_float(p.rowmax[b]);
    const int64_t t0 = (int64_t)blockIdx.x * LP_TILE;
    float* row = p.out + (int64_t)b * p.g;
#pragma unroll
    for (int j = 0; j < LP_ACC; ++j) {
        const int64_t g = t0 + j * LP_THREADS + threadIdx.x;
        if (g < p.g) row[g] = row[g] / m;
    }
}

}  // namespace

extern "C" int rho_line_profile(const float* grid, int64_t grid_size, const float* centers, const float* intensity, const float* line_width,
                                int64_t total, const int64_t* offsets, int64_t n_items, const int64_t* index, const float* widths,
                                int64_t batch, float* out, float* rowmax, int32_t* err_flag, void* stream) {
    if (!grid || !offsets || !index || !widths || !out) return RHO_E_ARG;
    if (total < 0 || (total > 0 && (!centers || !intensity))) return RHO_E_ARG;
    if (grid_size <= 0 || n_items <= 0 || batch <= 0 || batch > 65535) return RHO_E_ARG;
    const int64_t tiles = (grid_size + LP_TILE - 1) / LP_TILE;
    if (tiles > 0x7fffffff) return RHO_E_SHAPE;
    LineK p{};
    p.grid = grid;
    p.centers = centers;
    p.intensity = intensity;
    p.line_width = line_width;
    p.offsets = offsets;
    p.index = index;
    p.widths = widths;
    p.out = out;
    p.rowmax = reinterpret_cast<unsigned int*>(rowmax);
    p.err_flag = err_flag;
    p.n = n_items;
    p.total = total;
    p.g = grid_size;
    hipStream_t st = as_stream(stream);
    const dim3 blocks((unsigned)tiles, (unsigned)batch);
    if (rowmax != nullptr) {
        const hipError_t e = hipMemsetAsync(rowmax, 0, (size_t)batch * sizeof(float), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_line_profile, blocks, dim3(LP_THREADS), 0, st, p);
    RHO_LAUNCH_CHECK();
    if (rowmax != nullptr) {
        hipLaunchKernelGGL(k_line_profile_normalise, blocks, dim3(LP_THREADS), 0, st, p);
        RHO_LAUNCH_CHECK();
    }
    return 0;
}
