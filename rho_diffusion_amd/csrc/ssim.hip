// Structural similarity (SSIM) of two float32 fields [B, C, *spatial] with 1, 2 or 3 spatial dimensions: the metric of torchmetrics'
// StructuralSimilarityIndexMeasure, the package the reference's pipelines take their metrics from (abstract_diffusion.py:31,79), over
// the windows that lie wholly inside the field.  A field is always handled as (D, H, W): missing leading dimensions have size 1 and
// the window {1.0}, whose one-tap "sum" 1.0 * x is exact.
//
//   rho_ssim_range   min and max of both arrays in one pass (ordered partials) -> R = max(max p - min p, max t - min t) on the device
//   rho_ssim         five windowed moments per voxel, the index, its per-sample mean; optionally the map
//
// Arithmetic (tests/test_gpu_ssim.py counts its roundings from this text).  All of it float32, contraction off, fmaf where written:
//   s       = clamp(target[b, c, 0, .., 0])                  one constant per (sample, channel) slab
//   a       = clamp(p) - s,  b = clamp(t) - s                1 rounding each
//   x       = a, b, a * a, b * b, a * b                      1 rounding for each product
//   window  : acc = g[0] * x[0]; acc = fmaf(g[j], x[j], acc) for j = 1 .. k - 1 (taps ascending)   k roundings
//   passes  : along W, then along H, then along D            k_w + k_h + k_d roundings per moment
//   index   : the expression of ssim_index() below
// The means are mu_p = s + W[a], mu_t = s + W[b]; variances and covariance come from the shifted moments (they are shift-invariant):
// without the shift W[p^2] - mu_p^2 loses a field of small contrast on a large offset.  One expression per step serves the 16-byte and
// the scalar loads and every window form, so all of them give the same bits.
//
// Kernel.  A workgroup of 512 threads owns SSIM_TH x SSIM_TW = 16 x 32 output columns of one slab and SSIM_TD = 16 output planes, and
// marches along D over 16 + k_d - 1 input planes.  Per input plane: the shifted tile plus halo of both inputs goes to LDS (global
// loads of the next plane are issued before the passes of this one and stored after them); the W pass writes five moments per (row,
// column) to LDS; the H pass reads k_h rows of them per thread; the D pass is a shift register of k_d pending outputs per moment in
// the thread's registers.  A finished index goes into the thread's float64 sum and, if asked for, to the map; nothing else is written.
// The workgroup's sum is one float64 partial; k_ssim_final folds the partials of a sample in an order fixed by the shapes, divides by
// the window count and reduces over the batch.  No atomics: two runs give the same bits.
//
// Forms: window lengths (k_d, k_h, k_w) = (11, 11, 11), (1, 11, 11) and (1, 1, 11) - the default Gaussian in 3, 2 and 1 dimensions -
// are compiled with constant trip counts; every other window takes the form with runtime lengths (<= SSIM_MAXW).  Each has a 16-byte
// loader (both bases 16-byte aligned and W % 4 == 0) and a scalar one.
#include "common.h"

namespace {

constexpr int SSIM_MAXW = 15;                               // longest window per dimension
constexpr int SSIM_TD = 16, SSIM_TH = 16, SSIM_TW = 32;     // output planes / rows / columns per workgroup
constexpr int SSIM_THREADS = SSIM_TH * SSIM_TW;             // one thread per output column
constexpr int SSIM_ROWS = SSIM_TH + SSIM_MAXW - 1;          // staged rows
constexpr int SSIM_LD = 48;                                 // staged row stride >= SSIM_TW + SSIM_MAXW - 1 = 46, whole quads
constexpr int SSIM_SCALAR_PER_THREAD = (SSIM_ROWS * (SSIM_TW + SSIM_MAXW - 1) + SSIM_THREADS - 1) / SSIM_THREADS;   // 3
constexpr int SSIM_RANGE_BLOCKS = 1024;
static_assert(SSIM_ROWS * (SSIM_LD / 4) <= SSIM_THREADS, "one quad per thread and array");

struct SsimK {
    const float* p;
    const float* t;
    const float* gd;
    const float* gh;
    const float* gw;
    int kd, kh, kw;
    int D, H, W, Do, Ho, Wo;
    int nch, nth, ntw;
    const float* range_dev;
    float range;
    int clamp;
    float lo, hi, k1, k2;
    float* map;
    double* part;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float ssim_clamp(float v, int clamp, float lo, float hi) { return clamp ? fminf(fmaxf(v, lo), hi) : v; }

__device__ __forceinline__ float ssim_shift(float v, int clamp, float lo, float hi, float s) {
#pragma clang fp contract(off)
    return ssim_clamp(v, clamp, lo, hi) - s;
}

// m = {W[a], W[b], W[a a], W[b b], W[a b]} on the shifted data, s the shift
__device__ __forceinline__ float ssim_index(const float (&m)[5], float s, float c1, float c2) {
#pragma clang fp contract(off)
    const float mu_p = s + m[0], mu_t = s + m[1];
    const float s_pp = fmaxf(m[2] - m[0] * m[0], 0.0f);
    const float s_tt = fmaxf(m[3] - m[1] * m[1], 0.0f);
    const float s_pt = m[4] - m[0] * m[1];
    const float num = ((2.0f * mu_p) * mu_t + c1) * (2.0f * s_pt + c2);
    const float den = ((mu_p * mu_p + mu_t * mu_t) + c1) * ((s_pp + s_tt) + c2);
    return num / den;
}

template <int KD, int KH, int KW, bool VEC>
__global__ __launch_bounds__(SSIM_THREADS) void k_ssim(const SsimK a) {
#pragma clang fp contract(off)
    __shared__ float sa[SSIM_ROWS * SSIM_LD], sb[SSIM_ROWS * SSIM_LD];
    __shared__ float sm[5][SSIM_ROWS * SSIM_TW];
    __shared__ float sg[3][SSIM_MAXW + 1];
    __shared__ double red[SSIM_THREADS / 64];
    constexpr int RK = KD ? KD : SSIM_MAXW;
    const int tid = threadIdx.x;
    const int kd = KD ? KD : a.kd, kh = KH ? KH : a.kh, kw = KW ? KW : a.kw;
    // a NULL window is {1.0}: a dimension the field does not have.  The constant-length forms keep their taps in registers (uniform
    // loads), the runtime form reads them from LDS.
    if (tid < kd) sg[0][tid] = a.gd ? a.gd[tid] : 1.0f;
    if (tid < kh) sg[1][tid] = a.gh ? a.gh[tid] : 1.0f;
    if (tid < kw) sg[2][tid] = a.gw ? a.gw[tid] : 1.0f;
    float wd[KD ? KD : 1], wh[KH ? KH : 1], ww[KW ? KW : 1];
#pragma unroll
    for (int j = 0; j < KD; ++j) wd[j] = a.gd ? a.gd[j] : 1.0f;
#pragma unroll
    for (int j = 0; j < KH; ++j) wh[j] = a.gh ? a.gh[j] : 1.0f;
#pragma unroll
    for (int j = 0; j < KW; ++j) ww[j] = a.gw ? a.gw[j] : 1.0f;
    auto tap_d = [&](int j) { return KD ? wd[j] : sg[0][j]; };
    auto tap_h = [&](int j) { return KH ? wh[j] : sg[1][j]; };
    auto tap_w = [&](int j) { return KW ? ww[j] : sg[2][j]; };

    const int per_plane = a.nth * a.ntw, per_slab = a.nch * per_plane;
    const int64_t slab = blockIdx.x / per_slab;
    int rem = (int)(blockIdx.x - slab * per_slab);
    const int ch = rem / per_plane;
    rem -= ch * per_plane;
    const int th = rem / a.ntw, tw = rem - th * a.ntw;
    const int z0 = ch * SSIM_TD, y0 = th * SSIM_TH, x0 = tw * SSIM_TW;
    const int nzi = min(SSIM_TD, a.Do - z0) + kd - 1;                       // input planes of this workgroup
    const int rows = min(SSIM_TH + kh - 1, a.H - y0), cols = min(SSIM_TW + kw - 1, a.W - x0);      // staged, all inside the field
    const int hval = min(SSIM_TH, a.Ho - y0), wval = min(SSIM_TW, a.Wo - x0);                       // outputs of this tile
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t first = ((slab * a.D + z0) * a.H + y0) * (int64_t)a.W + x0;
    const float* pb = a.p + first;
    const float* tb = a.t + first;
    const float s = ssim_clamp(a.t[slab * a.D * plane], a.clamp, a.lo, a.hi);
    const float R = a.range_dev ? a.range_dev[0] : a.range;
    const float c1 = (a.k1 * R) * (a.k1 * R), c2 = (a.k2 * R) * (a.k2 * R);

    // staging: VEC one quad per thread and array (a quad that starts inside the field ends inside it: W % 4 == 0, x0 % 4 == 0)
    const int nq = (cols + 3) >> 2;
    const int n_items = VEC ? rows * nq : rows * cols, per_row = VEC ? nq : cols;
    constexpr int NPF = VEC ? 1 : SSIM_SCALAR_PER_THREAD;
    float4 pq = make_float4(0.0f, 0.0f, 0.0f, 0.0f), tq = pq;
    float ps[NPF], ts[NPF];
    int64_t goff[NPF];
    int loff[NPF];                                                // offsets inside a plane / inside the staged tile
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
        const int e = tid + u * SSIM_THREADS;
        const int row = e / per_row, c = (e - row * per_row) * (VEC ? 4 : 1);
        goff[u] = e < n_items ? (int64_t)row * a.W + c : -1;
        loff[u] = row * SSIM_LD + c;
        ps[u] = ts[u] = 0.0f;
    }
    auto fetch = [&](int zi) {
        const float* pz = pb + zi * plane;
        const float* tz = tb + zi * plane;
        if (VEC) {
            if (goff[0] >= 0) {
                pq = *reinterpret_cast<const float4*>(pz + goff[0]);
                tq = *reinterpret_cast<const float4*>(tz + goff[0]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NPF; ++u)
                if (goff[u] >= 0) { ps[u] = pz[goff[u]]; ts[u] = tz[goff[u]]; }
        }
    };
    auto stage = [&]() {
        if (VEC) {
            if (goff[0] >= 0) {
                float* da = sa + loff[0];
                float* db = sb + loff[0];
                da[0] = ssim_shift(pq.x, a.clamp, a.lo, a.hi, s); da[1] = ssim_shift(pq.y, a.clamp, a.lo, a.hi, s);
                da[2] = ssim_shift(pq.z, a.clamp, a.lo, a.hi, s); da[3] = ssim_shift(pq.w, a.clamp, a.lo, a.hi, s);
                db[0] = ssim_shift(tq.x, a.clamp, a.lo, a.hi, s); db[1] = ssim_shift(tq.y, a.clamp, a.lo, a.hi, s);
                db[2] = ssim_shift(tq.z, a.clamp, a.lo, a.hi, s); db[3] = ssim_shift(tq.w, a.clamp, a.lo, a.hi, s);
            }
        } else {
#pragma unroll
            for (int u = 0; u < NPF; ++u)
                if (goff[u] >= 0) {
                    sa[loff[u]] = ssim_shift(ps[u], a.clamp, a.lo, a.hi, s);
                    sb[loff[u]] = ssim_shift(ts[u], a.clamp, a.lo, a.hi, s);
                }
        }
    };

    const int oh = tid / SSIM_TW, ow = tid % SSIM_TW;
    const bool live = oh < hval && ow < wval;
    const int64_t map0 = ((slab * a.Do + z0) * a.Ho + (y0 + oh)) * (int64_t)a.Wo + (x0 + ow);
    const int64_t map_plane = (int64_t)a.Ho * a.Wo;
    float ring[5][RK];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int j = 0; j < RK; ++j) ring[m][j] = 0.0f;
    double acc = 0.0;

    fetch(0);
    for (int zi = 0; zi < nzi; ++zi) {
        stage();
        __syncthreads();                                  // the tile is staged; the last plane's H pass is over
        if (zi + 1 < nzi) fetch(zi + 1);
        // ---- W pass: five moments per (staged row, output column)
        for (int it = tid; it < rows * SSIM_TW; it += SSIM_THREADS) {
            const int row = it / SSIM_TW, col = it % SSIM_TW;
            if (col < wval) {
                const float* xa = sa + row * SSIM_LD + col;
                const float* xb = sb + row * SSIM_LD + col;
                float g = tap_w(0), u = xa[0], v = xb[0];
                float m0 = g * u, m1 = g * v, m2 = g * (u * u), m3 = g * (v * v), m4 = g * (u * v);
#pragma unroll
                for (int j = 1; j < (KW ? KW : kw); ++j) {
                    g = tap_w(j); u = xa[j]; v = xb[j];
                    m0 = fmaf(g, u, m0);
                    m1 = fmaf(g, v, m1);
                    m2 = fmaf(g, u * u, m2);
                    m3 = fmaf(g, v * v, m3);
                    m4 = fmaf(g, u * v, m4);
                }
                sm[0][it] = m0; sm[1][it] = m1; sm[2][it] = m2; sm[3][it] = m3; sm[4][it] = m4;
            }
        }
        __syncthreads();                                  // the moments of this plane are in LDS; sa / sb may be overwritten
        if (live) {
            // ---- H pass
            float v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = tap_h(0) * sm[m][tid];
#pragma unroll
            for (int j = 1; j < (KH ? KH : kh); ++j) {
                const float g = tap_h(j);
#pragma unroll
                for (int m = 0; m < 5; ++m) v[m] = fmaf(g, sm[m][tid + j * SSIM_TW], v[m]);
            }
            // ---- D pass: ring[m][j] holds the output that has received taps 0 .. j
#pragma unroll
            for (int j = RK - 1; j >= 1; --j)
                if (KD || j < kd) {
                    const float g = tap_d(j);
#pragma unroll
                    for (int m = 0; m < 5; ++m) ring[m][j] = fmaf(g, v[m], ring[m][j - 1]);
                }
            {
                const float g = tap_d(0);
#pragma unroll
                for (int m = 0; m < 5; ++m) ring[m][0] = g * v[m];
            }
            if (zi >= kd - 1) {
                float mo[5];
                if (KD) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) mo[m] = ring[m][RK - 1];
                } else {
#pragma unroll
                    for (int m = 0; m < 5; ++m) mo[m] = ring[m][0];
#pragma unroll
                    for (int j = 1; j < RK; ++j)
                        if (j == kd - 1) {
#pragma unroll
                            for (int m = 0; m < 5; ++m) mo[m] = ring[m][j];
                        }
                }
                const float S = ssim_index(mo, s, c1, c2);
                acc += (double)S;
                if (a.map) a.map[map0 + (zi - (kd - 1)) * map_plane] = S;
            }
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double tot = red[0];
#pragma unroll
        for (int w = 1; w < SSIM_THREADS / 64; ++w) tot += red[w];
        a.part[blockIdx.x] = tot;
    }
}

// One workgroup of 16 waves.  A wave takes samples w, w + 16, ..: lane l adds partials l, l + 64, .. of the sample, the lanes fold by a
// butterfly; per_sample[b] = sum / count.  Then wave 0 adds the per-sample values (float64, kept in `sval`) the same way.
__global__ __launch_bounds__(1024) void k_ssim_final(const double* __restrict__ part, int batch, int64_t parts_per_sample, double count,
                                                     double* __restrict__ sval, float* __restrict__ per_sample, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < batch; b += 16) {
        const double* p = part + (int64_t)b * parts_per_sample;
        double acc = 0.0;
        for (int64_t i = lane; i < parts_per_sample; i += 64) acc += p[i];
        acc = wave_sum_d(acc);
        if (lane == 0) {
            const double v = acc / count;
            sval[b] = v;
            per_sample[b] = (float)v;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double acc = 0.0;
        for (int b = lane; b < batch; b += 64) acc += sval[b];
        acc = wave_sum_d(acc);
        if (lane == 0) {
            out[0] = (float)(acc / (double)batch);
            out[1] = (float)acc;
        }
    }
}

// ----------------------------------------------------------------------------- data_range = None
__global__ __launch_bounds__(256) void k_ssim_range_part(const float* __restrict__ a, const float* __restrict__ b, int64_t n, int vec,
                                                         float* __restrict__ partials) {
    __shared__ float red[4][4];
    float amn = INFINITY, amx = -INFINITY, bmn = INFINITY, bmx = -INFINITY;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        for (int64_t i = tid; i < n4; i += nthr) {
            const float4 p = a4[i], t = b4[i];
            amn = fminf(fminf(amn, fminf(p.x, p.y)), fminf(p.z, p.w));
            amx = fmaxf(fmaxf(amx, fmaxf(p.x, p.y)), fmaxf(p.z, p.w));
            bmn = fminf(fminf(bmn, fminf(t.x, t.y)), fminf(t.z, t.w));
            bmx = fmaxf(fmaxf(bmx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nthr) {
        const float p = a[i], t = b[i];
        amn = fminf(amn, p); amx = fmaxf(amx, p);
        bmn = fminf(bmn, t); bmx = fmaxf(bmx, t);
    }
    amn = -wave_max(-amn); amx = wave_max(amx);
    bmn = -wave_max(-bmn); bmx = wave_max(bmx);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = amn; red[1][w] = amx; red[2][w] = bmn; red[3][w] = bmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[4 * blockIdx.x + 0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        partials[4 * blockIdx.x + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        partials[4 * blockIdx.x + 2] = fminf(fminf(red[2][0], red[2][1]), fminf(red[2][2], red[2][3]));
        partials[4 * blockIdx.x + 3] = fmaxf(fmaxf(red[3][0], red[3][1]), fmaxf(red[3][2], red[3][3]));
    }
}
__global__ __launch_bounds__(64) void k_ssim_range_final(const float* __restrict__ partials, int np, float* __restrict__ out) {
    float amn = INFINITY, amx = -INFINITY, bmn = INFINITY, bmx = -INFINITY;
    for (int i = threadIdx.x; i < np; i += 64) {
        amn = fminf(amn, partials[4 * i]);
        amx = fmaxf(amx, partials[4 * i + 1]);
        bmn = fminf(bmn, partials[4 * i + 2]);
        bmx = fmaxf(bmx, partials[4 * i + 3]);
    }
    amn = -wave_max(-amn); amx = wave_max(amx);
    bmn = -wave_max(-bmn); bmx = wave_max(bmx);
    if (threadIdx.x == 0) out[0] = fmaxf(amx - amn, bmx - bmn);
}

struct SsimGeom {
    int64_t d[3], k[3], o[3];         // sizes, windows, outputs as (D, H, W)
    int64_t nch, nth, ntw, groups;    // workgroups per slab dimension, in all
};

// RHO_E_* or 0
int ssim_geometry(int64_t batch, int64_t channels, int ndim, const int64_t* sizes, const int64_t* window_sizes, SsimGeom* g) {
    if (!sizes || !window_sizes || ndim < 1 || ndim > 3 || batch < 1 || channels < 1) return RHO_E_ARG;
    for (int i = 0; i < 3; ++i) { g->d[i] = 1; g->k[i] = 1; }
    for (int i = 0; i < ndim; ++i) { g->d[3 - ndim + i] = sizes[i]; g->k[3 - ndim + i] = window_sizes[i]; }
    int64_t vol = 1;
    for (int i = 0; i < 3; ++i) {
        if (g->k[i] < 1 || g->k[i] > SSIM_MAXW || (g->k[i] & 1) == 0) return RHO_E_SHAPE;
        if (g->d[i] < g->k[i] || g->d[i] > 0x7FFFFFFF) return RHO_E_SHAPE;
        g->o[i] = g->d[i] - g->k[i] + 1;
        vol *= g->d[i];
        if (vol > ((int64_t)1 << 40)) return RHO_E_SHAPE;
    }
    g->nch = (g->o[0] + SSIM_TD - 1) / SSIM_TD;
    g->nth = (g->o[1] + SSIM_TH - 1) / SSIM_TH;
    g->ntw = (g->o[2] + SSIM_TW - 1) / SSIM_TW;
    const int64_t per_slab = g->nch * g->nth * g->ntw;
    if (per_slab > 0x7FFFFFFF || batch > 0x7FFFFFFF || channels > 0x7FFFFFFF) return RHO_E_SHAPE;
    g->groups = batch * channels * per_slab;
    if (g->groups > 0x7FFFFFFF) return RHO_E_SHAPE;
    return 0;
}

template <int KD, int KH, int KW>
void ssim_launch(bool vec, unsigned grid, hipStream_t st, const SsimK& k) {
    if (vec) hipLaunchKernelGGL((k_ssim<KD, KH, KW, true>), dim3(grid), dim3(SSIM_THREADS), 0, st, k);
    else hipLaunchKernelGGL((k_ssim<KD, KH, KW, false>), dim3(grid), dim3(SSIM_THREADS), 0, st, k);
}

}  // namespace

extern "C" int64_t rho_ssim_max_window(void) { return SSIM_MAXW; }

extern "C" int64_t rho_ssim_workspace_bytes(int64_t batch, int64_t channels, int ndim, const int64_t* sizes, const int64_t* window_sizes) {
    SsimGeom g;
    if (ssim_geometry(batch, channels, ndim, sizes, window_sizes, &g) != 0) return -1;
    const int64_t fold = 8 * (g.groups + batch), range = (int64_t)SSIM_RANGE_BLOCKS * 4 * sizeof(float);
    return fold > range ? fold : range;
}

extern "C" int rho_ssim_range(const float* pred, const float* target, int64_t n, float* out_range, void* workspace, int64_t workspace_bytes,
                              void* stream) {
    if (!pred || !target || !out_range || !workspace || n <= 0 || workspace_bytes < (int64_t)SSIM_RANGE_BLOCKS * 4 * (int64_t)sizeof(float) ||
        ((uintptr_t)workspace & 3))
        return RHO_E_ARG;
    int64_t g = (n + 256 * 8 - 1) / (256 * 8);
    if (g > SSIM_RANGE_BLOCKS) g = SSIM_RANGE_BLOCKS;
    const int vec = ((((uintptr_t)pred | (uintptr_t)target) & 15) == 0) ? 1 : 0;
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(k_ssim_range_part, dim3((unsigned)g), dim3(256), 0, as_stream(stream), pred, target, n, vec, ws);
    hipLaunchKernelGGL(k_ssim_range_final, dim3(1), dim3(64), 0, as_stream(stream), ws, (int)g, out_range);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_ssim(const float* pred, const float* target, int64_t batch, int64_t channels, int ndim, const int64_t* sizes,
                        const float* const* windows, const int64_t* window_sizes, float data_range, const float* data_range_dev, int clamp,
                        float lo, float hi, float k1, float k2, float* per_sample, float* out, float* map, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (!pred || !target || !windows || !per_sample || !out || !workspace) return RHO_E_ARG;
    SsimGeom g;
    const int rc = ssim_geometry(batch, channels, ndim, sizes, window_sizes, &g);
    if (rc != 0) return rc;
    for (int i = 0; i < ndim; ++i)
        if (!windows[i]) return RHO_E_ARG;
    if (!data_range_dev && !(data_range > 0.0f)) return RHO_E_ARG;
    if (clamp && !(hi > lo)) return RHO_E_ARG;
    if (workspace_bytes < 8 * (g.groups + batch) || ((uintptr_t)workspace & 7)) return RHO_E_ARG;
    SsimK k;
    k.p = pred; k.t = target;
    // a dimension the field does not have keeps a NULL window: the kernel reads it as {1.0}
    const float* w3[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < ndim; ++i) w3[3 - ndim + i] = windows[i];
    k.gd = w3[0]; k.gh = w3[1]; k.gw = w3[2];
    k.kd = (int)g.k[0]; k.kh = (int)g.k[1]; k.kw = (int)g.k[2];
    k.D = (int)g.d[0]; k.H = (int)g.d[1]; k.W = (int)g.d[2];
    k.Do = (int)g.o[0]; k.Ho = (int)g.o[1]; k.Wo = (int)g.o[2];
    k.nch = (int)g.nch; k.nth = (int)g.nth; k.ntw = (int)g.ntw;
    k.range_dev = data_range_dev; k.range = data_range;
    k.clamp = clamp ? 1 : 0; k.lo = lo; k.hi = hi; k.k1 = k1; k.k2 = k2;
    k.map = map;
    k.part = static_cast<double*>(workspace);
    const bool vec = (g.d[2] % 4 == 0) && ((((uintptr_t)pred | (uintptr_t)target) & 15) == 0);
    const unsigned grid = (unsigned)g.groups;
    hipStream_t st = as_stream(stream);
    if (k.kd == 11 && k.kh == 11 && k.kw == 11) ssim_launch<11, 11, 11>(vec, grid, st, k);
    else if (k.kd == 1 && k.kh == 11 && k.kw == 11) ssim_launch<1, 11, 11>(vec, grid, st, k);
    else if (k.kd == 1 && k.kh == 1 && k.kw == 11) ssim_launch<1, 1, 11>(vec, grid, st, k);
    else ssim_launch<0, 0, 0>(vec, grid, st, k);
    const double count = (double)channels * (double)g.o[0] * (double)g.o[1] * (double)g.o[2];
    hipLaunchKernelGGL(k_ssim_final, dim3(1), dim3(1024), 0, st, k.part, (int)batch, channels * g.nch * g.nth * g.ntw, count,
                       k.part + g.groups, per_sample, out);
    RHO_LAUNCH_CHECK();
    return 0;
}
