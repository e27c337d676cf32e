// Batched gather + normalise + center crop + bilinear resize of stored images: the default transform of the reference's
// DeepGalaxyDataset (rho_diffusion/data/deep_galaxy.py:79-89: torchvision CenterCrop(256) -> Resize((128, 128)) -> 2 t - 1, applied
// per item to the float32 [C, W, H] tensor of :126 = swapaxes(1, 3) of the rows normalised by :283-289 images / np.max(images)).
//
// rho_crop_resize_taps (host) turns crop + resize of one axis into a table of taps: output o reads k consecutive pixels from start[o]
// with float32 weights; torchvision's crop offset and zero padding are folded in (taps on the padding are dropped: a padded pixel is
// 0).  The kernel is HBM-bound.  Each workgroup owns a 32 (ox) x ty (oy) tile of one item: it stages the raw rows of its window into
// LDS with 16-byte loads (normalising on the way: one division per pixel), resamples them along the raw w axis (image rows -> oy)
// into a second LDS buffer, then along the raw h axis (image columns -> ox) into registers.  The h window is walked in chunks of hc
// raw rows, so the LDS footprint is bounded for any scale.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_TX = 32;                                   // output columns (ox) per workgroup
constexpr int CR_TY_MAX = 32;                               // output rows (oy) per workgroup at most
constexpr int CR_ACC = CR_TX * CR_TY_MAX / CR_THREADS;      // outputs per thread and channel
constexpr int CR_CMAX = 4;
constexpr int64_t CR_LDS_BUDGET = 48 * 1024;

struct CropK {
    const unsigned char* raw;
    const int64_t* index;
    const double* rowmax;
    const int32_t* ys;
    const float* wy;
    const int32_t* xs;
    const float* wx;
    float* out;
    int32_t* err_flag;
    int64_t n, total;       // rows, elements of raw
    int h, w, c, ky, kx, out_h, out_w;
    int ty, hc, swp, ts;    // tile rows; raw rows staged per chunk; LDS floats per staged row; LDS floats per resampled row
};

template <int DT> struct RawT;
template <> struct RawT<RHO_U8> { typedef unsigned char T; };
template <> struct RawT<RHO_F32> { typedef float T; };
template <> struct RawT<RHO_F64> { typedef double T; };

// numpy's images / np.max(images) for one element, rounded to float32 as torch.FloatTensor does (uint8 / uint8 divides in float64)
__device__ __forceinline__ float norm_px(unsigned char x, double mx) { return (float)((double)x / mx); }
__device__ __forceinline__ float norm_px(float x, double mx) { return x / (float)mx; }
__device__ __forceinline__ float norm_px(double x, double mx) { return (float)(x / mx); }

template <int DT>
__global__ __launch_bounds__(CR_THREADS) void k_crop_resize(const CropK p) {
    typedef typename RawT<DT>::T T;
    constexpr int VE = 16 / (int)sizeof(T);                 // elements per 16-byte load
    extern __shared__ float4 lds4[];
    float* lds = reinterpret_cast<float*>(lds4);
    const int b = blockIdx.z;
    const int64_t row = p.index[b];
    if (row < 0 || row >= p.n) {                            // uniform over the workgroup, before any barrier
        if (threadIdx.x == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 4);
        return;
    }
    const double mx = p.rowmax[row];
    const int C = p.c;
    const int ox0 = blockIdx.x * CR_TX, oy0 = blockIdx.y * p.ty;
    const int nox = min(CR_TX, p.out_w - ox0), noy = min(p.ty, p.out_h - oy0);
    const int w_lo = p.ys[oy0], w_hi = p.ys[oy0 + noy - 1] + p.ky;      // raw w window of the tile (starts are non-decreasing)
    const int h_lo = p.xs[ox0], h_hi = p.xs[ox0 + nox - 1] + p.kx;      // raw h window
    const int nvec = ((w_hi - w_lo) * C + 2 * VE - 2) / VE;             // 16-byte loads per staged row, any alignment of its start
    if (nvec * VE > p.swp) {                                            // tables built for another crop than the launch's
        if (threadIdx.x == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 8);
        return;
    }
    float* S = lds;                                         // [hc][swp]: normalised raw rows of the window
    float* Tb = lds + p.hc * p.swp;                         // [hc][ts]: resampled along w, (oy, channel) interleaved
    const int64_t row0 = row * (int64_t)p.h * p.w * C;      // element index of raw[row, 0, 0, 0]
    const T* src = reinterpret_cast<const T*>(p.raw);
    float acc[CR_CMAX][CR_ACC];
#pragma unroll
    for (int ch = 0; ch < CR_CMAX; ++ch)
#pragma unroll
        for (int j = 0; j < CR_ACC; ++j) acc[ch][j] = 0.0f;

    for (int hc0 = h_lo; hc0 < h_hi; hc0 += p.hc) {
        const int nh = min(p.hc, h_hi - hc0);
        // 1. raw rows hc0 .. hc0 + nh - 1 from the 16-byte boundary at or below the window start, normalised
        for (int i = threadIdx.x; i < nh * nvec; i += CR_THREADS) {
            const int r = i / nvec, v = i - r * nvec;
            const int64_t g0 = row0 + ((int64_t)(hc0 + r) * p.w + w_lo) * C;
            const int64_t ga = (g0 / VE + v) * VE;
            float f[VE];
            if (ga + VE <= p.total) {
                const uint4 q = *reinterpret_cast<const uint4*>(src + ga);
                T e[VE];
                __builtin_memcpy(e, &q, 16);
#pragma unroll
                for (int k = 0; k < VE; ++k) f[k] = norm_px(e[k], mx);
            } else {
#pragma unroll
                for (int k = 0; k < VE; ++k) f[k] = ga + k < p.total ? norm_px(src[ga + k], mx) : 0.0f;
            }
            float* d = S + r * p.swp + v * VE;
            if constexpr (VE >= 4) {
#pragma unroll
                for (int k = 0; k < VE; k += 4) *reinterpret_cast<float4*>(d + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
            } else {
                *reinterpret_cast<float2*>(d) = make_float2(f[0], f[1]);
            }
        }
        __syncthreads();
        // 2. along w (image rows -> oy)
        for (int i = threadIdx.x; i < nh * noy * C; i += CR_THREADS) {
            const int ch = i % C, t2 = i / C, oyl = t2 % noy, r = t2 / noy;
            const int oy = oy0 + oyl;
            const int64_t g0 = row0 + ((int64_t)(hc0 + r) * p.w + w_lo) * C;
            const float* s = S + r * p.swp + (int)(g0 % VE) + (p.ys[oy] - w_lo) * C + ch;
            const float* wt = p.wy + (int64_t)oy * p.ky;
            float a = 0.0f;
            for (int k = 0; k < p.ky; ++k) a = fmaf(wt[k], s[k * C], a);
            Tb[r * p.ts + oyl * C + ch] = a;
        }
        __syncthreads();
        // 3. along h (image columns -> ox), accumulated over the chunks in tap order
#pragma unroll
        for (int j = 0; j < CR_ACC; ++j) {
            const int k = threadIdx.x + j * CR_THREADS;
            const int oyl = k / CR_TX, oxl = k % CR_TX;
            if (oyl < noy && oxl < nox) {
                const int ox = ox0 + oxl, x0 = p.xs[ox];
                const int q0 = max(0, hc0 - x0), q1 = min(p.kx, hc0 + nh - x0);
                const float* wt = p.wx + (int64_t)ox * p.kx;
                for (int q = q0; q < q1; ++q) {
                    const float wq = wt[q];
                    const float* t = Tb + (x0 + q - hc0) * p.ts + oyl * C;
#pragma unroll
                    for (int ch = 0; ch < CR_CMAX; ++ch)
                        if (ch < C) acc[ch][j] = fmaf(wq, t[ch], acc[ch][j]);
                }
            }
        }
        __syncthreads();
    }
    // 4. the Lambda of deep_galaxy.py:89: 2 t - 1
#pragma unroll
    for (int j = 0; j < CR_ACC; ++j) {
        const int k = threadIdx.x + j * CR_THREADS;
        const int oyl = k / CR_TX, oxl = k % CR_TX;
        if (oyl < noy && oxl < nox) {
#pragma unroll
            for (int ch = 0; ch < CR_CMAX; ++ch)
                if (ch < C)
                    p.out[(((int64_t)b * C + ch) * p.out_h + oy0 + oyl) * p.out_w + ox0 + oxl] = 2.0f * acc[ch][j] - 1.0f;
        }
    }
}

}  // namespace

extern "C" int64_t rho_crop_resize_taps(int64_t in_size, int64_t crop, int64_t out_size, int antialias, int32_t* start, float* weight) {
    if (in_size <= 0 || crop <= 0 || out_size <= 0 || in_size > (1 << 24) || crop > (1 << 24) || out_size > (1 << 24)) return RHO_E_ARG;
    if ((start == nullptr) != (weight == nullptr)) return RHO_E_ARG;
    // torchvision center_crop: a larger crop pads (crop - in) // 2 zeros in front, else the crop starts at int(round((in - crop) / 2))
    int64_t off;
    if (crop > in_size) {
        off = -((crop - in_size) / 2);
    } else {
        const int64_t d = in_size - crop;
        off = d / 2;
        if ((d & 1) && (off & 1)) off += 1;                  // Python's round: half to even
    }
    // interpolate(bilinear, align_corners=False) on the crop, in the float32 arithmetic of torch's CPU kernels for a float32 image
    const float scale = (float)crop / (float)out_size;
    std::vector<std::vector<std::pair<int64_t, float>>> taps((size_t)out_size);
    for (int64_t o = 0; o < out_size; ++o) {
        auto& t = taps[(size_t)o];
        if (antialias) {                                     // triangle filter whose support widens with the scale (_upsample_bilinear2d_aa)
            const float support = scale >= 1.0f ? scale : 1.0f;
            const float center = (float)((double)scale * ((double)o + 0.5));
            const float invscale = scale >= 1.0f ? (float)(1.0 / (double)scale) : 1.0f;
            const int64_t xmin = std::max((int64_t)((double)(center - support) + 0.5), (int64_t)0);
            const int64_t xsize = std::min((int64_t)((double)(center + support) + 0.5), crop) - xmin;
            float total = 0.0f;
            for (int64_t j = 0; j < xsize; ++j) {
                const float x = std::fabs((float)(((double)((float)(j + xmin) - center) + 0.5) * (double)invscale));
                const float wgt = x < 1.0f ? (float)(1.0 - (double)x) : 0.0f;
                t.push_back({xmin + j, wgt});
                total += wgt;
            }
            if (total != 0.0f)
                for (auto& e : t) e.second = e.second / total;
        } else if (crop == out_size) {                       // torch copies an axis whose size does not change
            t.push_back({o, 1.0f});
        } else {                                             // two taps, the source index clamped at 0 and at the last pixel
            float src = std::fma(scale, (float)o + 0.5f, -0.5f);       // rounded once, as torch's (contracted) CPU kernel does
            if (src < 0.0f) src = 0.0f;
            const int64_t i0 = std::min((int64_t)std::floor(src), crop - 1);
            const float l1 = std::min(std::max(src - (float)i0, 0.0f), 1.0f);
            if (i0 < crop - 1) {
                t.push_back({i0, 1.0f - l1});
                t.push_back({i0 + 1, l1});
            } else {
                t.push_back({i0, 1.0f});
            }
        }
    }
    // image pixels: drop the taps on the padding, one window of k pixels per output inside [0, in_size)
    int64_t k = 1;
    for (const auto& t : taps) {
        int64_t cnt = 0;
        for (const auto& e : t) cnt += (e.first + off >= 0 && e.first + off < in_size) ? 1 : 0;
        k = std::max(k, cnt);
    }
    if (start == nullptr) return k;
    for (int64_t o = 0; o < out_size; ++o) {
        const auto& t = taps[(size_t)o];
        const int64_t first = t.empty() ? 0 : t.front().first + off;
        const int64_t s = std::min(std::max(first, (int64_t)0), in_size - k);      // non-decreasing in o
        start[o] = (int32_t)s;
        for (int64_t j = 0; j < k; ++j) weight[o * k + j] = 0.0f;
        for (const auto& e : t) {
            const int64_t px = e.first + off;
            if (px >= 0 && px < in_size) weight[o * k + (px - s)] = e.second;
        }
    }
    return k;
}

extern "C" int rho_crop_resize(const void* raw, int dtype, int64_t n, int64_t h, int64_t w, int64_t c, const int64_t* index, int64_t batch,
                               const double* rowmax, const int32_t* ys, const float* wy, int64_t ky, const int32_t* xs, const float* wx,
                               int64_t kx, int64_t crop_h, int64_t crop_w, int64_t out_h, int64_t out_w, float* out, int32_t* err_flag,
                               void* stream) {
    if (!raw || !index || !rowmax || !ys || !wy || !xs || !wx || !out) return RHO_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c > CR_CMAX || w * c >= (1 << 30) || h >= (1 << 30) || batch <= 0 || batch > 65535 ||
        ky <= 0 || ky > w || kx <= 0 || kx > h || crop_h <= 0 || crop_w <= 0 || out_h <= 0 || out_w <= 0 || out_h > (1 << 24) ||
        out_w > (1 << 24))
        return RHO_E_ARG;
    int es;
    switch (dtype) {
        case RHO_U8: es = 1; break;
        case RHO_F32: es = 4; break;
        case RHO_F64: es = 8; break;
        default: return RHO_E_ARG;
    }
    if (reinterpret_cast<uintptr_t>(raw) % 16 != 0) return RHO_E_ALIGN;
    // tile rows: the largest ty whose staged w window leaves room for >= 8 raw rows per chunk in the LDS budget.  The windows are
    // bounded from the crop scales (consecutive starts differ by at most floor(scale) + 1); a chunk holds the whole h window of a
    // tile when it fits (one pass of the three phases: the 512^2 -> 256 -> 128 default takes 68 rows), else the window is walked
    // in chunks of hc rows.
    const int ve = 16 / es;
    const double sy = (double)crop_h / (double)out_h, sx = (double)crop_w / (double)out_w;
    const int64_t span_h = std::min<int64_t>(h, (int64_t)std::floor(sx * (double)(CR_TX - 1)) + 2 + kx);
    int ty = 0, hc = 0, swp = 0, ts = 0;
    for (int t = CR_TY_MAX; t >= 1; t /= 2) {
        const int64_t span = std::min<int64_t>(w, (int64_t)std::floor(sy * (double)(t - 1)) + 2 + ky);
        const int64_t sw = ((span * c + 2 * ve - 2) / ve) * ve, tsz = (int64_t)t * c + 1;
        const int64_t rows = std::min<int64_t>(span_h, CR_LDS_BUDGET / (4 * (sw + tsz)));
        if (rows >= std::min<int64_t>(8, span_h) || (t == 1 && rows >= 1)) {
            ty = t;
            hc = (int)rows;
            swp = (int)sw;
            ts = (int)tsz;
            break;
        }
    }
    if (ty == 0 || (out_h + ty - 1) / ty > 65535) return RHO_E_SHAPE;
    CropK p{};
    p.raw = reinterpret_cast<const unsigned char*>(raw);
    p.index = index;
    p.rowmax = rowmax;
    p.ys = ys;
    p.wy = wy;
    p.xs = xs;
    p.wx = wx;
    p.out = out;
    p.err_flag = err_flag;
    p.n = n;
    p.total = n * h * w * c;
    p.h = (int)h; p.w = (int)w; p.c = (int)c;
    p.ky = (int)ky; p.kx = (int)kx; p.out_h = (int)out_h; p.out_w = (int)out_w;
    p.ty = ty; p.hc = hc; p.swp = swp; p.ts = ts;
    const size_t shm = (size_t)hc * (size_t)(swp + ts) * sizeof(float);
    const dim3 grid((unsigned)((out_w + CR_TX - 1) / CR_TX), (unsigned)((out_h + ty - 1) / ty), (unsigned)batch);
    hipStream_t st = as_stream(stream);
    switch (dtype) {
        case RHO_U8: hipLaunchKernelGGL(k_crop_resize<RHO_U8>, grid, dim3(CR_THREADS), shm, st, p); break;
        case RHO_F32: hipLaunchKernelGGL(k_crop_resize<RHO_F32>, grid, dim3(CR_THREADS), shm, st, p); break;
        default: hipLaunchKernelGGL(k_crop_resize<RHO_F64>, grid, dim3(CR_THREADS), shm, st, p); break;
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// MNISTDataset / CIFAR10Dataset (rho_diffusion/data/wrappers.py:37-116): torchvision builds a PIL.Image per item and runs
// Resize((32, 32)) (MNIST only) -> ToTensor() -> 2 t - 1 on it.  Resize of a PIL image is Image.resize(size, BILINEAR): Pillow's
// two-pass fixed-point resample (src/libImaging/Resample.c), integer arithmetic on uint8 with a uint8 intermediate, so the whole
// transform is integers plus a 256-entry table and is restated here bit for bit.
//
// rho_pil_resize_taps (host) is precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter.  k_u8_image_batch walks the items
// with a capped grid, one item per workgroup and turn: the tap tables and the LUT go to LDS once per workgroup, then per item the raw
// bytes are staged (16-byte loads where the item size allows), resampled along x into a second uint8 LDS image, and resampled along
// y on the way out; each thread produces four consecutive floats of the [C, oh, ow] item, so the stores run along ox.  An item is
// hundreds of bytes in and a few KiB out: the kernel is bound by launch and memory latency, not by bandwidth.
namespace {

constexpr int UI_THREADS = 256;
constexpr int UI_MAX_WGS = 2048;                            // 8 workgroups on each of 256 CUs; larger batches take turns
constexpr int64_t UI_LDS_BUDGET = 64 * 1024;
constexpr int UI_PRECISION_BITS = 32 - 8 - 2;               // Resample.c PRECISION_BITS

struct U8K {
    const unsigned char* raw;
    const int64_t* index;
    const int32_t* ys; const int32_t* yn; const int32_t* ky;
    const int32_t* xs; const int32_t* xn; const int32_t* kx;
    const float* lut;
    float* out;
    int32_t* err_flag;
    int64_t n, batch;
    int h, w, c, ksy, ksx, out_h, out_w;
    int vec_in, vec_out;            // 16-byte loads of the item / 16-byte stores of the output are possible
    int o_x, o_y, o_raw, o_tmp;     // byte offsets of the LDS regions (the LUT is at 0)
};

// Resample.c clip8: (in >> PRECISION_BITS) clamped to [0, 255].  The sum is kept unsigned (tables from rho_pil_resize_taps never
// overflow it: 255 * (2^22 + ksize) + 2^21 < 2^31) and read back as int32.
__device__ __forceinline__ unsigned char ui_clip8(uint32_t acc) {
    const int v = (int)acc >> UI_PRECISION_BITS;
    return (unsigned char)min(max(v, 0), 255);
}

// one axis' tables -> LDS; returns 1 if a window does not lie inside [0, in_size) or is longer than ks
__device__ __forceinline__ int ui_load_taps(const int32_t* gs, const int32_t* gn, const int32_t* gk, int32_t* s, int32_t* nn, int32_t* k,
                                            int out_size, int ks, int in_size) {
    int bad = 0;
    for (int i = threadIdx.x; i < out_size; i += UI_THREADS) {
        const int32_t a = gs[i], cnt = gn[i];
        bad |= (a < 0 || cnt < 0 || cnt > ks || a > in_size - cnt) ? 1 : 0;
        s[i] = a;
        nn[i] = cnt;
    }
    for (int i = threadIdx.x; i < out_size * ks; i += UI_THREADS) k[i] = gk[i];
    return bad;
}

__global__ __launch_bounds__(UI_THREADS) void k_u8_image_batch(const U8K p) {
    extern __shared__ float4 lds4[];
    unsigned char* lds = reinterpret_cast<unsigned char*>(lds4);
    float* lut = reinterpret_cast<float*>(lds);
    int32_t* xs = reinterpret_cast<int32_t*>(lds + p.o_x);
    int32_t* xn = xs + p.out_w;
    int32_t* kx = xn + p.out_w;
    int32_t* ys = reinterpret_cast<int32_t*>(lds + p.o_y);
    int32_t* yn = ys + p.out_h;
    int32_t* ky = yn + p.out_h;
    unsigned char* rawL = lds + p.o_raw;
    unsigned char* tmpL = lds + p.o_tmp;
    const int tid = threadIdx.x;
    const int C = p.c, W = p.w, OW = p.out_w, OH = p.out_h;
    const int isz = p.h * W * C, tsz = p.h * OW * C, osz = C * OH * OW;

    int bad = 0;
    for (int i = tid; i < 256; i += UI_THREADS) lut[i] = p.lut[i];
    if (p.ksx > 0) bad |= ui_load_taps(p.xs, p.xn, p.kx, xs, xn, kx, OW, p.ksx, W);
    if (p.ksy > 0) bad |= ui_load_taps(p.ys, p.yn, p.ky, ys, yn, ky, OH, p.ksy, p.h);
    if (__syncthreads_or(bad)) {                            // tables built for another geometry: nothing is read through them
        if (tid == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 8);
        return;
    }

    for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
        const int64_t row = p.index[b];
        if (row < 0 || row >= p.n) {                        // uniform over the workgroup
            if (tid == 0 && p.err_flag != nullptr) atomicOr(p.err_flag, 4);
            continue;
        }
        // 1. the item's bytes
        const unsigned char* src = p.raw + row * (int64_t)isz;
        if (p.vec_in) {
            for (int i = tid; i < isz / 16; i += UI_THREADS)
                reinterpret_cast<uint4*>(rawL)[i] = reinterpret_cast<const uint4*>(src)[i];
        } else {
            for (int i = tid; i < isz; i += UI_THREADS) rawL[i] = src[i];
        }
        __syncthreads();
        // 2. ImagingResampleHorizontal_8bpc: every row, [h, w, c] -> uint8 [h, ow, c]
        const unsigned char* P = rawL;
        if (p.ksx > 0) {
            for (int i = tid; i < tsz; i += UI_THREADS) {
                const int ch = i % C, t = i / C, ox = t % OW, y = t / OW;
                const int cnt = xn[ox];
                const int32_t* k = kx + ox * p.ksx;
                const unsigned char* r = rawL + (y * W + xs[ox]) * C + ch;
                uint32_t acc = 1u << (UI_PRECISION_BITS - 1);
                for (int j = 0; j < cnt; ++j) acc += (uint32_t)r[j * C] * (uint32_t)k[j];
                tmpL[i] = ui_clip8(acc);
            }
            __syncthreads();
            P = tmpL;
        }
        // 3. ImagingResampleVertical_8bpc (or the copy of an axis that keeps its size), the LUT, HWC -> CHW: four consecutive
        //    outputs per thread in the order of the output's memory
        float* o = p.out + b * (int64_t)osz;
        const int sy = OW * C;                              // bytes between two rows of P
        for (int k0 = tid * 4; k0 < osz; k0 += UI_THREADS * 4) {
            int ox = k0 % OW, t = k0 / OW;
            int oy = t % OH, ch = t / OH;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = 0.0f;
                if (k0 + e < osz) {
                    unsigned char u;
                    if (p.ksy > 0) {
                        const int cnt = yn[oy];
                        const int32_t* k = ky + oy * p.ksy;
                        const unsigned char* r = P + (ys[oy] * OW + ox) * C + ch;
                        uint32_t acc = 1u << (UI_PRECISION_BITS - 1);
                        for (int i = 0; i < cnt; ++i) acc += (uint32_t)r[i * sy] * (uint32_t)k[i];
                        u = ui_clip8(acc);
                    } else {
                        u = P[(oy * OW + ox) * C + ch];
                    }
                    v[e] = lut[u];
                }
                if (++ox == OW) {
                    ox = 0;
                    if (++oy == OH) {
                        oy = 0;
                        ++ch;
                    }
                }
            }
            if (p.vec_out) {                                // osz is a multiple of 4 then: all four are inside the item
                *reinterpret_cast<float4*>(o + k0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e < osz) o[k0 + e] = v[e];
            }
        }
        __syncthreads();                                    // the next item overwrites the staged images
    }
}

double ui_bilinear(double x) {                              // Resample.c bilinear_filter, support 1.0
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

}  // namespace

extern "C" int64_t rho_pil_resize_taps(int64_t in_size, int64_t out_size, int32_t* start, int32_t* count, int32_t* coef) {
    if (in_size <= 0 || out_size <= 0 || in_size > (1 << 24) || out_size > (1 << 24)) return RHO_E_ARG;
    const int given = (start != nullptr) + (count != nullptr) + (coef != nullptr);
    if (given != 0 && given != 3) return RHO_E_ARG;
    // precompute_coeffs, in0 = 0 and in1 = in_size (the whole image), all in double
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int64_t ksize = (int64_t)std::ceil(support) * 2 + 1;
    if (given == 0) return ksize;
    const double ss = 1.0 / filterscale;                    // Pillow multiplies by the reciprocal, it does not divide
    std::vector<double> k((size_t)ksize);
    for (int64_t xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + ((double)xx + 0.5) * scale;
        double ww = 0.0;
        int64_t xmin = (int64_t)(int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int64_t xmax = (int64_t)(int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int64_t x = 0; x < xmax; ++x) {
            const double w = ui_bilinear(((double)(x + xmin) - center + 0.5) * ss);
            k[(size_t)x] = w;
            ww += w;
        }
        for (int64_t x = 0; x < xmax; ++x)
            if (ww != 0.0) k[(size_t)x] /= ww;
        for (int64_t x = xmax; x < ksize; ++x) k[(size_t)x] = 0.0;
        start[xx] = (int32_t)xmin;
        count[xx] = (int32_t)xmax;
        // normalize_coeffs_8bpc: (int)(0.5 + w * 2^22).  Its (int)(-0.5 + ...) branch is for negative weights, which the
        // triangle filter never produces.
        for (int64_t x = 0; x < ksize; ++x) coef[xx * ksize + x] = (int32_t)(0.5 + k[(size_t)x] * (double)(1 << UI_PRECISION_BITS));
    }
    return ksize;
}

extern "C" int rho_u8_image_batch(const uint8_t* raw, int64_t n, int64_t h, int64_t w, int64_t c, const int64_t* index, int64_t batch,
                                  const int32_t* ys, const int32_t* yn, const int32_t* ky, int64_t ksy, const int32_t* xs,
                                  const int32_t* xn, const int32_t* kx, int64_t ksx, int64_t out_h, int64_t out_w, const float* lut,
                                  float* out, int32_t* err_flag, void* stream) {
    if (!raw || !index || !lut || !out) return RHO_E_ARG;
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || c > CR_CMAX || batch <= 0 || batch > INT32_MAX || out_h <= 0 || out_w <= 0 || ksy < 0 ||
        ksx < 0)
        return RHO_E_ARG;
    // an axis without tables keeps its size (Pillow skips that pass); one with tables has all three
    if (ksy == 0 ? (ys || yn || ky || out_h != h) : (!ys || !yn || !ky)) return RHO_E_ARG;
    if (ksx == 0 ? (xs || xn || kx || out_w != w) : (!xs || !xn || !kx)) return RHO_E_ARG;
    if (reinterpret_cast<uintptr_t>(lut) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0) return RHO_E_ALIGN;
    // LDS: LUT | x tables | y tables | item | x-resampled item, each region 16-byte aligned.  Every term is bounded before it is
    // multiplied, so nothing overflows.
    const int64_t lim = UI_LDS_BUDGET;
    if (h > lim || w > lim || out_h > lim || out_w > lim || ksy > lim || ksx > lim) return RHO_E_SHAPE;
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    const int64_t isz = h * w * c, tsz = ksx > 0 ? h * out_w * c : 0;
    const int64_t o_x = 256 * 4, o_y = o_x + up16(ksx > 0 ? (2 + ksx) * out_w * 4 : 0);
    const int64_t o_raw = o_y + up16(ksy > 0 ? (2 + ksy) * out_h * 4 : 0), o_tmp = o_raw + up16(isz), shm = o_tmp + up16(tsz);
    if (shm > UI_LDS_BUDGET) return RHO_E_SHAPE;
    U8K p{};
    p.raw = raw;
    p.index = index;
    p.ys = ys; p.yn = yn; p.ky = ky;
    p.xs = xs; p.xn = xn; p.kx = kx;
    p.lut = lut;
    p.out = out;
    p.err_flag = err_flag;
    p.n = n;
    p.batch = batch;
    p.h = (int)h; p.w = (int)w; p.c = (int)c;
    p.ksy = (int)ksy; p.ksx = (int)ksx; p.out_h = (int)out_h; p.out_w = (int)out_w;
    p.vec_in = (isz % 16 == 0 && reinterpret_cast<uintptr_t>(raw) % 16 == 0) ? 1 : 0;
    p.vec_out = ((c * out_h * out_w) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) ? 1 : 0;
    p.o_x = (int)o_x; p.o_y = (int)o_y; p.o_raw = (int)o_raw; p.o_tmp = (int)o_tmp;
    const dim3 grid((unsigned)std::min<int64_t>(batch, UI_MAX_WGS));
    hipLaunchKernelGGL(k_u8_image_batch, grid, dim3(UI_THREADS), (size_t)shm, as_stream(stream), p);
    RHO_LAUNCH_CHECK();
    return 0;
}
