// Sample metrics on the device: the debiased Sinkhorn divergence behind WassersteinWrapper (metrics/geom.py:28-37, geomloss's
// SamplesLoss("sinkhorn", p=1, blur=0.01) over flatten(1)) and PeakSignalNoiseRatio (abstract_diffusion.py:79).  Inputs, outputs
// and the streaming passes are float32; the cost sums, the diameter and the loop run in float64.
//
//   rho_pairwise_cost    one streaming pass over z = [x; y] -> per-chunk partial squared distances, then an ordered sum over chunks
//   rho_max_diameter     per-coordinate extent of z -> one float
//   rho_sinkhorn_loop    the whole epsilon-scaling schedule in ONE workgroup (cost matrices in LDS while they fit), + the weights of
//                        the last step's gradient
//   rho_rows_combine     grad_x = A z, the second streaming pass
//   rho_psnr             sum of squared error, min and max of the target in one pass
//
// No atomics anywhere: every reduction adds its pieces in an order fixed by the shapes alone, so two runs give the same bits.
#include "common.h"

namespace {

constexpr int SK_MAXN = 128;      // samples per side (N, M)
constexpr int SK_CHUNK = 512;     // floats of D per workgroup = per partial (fixed: the summation order does not depend on the grid)
constexpr int SK_TW = 64;         // columns of the chunk staged in LDS per step (rho_rows_combine; rho_pairwise_cost: 64 .. 512 by row count)
constexpr int SK_LD = SK_TW + 1;  // row stride of the staged tile, tw + 1: rows land on different banks

__device__ __forceinline__ const float* z_row(const float* x, const float* y, int n, int64_t d, int r) {
    return r < n ? x + (int64_t)r * d : y + (int64_t)(r - n) * d;
}

// Stage columns [d0, d0 + tw) of all R rows (zero beyond dend), tw = 1 << tw_log2 >= 64, row stride tw + 1.  VEC: every row start is
// 16-byte aligned (D % 4 == 0, bases aligned).
template <bool VEC>
__device__ __forceinline__ void stage_tile(float* tile, const float* x, const float* y, int n, int R, int64_t D, int64_t d0, int64_t dend,
                                           int tw_log2) {
    const int ld = (1 << tw_log2) + 1;
    if (VEC) {
        const int q_log2 = tw_log2 - 2;
#pragma unroll 4
        for (int e = threadIdx.x; e < (R << q_log2); e += blockDim.x) {
            const int row = e >> q_log2, c4 = e & ((1 << q_log2) - 1);
            const int64_t col = d0 + 4 * c4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (col < dend) v = *reinterpret_cast<const float4*>(z_row(x, y, n, D, row) + col);     // dend % 4 == 0 here
            float* t = tile + row * ld + 4 * c4;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    } else {
#pragma unroll 4
        for (int e = threadIdx.x; e < (R << tw_log2); e += blockDim.x) {
            const int row = e >> tw_log2, c = e & ((1 << tw_log2) - 1);
            const int64_t col = d0 + c;
            tile[row * ld + c] = col < dend ? z_row(x, y, n, D, row)[col] : 0.0f;
        }
    }
}

// ----------------------------------------------------------------------------- pairwise squared distances
// Workgroup (round, chunk): the chunk's columns of all R = N + M rows pass through LDS once and serve every pair.  The upper triangle
// of the R x R matrix is cut into 4 x 4 blocks of pairs; a thread owns one block and every S-th column (S * blocks <= 256 where the
// blocks allow it: two samples a side still keep a wave busy), holds the 16 sums in registers over the whole chunk and the S column
// slices are added by a butterfly at the end.  The chunk is staged 64 .. 512 columns at a time (fewer rows, wider steps); a thread's
// columns come in the same order whatever the width.  More than 256 blocks (N + M > 88) take further rounds = workgroups on the same chunk.
// The sums run in float64 (the inputs are float32, so every difference is exact and a square carries 1e-16): the transport plan of
// a small blur is decided by cost differences ~1e-7 of the costs themselves, which float32 sums cannot hold.
template <bool VEC>
__global__ __launch_bounds__(256) void k_pair_part(const float* __restrict__ x, const float* __restrict__ y, int n, int R, int64_t D,
                                                   int nbr, int nblk, int S, int tw_log2, double* __restrict__ part) {
    extern __shared__ float tile[];
    const int TW = 1 << tw_log2, LD = TW + 1;
    const int chunk = blockIdx.y;
    const int s = threadIdx.x % S;
    const int b = blockIdx.x * (256 / S) + threadIdx.x / S;
    const bool live = b < nblk;
    int bi = 0;
    if (live)
        while (bi + 1 < nbr && (bi + 1) * nbr - ((bi + 1) * bi) / 2 <= b) ++bi;
    const int bj = live ? bi + (b - (bi * nbr - (bi * (bi - 1)) / 2)) : 0;
    int ra[4], rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        ra[u] = min(bi * 4 + u, R - 1) * LD;
        rb[u] = min(bj * 4 + u, R - 1) * LD;
    }
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;

    const int64_t dbeg = (int64_t)chunk * SK_CHUNK;
    const int64_t dend = dbeg + SK_CHUNK < D ? dbeg + SK_CHUNK : D;
    for (int64_t d0 = dbeg; d0 < dend; d0 += TW) {
        __syncthreads();
        stage_tile<VEC>(tile, x, y, n, R, D, d0, dend, tw_log2);
        __syncthreads();
        const int tw = (int)(dend - d0 < TW ? dend - d0 : TW);
        if (live) {
#pragma unroll 2
            for (int c = s; c < tw; c += S) {
                double a[4], bb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = (double)tile[ra[u] + c]; bb[u] = (double)tile[rb[u] + c]; }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const double df = a[u] - bb[v];
                        acc[u][v] += df * df;
                    }
            }
        }
    }
    // the S slices of a block sit on S consecutive lanes of one wave
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            for (int o = S >> 1; o > 0; o >>= 1) acc[u][v] += __shfl_xor(acc[u][v], o, 64);
    if (live && s == 0) {
        const int64_t npairs = (int64_t)R * (R + 1) / 2;
        double* out = part + (int64_t)chunk * npairs;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = bi * 4 + u, j = bj * 4 + v;
                if (i < R && j < R && i <= j) out[i * R - (i * (i - 1)) / 2 + (j - i)] = acc[u][v];
            }
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per entry of C_xy | C_xx | C_yy: lane l adds chunks l, l + 64, ... in index order, then the butterfly.  The cost is written
// as float32 and, for the loop, as float64 (c64: the three matrices back to back, or NULL).
__global__ __launch_bounds__(256) void k_pair_final(const double* __restrict__ part, int nchunks, int n, int m, int p,
                                                    float* __restrict__ c_xy, float* __restrict__ c_xx, float* __restrict__ c_yy,
                                                    double* __restrict__ c64) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_xy = n * m, n_xx = n * n, n_yy = m * m;
    if (e >= n_xy + n_xx + n_yy) return;                      // whole waves leave together
    const int R = n + m;
    int zi, zj;
    float* dst;
    if (e < n_xy) { zi = e / m; zj = n + e % m; dst = c_xy + e; }
    else if (e < n_xy + n_xx) { const int q = e - n_xy; zi = q / n; zj = q % n; dst = c_xx + q; }
    else { const int q = e - n_xy - n_xx; zi = n + q / m; zj = n + q % m; dst = c_yy + q; }
    const int i = zi < zj ? zi : zj, j = zi < zj ? zj : zi;
    const int64_t npairs = (int64_t)R * (R + 1) / 2;
    const double* src = part + (i * R - (i * (i - 1)) / 2 + (j - i));
    double acc = 0.0;
    for (int c0 = lane; c0 < nchunks; c0 += 64 * 8) {         // 8 loads in flight; added in index order (+0 beyond the end)
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = c0 + 64 * k < nchunks ? src[(int64_t)(c0 + 64 * k) * npairs] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
    }
    acc = wave_sum_d(acc);
    if (lane == 0) {
        const double c = p == 2 ? 0.5 * acc : (acc <= 1e-8 ? 1e-4 : sqrt(acc));
        *dst = (float)c;
        if (c64) c64[e] = c;
    }
}

// ----------------------------------------------------------------------------- diameter
__global__ __launch_bounds__(256) void k_diam_part(const float* __restrict__ x, const float* __restrict__ y, int n, int R, int64_t D,
                                                   double* __restrict__ partials) {
    __shared__ double red[4];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t d = (int64_t)blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (d < D) {
            float mn = x[d], mx = mn;
            for (int r = 1; r < R; ++r) {
                const float v = z_row(x, y, n, D, r)[d];
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
            const double t = (double)mx - (double)mn;
            acc += t * t;
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_diam_final(const double* __restrict__ partials, int np, double* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += partials[i];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *out = sqrt((red[0] + red[1]) + (red[2] + red[3]));
}

// ----------------------------------------------------------------------------- the Sinkhorn loop
struct LoopArgs {
    const double *c_xy, *c_xx, *c_yy, *eps_list;
    int n_eps, n, m, debias, p;
    int lds_xy, lds_xx, lds_yy;          // which matrices are copied into LDS
    float *f_ba, *g_ab, *f_aa, *g_bb, *h_b, *h_a, *loss;
    float *wp, *wq, *rp, *rq;            // gradient weights (all four or none)
};

// softmin with the uniform log-weight -log(len) folded in analytically: -eps * logsumexp_k(-log(len) + (pot[k] - C[k * stride]) / eps)
// = -eps * (max_k u_k + log1p(mean_k expm1(u_k - max))), u_k = (pot[k] - C[k * stride]) / eps.  The same function as the
// max-subtracted logsumexp of h = log-weight + pot / eps, without its cancellation: at the large temperatures the schedule starts
// from, log(len) and the logsumexp cancel to ~C / eps, and their float32 rounding times eps (up to diameter^p) would shift all
// potentials by many ulps of C.  By the L lanes of one row group (lane index l).
__device__ __forceinline__ double softmin_uniform(const double* c, int stride, const double* pot, int len, double eps, int l, int L) {
    double mx = -INFINITY;
    for (int k = l; k < len; k += L) mx = fmax(mx, (pot[k] - c[k * stride]) / eps);
    for (int o = L >> 1; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    double sum = 0.0;
    for (int k = l; k < len; k += L) sum += expm1((pot[k] - c[k * stride]) / eps - mx);
    for (int o = L >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    return -eps * (mx + log1p(sum / (double)(len > 0 ? len : 1)));
}

// -eps * logsumexp_k(h[k] - C[k * stride] / eps) over `len` entries, max-subtracted, with the maximum and the sum of exponentials
// (the softmax of the gradient weights).
__device__ __forceinline__ double softmin_row(const double* c, int stride, const double* h, int len, double eps, int l, int L, double* mx_out,
                                             double* sum_out) {
    double mx = -INFINITY;
    for (int k = l; k < len; k += L) mx = fmax(mx, h[k] - c[k * stride] / eps);
    for (int o = L >> 1; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    double sum = 0.0;
    for (int k = l; k < len; k += L) sum += exp((h[k] - c[k * stride] / eps) - mx);
    for (int o = L >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    *mx_out = mx;
    *sum_out = sum;
    return -eps * (mx + log(sum));
}

// One workgroup of 1024 threads.  A "row" is one softmin: N rows of f_ba, M of g_ab, N of f_aa, M of g_bb (the last two only with
// debias), each owned by L consecutive lanes (L a power of two, rows * L <= 1024), so one sweep computes all new potentials from
// the old ones.
__global__ __launch_bounds__(1024) void k_sinkhorn_loop(LoopArgs a, int L) {
    extern __shared__ double sm[];
    const int n = a.n, m = a.m, tid = threadIdx.x;
    // potentials (old, new) and the softmin inputs h = log-weight + potential / eps, then the matrices
    double* f_ba = sm;              double* g_ab = f_ba + n;
    double* f_aa = g_ab + m;        double* g_bb = f_aa + n;
    double* nf_ba = g_bb + m;       double* ng_ab = nf_ba + n;
    double* nf_aa = ng_ab + m;      double* ng_bb = nf_aa + n;
    double* hb_ab = ng_bb + m;      /* [m] b_log + g_ab / eps */
    double* ha_ba = hb_ab + m;      /* [n] a_log + f_ba / eps */
    double* ha_aa = ha_ba + n;      /* [n] */
    double* hb_bb = ha_aa + n;      /* [m] */
    double* mats = hb_bb + m;
    const double *c_xy = a.c_xy, *c_xx = a.c_xx, *c_yy = a.c_yy;
    if (a.lds_xy) { for (int i = tid; i < n * m; i += 1024) mats[i] = a.c_xy[i]; c_xy = mats; mats += n * m; }
    if (a.lds_xx) { for (int i = tid; i < n * n; i += 1024) mats[i] = a.c_xx[i]; c_xx = mats; mats += n * n; }
    if (a.lds_yy) { for (int i = tid; i < m * m; i += 1024) mats[i] = a.c_yy[i]; c_yy = mats; }
    const double a_log = -log((double)n), b_log = -log((double)m);

    // row of this thread
    const int rows = a.debias ? 2 * (n + m) : n + m;
    const int row = tid / L, l = tid % L;
    const double* rc = c_xy; const double* rh = g_ab; double* rout = nf_ba;      // rh: the potential a row's softmin reads
    int rstride = 1, rlen = 1, ridx = 0;
    const bool live = row < rows;
    if (live) {
        if (row < n)              { ridx = row;             rc = c_xy + ridx * m; rstride = 1; rlen = m; rh = g_ab; rout = nf_ba; }
        else if (row < n + m)     { ridx = row - n;         rc = c_xy + ridx;     rstride = m; rlen = n; rh = f_ba; rout = ng_ab; }
        else if (row < 2 * n + m) { ridx = row - n - m;     rc = c_xx + ridx * n; rstride = 1; rlen = n; rh = f_aa; rout = nf_aa; }
        else                      { ridx = row - 2 * n - m; rc = c_yy + ridx * m; rstride = 1; rlen = m; rh = g_bb; rout = ng_bb; }
    }

    // start: the softmins of the bare log-weights (zero potentials) at eps_list[0]
    for (int i = tid; i < n; i += 1024) { f_ba[i] = 0.0; f_aa[i] = 0.0; }
    for (int j = tid; j < m; j += 1024) { g_ab[j] = 0.0; g_bb[j] = 0.0; }
    __syncthreads();
    {
        const double eps = a.eps_list[0];
        const double v = softmin_uniform(rc, rstride, rh, live ? rlen : 0, eps, l, L);
        if (live && l == 0) rout[ridx] = v;
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) { f_ba[i] = nf_ba[i]; f_aa[i] = a.debias ? nf_aa[i] : 0.0; }
    for (int j = tid; j < m; j += 1024) { g_ab[j] = ng_ab[j]; g_bb[j] = a.debias ? ng_bb[j] : 0.0; }
    __syncthreads();

    // n_eps averaged steps, then one plain step at the last eps
    for (int it = 0; it <= a.n_eps; ++it) {
        const bool last = it == a.n_eps;
        const double eps = a.eps_list[last ? a.n_eps - 1 : it];
        for (int i = tid; i < n; i += 1024) { ha_ba[i] = a_log + f_ba[i] / eps; ha_aa[i] = a_log + f_aa[i] / eps; }
        for (int j = tid; j < m; j += 1024) { hb_ab[j] = b_log + g_ab[j] / eps; hb_bb[j] = b_log + g_bb[j] / eps; }
        __syncthreads();
        const double v = softmin_uniform(rc, rstride, rh, live ? rlen : 0, eps, l, L);
        if (live && l == 0) rout[ridx] = v;
        __syncthreads();
        if (last) {
            for (int i = tid; i < n; i += 1024) { f_ba[i] = nf_ba[i]; if (a.debias) f_aa[i] = nf_aa[i]; }
            for (int j = tid; j < m; j += 1024) { g_ab[j] = ng_ab[j]; if (a.debias) g_bb[j] = ng_bb[j]; }
        } else {
            for (int i = tid; i < n; i += 1024) { f_ba[i] = 0.5 * (f_ba[i] + nf_ba[i]); if (a.debias) f_aa[i] = 0.5 * (f_aa[i] + nf_aa[i]); }
            for (int j = tid; j < m; j += 1024) { g_ab[j] = 0.5 * (g_ab[j] + ng_ab[j]); if (a.debias) g_bb[j] = 0.5 * (g_bb[j] + ng_bb[j]); }
        }
        __syncthreads();
    }

    for (int i = tid; i < n; i += 1024) { a.f_ba[i] = (float)f_ba[i]; a.f_aa[i] = (float)f_aa[i]; a.h_a[i] = (float)ha_aa[i]; }
    for (int j = tid; j < m; j += 1024) { a.g_ab[j] = (float)g_ab[j]; a.g_bb[j] = (float)g_bb[j]; a.h_b[j] = (float)hb_ab[j]; }
    if (tid < 64) {                                           // loss = mean_i(f_ba - f_aa) + mean_j(g_ab - g_bb)
        double sf = 0.0, sg = 0.0;
        for (int i = tid; i < n; i += 64) sf += f_ba[i] - f_aa[i];
        for (int j = tid; j < m; j += 64) sg += g_ab[j] - g_bb[j];
        sf = wave_sum_d(sf);
        sg = wave_sum_d(sg);
        if (tid == 0) *a.loss = (float)(sf / (double)n + sg / (double)m);
    }

    // Gradient of the last step with its inputs held constant: P = softmax_j(h_b - C_xy / eps), Q = softmax_k(h_a - C_xx / eps);
    // p = 1 divides by the cost (0 where the clamp holds: it has no derivative there).  hb_ab / ha_aa still hold the last step's inputs.
    if (a.wp) {
        const double eps = a.eps_list[a.n_eps - 1];
        const int wrows = a.debias ? 2 * n : n;
        const int LW = L;                                     // 2 n <= rows: the same grouping fits
        const int wr = tid / LW, wl = tid % LW;
        const bool wlive = wr < wrows;
        const bool isq = wr >= n;
        const int i = isq ? wr - n : wr;
        const double* c = wlive ? (isq ? c_xx + i * n : c_xy + i * m) : c_xy;
        const double* h = isq ? ha_aa : hb_ab;
        const int len = wlive ? (isq ? n : m) : 0;
        double mx, sum;
        softmin_row(c, 1, h, len, eps, wl, LW, &mx, &sum);
        float* w = isq ? a.wq + i * n : a.wp + i * m;
        double rs = 0.0;
        for (int k = wl; k < len; k += LW) {
            double v = exp((h[k] - c[k] / eps) - mx) / sum;
            if (a.p == 1) v = c[k] <= 1e-4 ? 0.0 : v / c[k];
            w[k] = (float)v;
            rs += v;
        }
        for (int o = LW >> 1; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
        if (wlive && wl == 0) (isq ? a.rq : a.rp)[i] = (float)rs;
        if (!a.debias) {
            for (int k = tid; k < n * n; k += 1024) a.wq[k] = 0.0;
            for (int k = tid; k < n; k += 1024) a.rq[k] = 0.0;
        }
    }
}

// ----------------------------------------------------------------------------- grad_x = (g / N) * A z
// A[i, :] over z = [x; y]: Wq[i, k] on the x rows (+ rp[i] - rq[i] on k = i), -Wp[i, j] on the y rows.  Workgroup = one chunk of
// columns: the tile of all rows passes through LDS once; wave w owns rows i = w, w + 4, ... (8 at a time in registers), lanes run
// along the columns, so A[i, k] is the same for a whole wave.  k ascends: a fixed order.
template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_combine(const float* __restrict__ x, const float* __restrict__ y, int n, int m, int64_t D,
                                                      const float* __restrict__ wp, const float* __restrict__ wq,
                                                      const float* __restrict__ rp, const float* __restrict__ rq,
                                                      const float* __restrict__ g_out, float* __restrict__ grad) {
    extern __shared__ float tile[];
    const int R = n + m;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float scale = g_out[0] / (float)n;
    const int64_t dbeg = (int64_t)blockIdx.x * SK_CHUNK;
    const int64_t dend = dbeg + SK_CHUNK < D ? dbeg + SK_CHUNK : D;
    for (int64_t d0 = dbeg; d0 < dend; d0 += SK_TW) {
        __syncthreads();
        stage_tile<VEC>(tile, x, y, n, R, D, d0, dend, 6);
        __syncthreads();
        const int64_t col = d0 + lane;
        for (int i0 = w; i0 < n; i0 += 32) {
            float acc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
            for (int k = 0; k < n; ++k) {
                const float zv = tile[k * SK_LD + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + 4 * u;
                    if (i < n) {
                        float aik = wq[i * n + k];
                        if (i == k) aik += rp[i] - rq[i];
                        acc[u] += aik * zv;
                    }
                }
            }
            for (int j = 0; j < m; ++j) {
                const float zv = tile[(n + j) * SK_LD + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + 4 * u;
                    if (i < n) acc[u] -= wp[i * m + j] * zv;
                }
            }
            if (col < dend) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = i0 + 4 * u;
                    if (i < n) grad[(int64_t)i * D + col] = scale * acc[u];
                }
            }
        }
    }
}

// ----------------------------------------------------------------------------- PSNR
// Per block: sum (a - b)^2, min b, max b; one block adds / folds the block partials in index order and writes
// out = {10 log10(range^2 / mse), mse, min, max}.
__global__ __launch_bounds__(256) void k_psnr_part(const float* __restrict__ a, const float* __restrict__ b, int64_t n, int vec,
                                                   float* __restrict__ partials) {
    __shared__ float red[3][4];
    float acc = 0.0f, mn = INFINITY, mx = -INFINITY;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        for (int64_t i = tid; i < n4; i += nthr) {
            const float4 p = a4[i], t = b4[i];
            const float d0 = p.x - t.x, d1 = p.y - t.y, d2 = p.z - t.z, d3 = p.w - t.w;
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
            mn = fminf(fminf(mn, fminf(t.x, t.y)), fminf(t.z, t.w));
            mx = fmaxf(fmaxf(mx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nthr) {
        const float t = b[i], d = a[i] - t;
        acc += d * d;
        mn = fminf(mn, t);
        mx = fmaxf(mx, t);
    }
    acc = wave_sum(acc);
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = mn; red[2][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[3 * blockIdx.x + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partials[3 * blockIdx.x + 1] = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
        partials[3 * blockIdx.x + 2] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    }
}
__global__ __launch_bounds__(64) void k_psnr_final(const float* __restrict__ partials, int np, int64_t n, float data_range,
                                                   float* __restrict__ out) {
    float acc = 0.0f, mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < np; i += 64) {
        acc += partials[3 * i];
        mn = fminf(mn, partials[3 * i + 1]);
        mx = fmaxf(mx, partials[3 * i + 2]);
    }
    acc = wave_sum(acc);
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if (threadIdx.x == 0) {
        const float mse = acc / (float)n;
        const float range = data_range > 0.0f ? data_range : mx - mn;
        out[0] = 10.0f * log10f(range * range / mse);
        out[1] = mse;
        out[2] = mn;
        out[3] = mx;
    }
}

constexpr int PSNR_MAX_BLOCKS = 1024;

int pair_geometry(int64_t n, int64_t m, int* nbr, int* nblk, int* S) {
    const int R = (int)(n + m);
    *nbr = (R + 3) / 4;
    *nblk = *nbr * (*nbr + 1) / 2;
    int s = 64;
    while (s > 1 && *nblk * s > 256) s >>= 1;
    *S = s;
    return (*nblk + (256 / s) - 1) / (256 / s);              // rounds
}

bool sizes_ok(int64_t n, int64_t m, int64_t d) { return n >= 1 && m >= 1 && n <= SK_MAXN && m <= SK_MAXN && d >= 1; }

bool rows_aligned(const float* x, const float* y, int64_t d) { return d % 4 == 0 && ((((uintptr_t)x | (uintptr_t)y) & 15) == 0); }

}  // namespace

extern "C" int64_t rho_sinkhorn_max_samples(void) { return SK_MAXN; }

extern "C" int64_t rho_pairwise_cost_workspace_bytes(int64_t n, int64_t m, int64_t d) {
    if (!sizes_ok(n, m, d)) return -1;
    const int64_t R = n + m, nchunks = (d + SK_CHUNK - 1) / SK_CHUNK;
    const int64_t pair = nchunks * (R * (R + 1) / 2), diam = (d + 1023) / 1024;
    return 8 * (pair > diam ? pair : diam);
}

extern "C" int rho_pairwise_cost(const float* x, const float* y, int64_t n, int64_t m, int64_t d, int p, float* c_xy, float* c_xx,
                                 float* c_yy, double* c64, double* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !y || !c_xy || !c_xx || !c_yy || !workspace || (p != 1 && p != 2)) return RHO_E_ARG;
    if (!sizes_ok(n, m, d)) return RHO_E_SHAPE;
    if (workspace_bytes < rho_pairwise_cost_workspace_bytes(n, m, d)) return RHO_E_ARG;
    const int64_t nchunks = (d + SK_CHUNK - 1) / SK_CHUNK;
    if (nchunks > 65535) return RHO_E_SHAPE;                  // D <= 33 553 920
    int nbr, nblk, S;
    const int rounds = pair_geometry(n, m, &nbr, &nblk, &S);
    const int R = (int)(n + m);
    int tw_log2 = 9;                                           // 512, 256, 128 or 64 columns per step: about 32 KB of LDS, <= 66 560 bytes
    while (tw_log2 > 6 && (size_t)R * ((1 << tw_log2) + 1) * sizeof(float) > 36 * 1024) --tw_log2;
    const size_t lds = (size_t)R * ((1 << tw_log2) + 1) * sizeof(float);
    const dim3 grid((unsigned)rounds, (unsigned)nchunks);
    if (rows_aligned(x, y, d)) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_part<true>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 256 * SK_LD * 4);
        if (attr != hipSuccess) return (int)attr;
        hipLaunchKernelGGL(k_pair_part<true>, grid, dim3(256), lds, as_stream(stream), x, y, (int)n, R, d, nbr, nblk, S, tw_log2, workspace);
    } else {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_part<false>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 256 * SK_LD * 4);
        if (attr != hipSuccess) return (int)attr;
        hipLaunchKernelGGL(k_pair_part<false>, grid, dim3(256), lds, as_stream(stream), x, y, (int)n, R, d, nbr, nblk, S, tw_log2, workspace);
    }
    const int64_t n_out = n * m + n * n + m * m;
    hipLaunchKernelGGL(k_pair_final, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, as_stream(stream), workspace, (int)nchunks, (int)n,
                       (int)m, p, c_xy, c_xx, c_yy, c64);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_max_diameter(const float* x, const float* y, int64_t n, int64_t m, int64_t d, double* out, double* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (!x || !y || !out || !workspace) return RHO_E_ARG;
    if (!sizes_ok(n, m, d)) return RHO_E_SHAPE;
    const int64_t np = (d + 1023) / 1024;
    if (workspace_bytes < 8 * np || np > 0x7FFFFFFF) return RHO_E_ARG;
    hipLaunchKernelGGL(k_diam_part, dim3((unsigned)np), dim3(256), 0, as_stream(stream), x, y, (int)n, (int)(n + m), d, workspace);
    hipLaunchKernelGGL(k_diam_final, dim3(1), dim3(256), 0, as_stream(stream), workspace, (int)np, out);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_sinkhorn_loop(const double* c_xy, const double* c_xx, const double* c_yy, int64_t n, int64_t m, const double* eps_list,
                                 int64_t n_eps, int p, int debias, float* f_ba, float* g_ab, float* f_aa, float* g_bb, float* h_b,
                                 float* h_a, float* loss, float* wp, float* wq, float* rp, float* rq, void* stream) {
    if (!c_xy || !c_xx || !c_yy || !eps_list || n_eps < 1 || n_eps > 0x7FFFFFFF || (p != 1 && p != 2) || !f_ba || !g_ab || !f_aa ||
        !g_bb || !h_b || !h_a || !loss)
        return RHO_E_ARG;
    if ((wp || wq || rp || rq) && !(wp && wq && rp && rq)) return RHO_E_ARG;
    if (!sizes_ok(n, m, 1)) return RHO_E_SHAPE;
    LoopArgs a;
    a.c_xy = c_xy; a.c_xx = c_xx; a.c_yy = c_yy; a.eps_list = eps_list;
    a.n_eps = (int)n_eps; a.n = (int)n; a.m = (int)m; a.debias = debias ? 1 : 0; a.p = p;
    a.f_ba = f_ba; a.g_ab = g_ab; a.f_aa = f_aa; a.g_bb = g_bb; a.h_b = h_b; a.h_a = h_a; a.loss = loss;
    a.wp = wp; a.wq = wq; a.rp = rp; a.rq = rq;
    // LDS: 12 vectors, then the matrices in the order xy, xx, yy while they fit under the 160 KiB one workgroup may declare
    const size_t cap = 160 * 1024;
    size_t lds = (size_t)6 * (n + m) * sizeof(double);
    a.lds_xy = a.lds_xx = a.lds_yy = 0;
    if (lds + (size_t)n * m * 8 <= cap) { a.lds_xy = 1; lds += (size_t)n * m * 8; }
    if (a.debias && lds + (size_t)n * n * 8 <= cap) { a.lds_xx = 1; lds += (size_t)n * n * 8; }
    if (a.debias && lds + (size_t)m * m * 8 <= cap) { a.lds_yy = 1; lds += (size_t)m * m * 8; }
    const int rows = (int)(a.debias ? 2 * (n + m) : n + m);
    int L = 64;
    while (L > 1 && rows * L > 1024) L >>= 1;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_sinkhorn_loop),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
    if (attr != hipSuccess) return (int)attr;
    hipLaunchKernelGGL(k_sinkhorn_loop, dim3(1), dim3(1024), lds, as_stream(stream), a, L);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_rows_combine(const float* x, const float* y, int64_t n, int64_t m, int64_t d, const float* wp, const float* wq,
                                const float* rp, const float* rq, const float* g_out, float* grad_x, void* stream) {
    if (!x || !y || !wp || !wq || !rp || !rq || !g_out || !grad_x) return RHO_E_ARG;
    if (!sizes_ok(n, m, d)) return RHO_E_SHAPE;
    const int64_t nchunks = (d + SK_CHUNK - 1) / SK_CHUNK;
    if (nchunks > 0x7FFFFFFF) return RHO_E_SHAPE;
    const size_t lds = (size_t)(n + m) * SK_LD * sizeof(float);
    if (rows_aligned(x, y, d)) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rows_combine<true>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 256 * SK_LD * 4);
        if (attr != hipSuccess) return (int)attr;
        hipLaunchKernelGGL(k_rows_combine<true>, dim3((unsigned)nchunks), dim3(256), lds, as_stream(stream), x, y, (int)n, (int)m, d, wp,
                           wq, rp, rq, g_out, grad_x);
    } else {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_rows_combine<false>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 256 * SK_LD * 4);
        if (attr != hipSuccess) return (int)attr;
        hipLaunchKernelGGL(k_rows_combine<false>, dim3((unsigned)nchunks), dim3(256), lds, as_stream(stream), x, y, (int)n, (int)m, d,
                           wp, wq, rp, rq, g_out, grad_x);
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t rho_psnr_workspace_bytes(void) { return (int64_t)PSNR_MAX_BLOCKS * 3 * sizeof(float); }

extern "C" int rho_psnr(const float* pred, const float* target, int64_t n, float data_range, float* out, float* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (!pred || !target || !out || !workspace || n <= 0 || workspace_bytes < rho_psnr_workspace_bytes()) return RHO_E_ARG;
    int64_t g = (n + 256 * 8 - 1) / (256 * 8);
    if (g > PSNR_MAX_BLOCKS) g = PSNR_MAX_BLOCKS;
    const int vec = ((((uintptr_t)pred | (uintptr_t)target) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_psnr_part, dim3((unsigned)g), dim3(256), 0, as_stream(stream), pred, target, n, vec, workspace);
    hipLaunchKernelGGL(k_psnr_final, dim3(1), dim3(64), 0, as_stream(stream), workspace, (int)g, n, data_range, out);
    RHO_LAUNCH_CHECK();
    return 0;
}
