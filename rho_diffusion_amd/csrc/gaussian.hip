// GaussianDiffusionPipeline beyond the fixed DDIM path (rho_diffusion/diffusion/gaussian_diffusion.py:277-1009, guided-diffusion):
// the per-step arithmetic of p_mean_variance / p_sample (ancestral), ddim_sample with eta / condition_score, ddim_reverse_sample,
// the variational bound (_vb_terms_bpd, _prior_bpd) and the metrics of rho_diffusion/metrics/losses.py.
//
// Every kernel gathers per-sample rows of one packed float32 table [RHO_GD_ROWS, table_len] (the float64 tables of the pipeline
// cast to float32, as _extract_into_tensor does) at t[b]; a t[b] outside [0, table_len) sets *err_flag |= 4 and reads the clamped
// row, as rho_q_sample_coef.  The step kernels run a (chunks, batch) grid: the table row is uniform per workgroup, so the per-sample
// coefficients are evaluated once per thread, not per element.  The per-sample reductions are two-stage and fixed-order (double
// partials per workgroup in a workspace, then one workgroup per sample adds them in index order): no float atomics, results are
// bit-reproducible, and a sample is split across enough workgroups that a batch of 2 still fills the GPU.
#include "common.h"

// float32 tensor expressions of the reference restated op by op, each rounding once (see select.hip)
#pragma clang fp contract(off)

namespace {

constexpr int GD_THREADS = 256;
constexpr int GD_TARGET_WGS = 2048;     // >= 8 workgroups per CU of the 256 for any batch (as long as a sample has that many elements)

// workgroups per sample: enough for GD_TARGET_WGS in all, no more than one per GD_THREADS elements
__host__ __device__ inline int64_t gd_chunks(int64_t batch, int64_t per_sample) {
    int64_t g = (GD_TARGET_WGS + batch - 1) / batch;
    const int64_t cap = (per_sample + GD_THREADS - 1) / GD_THREADS;
    if (g > cap) g = cap;
    if (g > 65535) g = 65535;
    return g < 1 ? 1 : g;
}

__device__ __forceinline__ int64_t gd_row_index(const int64_t* __restrict__ t, int b, int64_t len, int32_t* err_flag) {
    int64_t tb = t[b];
    if (tb < 0 || tb >= len) {                     // the reference's table gather raises IndexError
        if (err_flag != nullptr && threadIdx.x == 0) atomicOr(err_flag, 4);
        tb = tb < 0 ? 0 : len - 1;
    }
    return tb;
}

__device__ __forceinline__ float gd_tab(const float* __restrict__ tab, int64_t len, int row, int64_t tb) { return tab[(int64_t)row * len + tb]; }

// dynamic thresholding (:400-415): s = max(q, 1); clamp(x0, -s, s) / s
__device__ __forceinline__ float gd_threshold(float x0, float s) { return fminf(fmaxf(x0, -s), s) / s; }

// approx_standard_normal_cdf (metrics/losses.py:56-61): 0.5 * (1 + tanh(sqrt(2/pi) * (x + 0.044715 * x^3))), x^3 = (x*x)*x as ATen's pow
__device__ __forceinline__ float gd_cdf(float x) {
    const float x3 = (x * x) * x;
    const float p = 0.044715f * x3;
    const float u = x + p;
    const float v = 0.7978845608028654f * u;
    return 0.5f * (1.0f + tanhf(v));
}

// discretized_gaussian_log_likelihood (metrics/losses.py:64-93), one element
__device__ __forceinline__ float gd_dgll(float x, float mean, float log_scale) {
    const float centered = x - mean;
    const float inv_stdv = expf(-log_scale);
    const float bin = (float)(1.0 / 255.0);
    const float plus_in = inv_stdv * (centered + bin);
    const float cdf_plus = gd_cdf(plus_in);
    const float min_in = inv_stdv * (centered - bin);
    const float cdf_min = gd_cdf(min_in);
    if (x < -0.999f) return logf(fmaxf(cdf_plus, 1e-12f));
    if (x > 0.999f) return logf(fmaxf(1.0f - cdf_min, 1e-12f));
    return logf(fmaxf(cdf_plus - cdf_min, 1e-12f));
}

// normal_kl (metrics/losses.py:28-53): 0.5 * (-1 + lv2 - lv1 + exp(lv1 - lv2) + (m1 - m2)^2 * exp(-lv2)), left to right, in two parts:
// the log-variance terms (with a fixed variance uniform per sample: evaluated once per thread) and the per-element remainder
struct GdKlTerms {
    float e2, k0;                // exp(-lv2);  ((-1 + lv2) - lv1) + exp(lv1 - lv2)
};

__device__ __forceinline__ GdKlTerms gd_kl_terms(float lv1, float lv2) { return {expf(-lv2), ((-1.0f + lv2) - lv1) + expf(lv1 - lv2)}; }

__device__ __forceinline__ float gd_kl_elem(const GdKlTerms& k, float m1, float m2) {
    const float d = m1 - m2;
    const float q = (d * d) * k.e2;
    return 0.5f * (k.k0 + q);
}

__device__ __forceinline__ float gd_normal_kl(float m1, float lv1, float m2, float lv2) { return gd_kl_elem(gd_kl_terms(lv1, lv2), m1, m2); }

// What a thread of the step kernels knows of its sample: the launch's modes and the rows of the table at t[b], gathered once per thread.
// LV (learned variance) reads max_log where a fixed variance reads its model_var / model_logvar rows; a kernel gathers further rows of
// its own at tb.
struct GdCoef {
    int eps_mode, range;        // the model predicts epsilon (else x0);  LEARNED_RANGE (else LEARNED)
    int64_t tb;                 // the clamped row index
    bool t0;                    // t[b] == 0: no noise, and the VLB takes the decoder NLL
    float sr, srm1, c1, c2;     // sqrt_recip, sqrt_recipm1, posterior mean coef1 / coef2
    float post_logvar;          // the true posterior's log-variance; min_log of LEARNED_RANGE
    float var, logvar;          // fixed variance
    float max_log;              // learned variance
};

template <bool LV>
__device__ __forceinline__ GdCoef gd_coef(const int64_t* __restrict__ t, const float* __restrict__ tab, int64_t len, int b, int eps_mode,
                                          int range, int32_t* err_flag) {
    GdCoef c = {};
    c.eps_mode = eps_mode;
    c.range = range;
    c.tb = gd_row_index(t, b, len, err_flag);
    c.t0 = t[b] == 0;
    c.sr = gd_tab(tab, len, RHO_GD_SQRT_RECIP, c.tb);
    c.srm1 = gd_tab(tab, len, RHO_GD_SQRT_RECIPM1, c.tb);
    c.c1 = gd_tab(tab, len, RHO_GD_COEF1, c.tb);
    c.c2 = gd_tab(tab, len, RHO_GD_COEF2, c.tb);
    c.post_logvar = gd_tab(tab, len, RHO_GD_POST_LOGVAR, c.tb);
    if constexpr (LV) {
        c.max_log = gd_tab(tab, len, RHO_GD_LOG_BETA, c.tb);
    } else {
        c.var = gd_tab(tab, len, RHO_GD_MODEL_VAR, c.tb);
        c.logvar = gd_tab(tab, len, RHO_GD_MODEL_LOGVAR, c.tb);
    }
    return c;
}

// x0 from the model output: START_X as is; EPSILON _predict_xstart_from_eps (:445-450): sqrt_recip * x - sqrt_recipm1 * eps
__device__ __forceinline__ float gd_x0(const GdCoef& c, float x, float m) {
    if (!c.eps_mode) return m;
    const float p0 = c.sr * x, p1 = c.srm1 * m;
    return p0 - p1;
}

// learned variances (:368-383), per element, float32 in the reference's order:
//   LEARNED:        logvar = v
//   LEARNED_RANGE:  frac = (v + 1) / 2;  logvar = frac*max_log + (1 - frac)*min_log   (max_log = log(betas), min_log = post_logvar)
__device__ __forceinline__ float gd_learned_logvar(const GdCoef& c, float v) {
    if (!c.range) return v;
    const float frac = (v + 1.0f) / 2.0f;
    const float p0 = frac * c.max_log, p1 = (1.0f - frac) * c.post_logvar;
    return p0 + p1;
}

__device__ __forceinline__ double gd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order workgroup sum of K doubles per thread; the result is valid in thread 0
template <int K>
__device__ __forceinline__ void gd_block_sum(double (&acc)[K]) {
    __shared__ double red[GD_THREADS / 64][K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = gd_wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wv][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double s = red[0][k];
            for (int w = 1; w < GD_THREADS / 64; ++w) s += red[w][k];
            acc[k] = s;
        }
    }
}

// stage 2: one workgroup per sample adds its chunks' partials (ws[b][chunk][K]) in index order
template <int K>
__device__ __forceinline__ void gd_sum_partials(const double* __restrict__ ws, int64_t chunks, int b, double (&acc)[K]) {
    const double* p = ws + (int64_t)b * chunks * K;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int64_t c = threadIdx.x; c < chunks; c += GD_THREADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += p[c * K + k];
    }
    gd_block_sum<K>(acc);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- affine helpers
// out = a[t]*x (op 0) | a[t]*x + b[t]*y (1) | a[t]*x - b[t]*y (2) | (a[t]*x - y) / b[t] (3)
__global__ __launch_bounds__(GD_THREADS) void k_gd_affine(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                                                          const int64_t* __restrict__ t, const float* __restrict__ tab, int64_t len, int row_a,
                                                          int row_b, int op, int64_t n, int32_t* err_flag) {
    const int b = blockIdx.y;
    const int64_t tb = gd_row_index(t, b, len, err_flag);
    const float a = gd_tab(tab, len, row_a, tb);
    const float c = op == 0 ? 0.0f : gd_tab(tab, len, row_b, tb);
    const float* xb = x + (int64_t)b * n;
    const float* yb = y + (int64_t)b * n;
    float* ob = out + (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float p0 = a * xb[i];
        float v;
        if (op == 0) {
            v = p0;
        } else if (op == 3) {
            v = (p0 - yb[i]) / c;
        } else {
            const float p1 = c * yb[i];
            v = op == 1 ? p0 + p1 : p0 - p1;
        }
        ob[i] = v;
    }
}

extern "C" int rho_gd_affine(const float* x, const float* y, float* out, const int64_t* t, const float* tab, int64_t table_len, int row_a,
                             int row_b, int op, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    if (!x || !out || !t || !tab || batch <= 0 || per_sample <= 0 || table_len <= 0 || op < 0 || op > 3) return RHO_E_ARG;
    if (op != 0 && !y) return RHO_E_ARG;
    if (row_a < 0 || row_a >= RHO_GD_ROWS || (op != 0 && (row_b < 0 || row_b >= RHO_GD_ROWS))) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    dim3 grid((unsigned)gd_chunks(batch, per_sample), (unsigned)batch);
    hipLaunchKernelGGL(k_gd_affine, grid, dim3(GD_THREADS), 0, as_stream(stream), x, op == 0 ? x : y, out, t, tab, table_len, row_a,
                       row_b, op, per_sample, err_flag);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- posterior / ancestral
// p_mean_variance (:338-443) + condition_mean (:473-486) + p_sample (:512-556):
//   x0 = START_X ? m : sqrt_recip*x - sqrt_recipm1*m;  thresholded when quantile != NULL
//   mean = coef1*x0 + coef2*x  (+ variance*grad)  (+ ((t != 0) * exp(0.5*logvar)) * noise)
// Sample b's model output (or x0) is read at mo + b*mo_stride.  A fixed variance (LV = false) takes variance and log-variance from the
// table, once per thread.  A learned one (:368-383) evaluates them per element from the variance values at vv + b*v_stride (for a
// [B, 2C, ...] output read in place: the same base + C*S, both strides 2*C*S) and can write them out; every output is optional there.
template <bool LV>
__global__ __launch_bounds__(GD_THREADS) void k_gd_posterior(const float* __restrict__ xt, const float* __restrict__ mo, int64_t mo_stride,
                                                             const float* __restrict__ vv, int64_t v_stride, const int64_t* __restrict__ t,
                                                             const float* __restrict__ tab, int64_t len, int eps_mode, int range,
                                                             const float* __restrict__ quant, const float* __restrict__ grad,
                                                             const float* __restrict__ noise, float* __restrict__ out,
                                                             float* __restrict__ pred_x0, float* __restrict__ var_out,
                                                             float* __restrict__ logvar_out, int64_t n, int32_t* err_flag) {
    const int b = blockIdx.y;
    const GdCoef c = gd_coef<LV>(t, tab, len, b, eps_mode, range, err_flag);
    const float nmask = c.t0 ? 0.0f : 1.0f;
    const float half_lv = 0.5f * c.logvar;
    const float nstd = nmask * expf(half_lv);
    const float s = quant != nullptr ? fmaxf(quant[b], 1.0f) : 1.0f;
    const int64_t off = (int64_t)b * n;
    const float* mob = mo + (int64_t)b * mo_stride - off;
    const float* vb = LV ? vv + (int64_t)b * v_stride - off : nullptr;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float x = xt[i];
        float x0 = gd_x0(c, x, mob[i]);
        if (quant != nullptr) x0 = gd_threshold(x0, s);
        float lv = c.logvar;
        if constexpr (LV) lv = gd_learned_logvar(c, vb[i]);
        const float p0 = c.c1 * x0, p1 = c.c2 * x;
        float v = p0 + p1;
        if (grad != nullptr) {
            const float p2 = (LV ? expf(lv) : c.var) * grad[i];
            v = v + p2;
        }
        if (noise != nullptr) {
            const float h = 0.5f * lv;
            const float p3 = (LV ? nmask * expf(h) : nstd) * noise[i];
            v = v + p3;
        }
        if (!LV || out != nullptr) out[i] = v;
        if (pred_x0 != nullptr) pred_x0[i] = x0;
        if constexpr (LV) {
            if (var_out != nullptr) var_out[i] = expf(lv);
            if (logvar_out != nullptr) logvar_out[i] = lv;
        }
    }
}

namespace {
bool gd_mean_ok(int mean_type) { return mean_type == RHO_GD_START_X || mean_type == RHO_GD_EPSILON; }
bool gd_lv_ok(int mean_type, int var_type) { return gd_mean_ok(mean_type) && (var_type == RHO_GD_LEARNED || var_type == RHO_GD_LEARNED_RANGE); }
}  // namespace

extern "C" int rho_gd_posterior_step(const float* x_t, const float* model_out, const int64_t* t, const float* tab, int64_t table_len,
                                     int mean_type, const float* quantile, const float* grad, const float* noise, float* out,
                                     float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    if (!x_t || !model_out || !t || !tab || !out || batch <= 0 || per_sample <= 0 || table_len <= 0) return RHO_E_ARG;
    if (!gd_mean_ok(mean_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    dim3 grid((unsigned)gd_chunks(batch, per_sample), (unsigned)batch);
    hipLaunchKernelGGL(k_gd_posterior<false>, grid, dim3(GD_THREADS), 0, as_stream(stream), x_t, model_out, per_sample, nullptr, 0, t, tab,
                       table_len, mean_type == RHO_GD_EPSILON ? 1 : 0, 0, quantile, grad, noise, out, pred_xstart, nullptr, nullptr, per_sample,
                       err_flag);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_gd_posterior_step_lv(const float* x_t, const float* model_out, int64_t mean_stride, const float* var_values,
                                        int64_t var_stride, const int64_t* t, const float* tab, int64_t table_len, int mean_type, int var_type,
                                        const float* quantile, const float* grad, const float* noise, float* out, float* pred_xstart,
                                        float* variance, float* log_variance, int64_t batch, int64_t per_sample, int32_t* err_flag,
                                        void* stream) {
    if (!x_t || !model_out || !var_values || !t || !tab || batch <= 0 || per_sample <= 0 || table_len <= 0) return RHO_E_ARG;
    if (!out && !pred_xstart && !variance && !log_variance) return RHO_E_ARG;
    if (mean_stride < per_sample || var_stride < per_sample || !gd_lv_ok(mean_type, var_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    dim3 grid((unsigned)gd_chunks(batch, per_sample), (unsigned)batch);
    hipLaunchKernelGGL(k_gd_posterior<true>, grid, dim3(GD_THREADS), 0, as_stream(stream), x_t, model_out, mean_stride, var_values, var_stride,
                       t, tab, table_len, mean_type == RHO_GD_EPSILON ? 1 : 0, var_type == RHO_GD_LEARNED_RANGE ? 1 : 0, quantile, grad,
                       noise, out, pred_xstart, variance, log_variance, per_sample, err_flag);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- DDIM, per-sample t
// ddim_sample (:654-702) with condition_score (:488-510), or ddim_reverse_sample (:704-740):
//   x0 as k_gd_posterior;  with grad: eps = (sr*x - x0)/srm1;  eps = eps - sqrt(1 - abar)*g;  x0 = sr*x - srm1*eps
//   eps = (sr*x - x0) / srm1
//   forward: sigma = eta * sqrt((1 - abar_prev)/(1 - abar)) * sqrt(1 - abar/abar_prev)
//            sample = x0*sqrt(abar_prev) + sqrt(1 - abar_prev - sigma^2)*eps  (+ ((t != 0) * sigma) * noise)
//   reverse: sample = x0*sqrt(abar_next) + sqrt(1 - abar_next)*eps
__global__ __launch_bounds__(GD_THREADS) void k_gd_ddim(const float* __restrict__ xt, const float* __restrict__ mo, const int64_t* __restrict__ t,
                                                        const float* __restrict__ tab, int64_t len, int eps_mode, const float* __restrict__ quant,
                                                        const float* __restrict__ grad, const float* __restrict__ noise, float eta, int reverse,
                                                        float* __restrict__ sample, float* __restrict__ pred_x0, int64_t n, int64_t mo_stride,
                                                        int32_t* err_flag) {
    const int b = blockIdx.y;
    const GdCoef c = gd_coef<false>(t, tab, len, b, eps_mode, 0, err_flag);
    const float sr = c.sr, srm1 = c.srm1;
    const float ab = gd_tab(tab, len, RHO_GD_ABAR, c.tb);
    const float sq1mab = sqrtf(1.0f - ab);
    float c_x0, c_eps, msig = 0.0f;
    if (reverse) {
        const float abn = gd_tab(tab, len, RHO_GD_ABAR_NEXT, c.tb);
        c_x0 = sqrtf(abn);
        c_eps = sqrtf(1.0f - abn);
    } else {
        const float abp = gd_tab(tab, len, RHO_GD_ABAR_PREV, c.tb);
        float sigma = eta * sqrtf((1.0f - abp) / (1.0f - ab));
        sigma = sigma * sqrtf(1.0f - ab / abp);
        c_x0 = sqrtf(abp);
        c_eps = sqrtf((1.0f - abp) - sigma * sigma);
        msig = (c.t0 ? 0.0f : 1.0f) * sigma;
    }
    const float s = quant != nullptr ? fmaxf(quant[b], 1.0f) : 1.0f;
    const int64_t off = (int64_t)b * n;
    const float* mob = mo + (int64_t)b * mo_stride - off;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float x = xt[i];
        float x0 = gd_x0(c, x, mob[i]);
        if (quant != nullptr) x0 = gd_threshold(x0, s);
        const float ax = sr * x;
        if (grad != nullptr) {
            float e = (ax - x0) / srm1;
            const float pg = sq1mab * grad[i];
            e = e - pg;
            const float pe = srm1 * e;
            x0 = ax - pe;
        }
        const float eps = (ax - x0) / srm1;
        const float p0 = x0 * c_x0, p1 = c_eps * eps;
        float v = p0 + p1;
        if (noise != nullptr) {
            const float p2 = msig * noise[i];
            v = v + p2;
        }
        sample[i] = v;
        if (pred_x0 != nullptr) pred_x0[i] = x0;
    }
}

namespace {
int gd_ddim_step(const float* x_t, const float* model_out, int64_t model_stride, const int64_t* t, const float* tab, int64_t table_len,
                 int mean_type, const float* quantile, const float* grad, const float* noise, float eta, int reverse, float* sample,
                 float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    if (!x_t || !model_out || !t || !tab || !sample || batch <= 0 || per_sample <= 0 || table_len <= 0) return RHO_E_ARG;
    if (model_stride < per_sample || !gd_mean_ok(mean_type)) return RHO_E_ARG;
    if (reverse && (eta != 0.0f || noise || grad)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    dim3 grid((unsigned)gd_chunks(batch, per_sample), (unsigned)batch);
    hipLaunchKernelGGL(k_gd_ddim, grid, dim3(GD_THREADS), 0, as_stream(stream), x_t, model_out, t, tab, table_len,
                       mean_type == RHO_GD_EPSILON ? 1 : 0, quantile, grad, noise, eta, reverse, sample, pred_xstart, per_sample, model_stride,
                       err_flag);
    RHO_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int rho_gd_ddim_step(const float* x_t, const float* model_out, const int64_t* t, const float* tab, int64_t table_len,
                                int mean_type, const float* quantile, const float* grad, const float* noise, float eta, int reverse,
                                float* sample, float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    return gd_ddim_step(x_t, model_out, per_sample, t, tab, table_len, mean_type, quantile, grad, noise, eta, reverse, sample, pred_xstart,
                        batch, per_sample, err_flag, stream);
}

// the same reading sample b's model output at model_out + b*model_stride: the mean half of a learned-variance [B, 2C, ...] output in
// place (model_stride = 2*per_sample); DDIM ignores the variance half, as the reference does
extern "C" int rho_gd_ddim_step_strided(const float* x_t, const float* model_out, int64_t model_stride, const int64_t* t, const float* tab,
                                        int64_t table_len, int mean_type, const float* quantile, const float* grad, const float* noise,
                                        float eta, int reverse, float* sample, float* pred_xstart, int64_t batch, int64_t per_sample,
                                        int32_t* err_flag, void* stream) {
    return gd_ddim_step(x_t, model_out, model_stride, t, tab, table_len, mean_type, quantile, grad, noise, eta, reverse, sample, pred_xstart,
                        batch, per_sample, err_flag, stream);
}

// ---------------------------------------------------------------------------------------------------------------- variational bound
// _vb_terms_bpd (:826-859) + the per-step statistics of calc_bpd_loop (:936-1009), or _prior_bpd (:936-951).  Stage 1 per element:
//   x0 (model output, thresholded), true mean coef1*x_start + coef2*x_t, model mean coef1*x0 + coef2*x_t,
//   kl  = normal_kl(true_mean, post_logvar, model_mean, model_logvar)
//   nll = -discretized_gaussian_log_likelihood(x_start, model_mean, 0.5*model_logvar)
//   (x0 - x_start)^2,  ((sr*x_t - x0)/srm1 - noise)^2
// prior: normal_kl(sqrt_abar[T-1]*x_start, log(1-abar)[T-1], 0, 0).  Partials ws[b][chunk][4] in double.
// The model output and, with a learned variance (LV), the variance values are read per sample as in k_gd_posterior; a fixed variance
// evaluates the KL's log-variance terms and the NLL's log-scale once per thread, a learned one per element.
constexpr int GD_VLB_K = 4;

// workgroup sum of the partials, written to ws[b][chunk][:]
__device__ __forceinline__ void gd_vlb_store(double (&acc)[GD_VLB_K], double* __restrict__ ws) {
    gd_block_sum<GD_VLB_K>(acc);
    if (threadIdx.x == 0) {
        double* w = ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * GD_VLB_K;
#pragma unroll
        for (int k = 0; k < GD_VLB_K; ++k) w[k] = acc[k];
    }
}

template <bool LV>
__global__ __launch_bounds__(GD_THREADS) void k_gd_vlb_partial(const float* __restrict__ xs, const float* __restrict__ xt,
                                                               const float* __restrict__ mo, int64_t mo_stride, const float* __restrict__ vv,
                                                               int64_t v_stride, const int64_t* __restrict__ t, const float* __restrict__ tab,
                                                               int64_t len, int eps_mode, int range, const float* __restrict__ quant,
                                                               const float* __restrict__ noise, float* __restrict__ pred_x0,
                                                               double* __restrict__ ws, int64_t n, int32_t* err_flag) {
    const int b = blockIdx.y;
    double acc[GD_VLB_K] = {0.0, 0.0, 0.0, 0.0};
    const GdCoef c = gd_coef<LV>(t, tab, len, b, eps_mode, range, err_flag);
    GdKlTerms kl = gd_kl_terms(c.post_logvar, c.logvar);
    float log_scale = 0.5f * c.logvar;
    const float s = quant != nullptr ? fmaxf(quant[b], 1.0f) : 1.0f;
    const int64_t off = (int64_t)b * n;
    const float* mob = mo + (int64_t)b * mo_stride - off;
    const float* vb = LV ? vv + (int64_t)b * v_stride - off : nullptr;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float x = xt[i], x_start = xs[i];
        float x0 = gd_x0(c, x, mob[i]);
        if (quant != nullptr) x0 = gd_threshold(x0, s);
        if (pred_x0 != nullptr) pred_x0[i] = x0;
        if constexpr (LV) {
            const float lv2 = gd_learned_logvar(c, vb[i]);
            kl = gd_kl_terms(c.post_logvar, lv2);
            log_scale = 0.5f * lv2;
        }
        const float cx = c.c2 * x;
        const float tm = (c.c1 * x_start) + cx;
        const float mm = (c.c1 * x0) + cx;
        acc[0] += (double)gd_kl_elem(kl, tm, mm);
        acc[1] -= (double)gd_dgll(x_start, mm, log_scale);
        const float dx = x0 - x_start;
        acc[2] += (double)(dx * dx);
        if (noise != nullptr) {
            const float eps = ((c.sr * x) - x0) / c.srm1;
            const float de = eps - noise[i];
            acc[3] += (double)(de * de);
        }
    }
    gd_vlb_store(acc, ws);
}

// _prior_bpd: the KL of q(x_{T-1} | x_0) against N(0, 1); it reads the last table column and none of a step's inputs
__global__ __launch_bounds__(GD_THREADS) void k_gd_prior_partial(const float* __restrict__ xs, const float* __restrict__ tab, int64_t len,
                                                                 double* __restrict__ ws, int64_t n) {
    double acc[GD_VLB_K] = {0.0, 0.0, 0.0, 0.0};
    const float sa = gd_tab(tab, len, RHO_GD_SQRT_ABAR, len - 1);
    const GdKlTerms kl = gd_kl_terms(gd_tab(tab, len, RHO_GD_LOG_1M_ABAR, len - 1), 0.0f);
    const int64_t off = (int64_t)blockIdx.y * n;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS)
        acc[0] += (double)gd_kl_elem(kl, sa * xs[i], 0.0f);
    gd_vlb_store(acc, ws);
}

// stage 2: per sample means (float32, as mean_flat returns them) / ln 2; vb = where(t == 0, nll, kl)
__global__ __launch_bounds__(GD_THREADS) void k_gd_vlb_final(const double* __restrict__ ws, int64_t chunks, const int64_t* __restrict__ t,
                                                             int prior, int64_t n, float* __restrict__ vb, float* __restrict__ xstart_mse,
                                                             float* __restrict__ mse, int64_t out_stride, float* __restrict__ raw_kl,
                                                             float* __restrict__ raw_nll) {
    const int b = blockIdx.x;
    double acc[GD_VLB_K];
    gd_sum_partials<GD_VLB_K>(ws, chunks, b, acc);
    if (threadIdx.x != 0) return;
    const float ln2 = (float)0.69314718055994530942;
    const float kl = (float)(acc[0] / (double)n) / ln2;
    if (prior) {
        vb[(int64_t)b * out_stride] = kl;
        return;
    }
    const float nll = (float)(acc[1] / (double)n) / ln2;
    vb[(int64_t)b * out_stride] = t[b] == 0 ? nll : kl;
    if (xstart_mse != nullptr) xstart_mse[(int64_t)b * out_stride] = (float)(acc[2] / (double)n);
    if (mse != nullptr) mse[(int64_t)b * out_stride] = (float)(acc[3] / (double)n);
    if (raw_kl != nullptr) raw_kl[b] = kl;
    if (raw_nll != nullptr) raw_nll[b] = nll;
}

extern "C" int64_t rho_gd_reduce_workspace_bytes(int64_t batch, int64_t per_sample) {
    if (batch <= 0 || per_sample <= 0) return 0;
    return batch * gd_chunks(batch, per_sample) * GD_VLB_K * (int64_t)sizeof(double);
}

extern "C" int rho_gd_vlb_terms(const float* x_start, const float* x_t, const float* model_out, const int64_t* t, const float* tab,
                                int64_t table_len, int mean_type, const float* quantile, const float* noise, int prior, float* vb,
                                float* xstart_mse, float* mse, int64_t out_stride, float* raw_kl, float* raw_nll, float* pred_xstart,
                                void* workspace, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    if (!x_start || !tab || !vb || !workspace || batch <= 0 || per_sample <= 0 || table_len <= 0 || out_stride < 1) return RHO_E_ARG;
    if (!prior && (!x_t || !model_out || !t || (mse && !noise))) return RHO_E_ARG;
    if (!gd_mean_ok(mean_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    const int64_t chunks = gd_chunks(batch, per_sample);
    const dim3 grid((unsigned)chunks, (unsigned)batch);
    hipStream_t st = as_stream(stream);
    if (prior)
        hipLaunchKernelGGL(k_gd_prior_partial, grid, dim3(GD_THREADS), 0, st, x_start, tab, table_len, (double*)workspace, per_sample);
    else
        hipLaunchKernelGGL(k_gd_vlb_partial<false>, grid, dim3(GD_THREADS), 0, st, x_start, x_t, model_out, per_sample, nullptr, 0, t, tab,
                           table_len, mean_type == RHO_GD_EPSILON ? 1 : 0, 0, quantile, noise, pred_xstart, (double*)workspace, per_sample,
                           err_flag);
    hipLaunchKernelGGL(k_gd_vlb_final, dim3((unsigned)batch), dim3(GD_THREADS), 0, st, (const double*)workspace, chunks, t, prior,
                       per_sample, vb, xstart_mse, mse, out_stride, raw_kl, raw_nll);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_gd_vlb_terms_lv(const float* x_start, const float* x_t, const float* model_out, int64_t mean_stride, const float* var_values,
                                   int64_t var_stride, const int64_t* t, const float* tab, int64_t table_len, int mean_type, int var_type,
                                   const float* quantile, const float* noise, float* vb, float* xstart_mse, float* mse, int64_t out_stride,
                                   float* raw_kl, float* raw_nll, float* pred_xstart, void* workspace, int64_t batch, int64_t per_sample,
                                   int32_t* err_flag, void* stream) {
    if (!x_start || !x_t || !model_out || !var_values || !t || !tab || !vb || !workspace || (mse && !noise)) return RHO_E_ARG;
    if (batch <= 0 || per_sample <= 0 || table_len <= 0 || out_stride < 1) return RHO_E_ARG;
    if (mean_stride < per_sample || var_stride < per_sample || !gd_lv_ok(mean_type, var_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    const int64_t chunks = gd_chunks(batch, per_sample);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_gd_vlb_partial<true>, dim3((unsigned)chunks, (unsigned)batch), dim3(GD_THREADS), 0, st, x_start, x_t, model_out,
                       mean_stride, var_values, var_stride, t, tab, table_len, mean_type == RHO_GD_EPSILON ? 1 : 0,
                       var_type == RHO_GD_LEARNED_RANGE ? 1 : 0, quantile, noise, pred_xstart, (double*)workspace, per_sample, err_flag);
    hipLaunchKernelGGL(k_gd_vlb_final, dim3((unsigned)batch), dim3(GD_THREADS), 0, st, (const double*)workspace, chunks, t, 0, per_sample, vb,
                       xstart_mse, mse, out_stride, raw_kl, raw_nll);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- hybrid loss
// training_losses (:893-930), MSE / RESCALED_MSE with a learned variance, model output mo [B, 2C, ...] read in place:
//   mse[b]  = mean((target - m)^2)
//   vb[b]   = _vb_terms_bpd(frozen m, v; clip_denoised=False) (* vb_scale = T/1000 for RESCALED_MSE);  loss = mse + vb
// Only the term where(t == 0, nll, kl) selects is evaluated.  Backward: the mean half gets the MSE gradient only (the reference
// detaches m for the VLB), the variance half g_vb / ln2 / n * d term / d logvar * d logvar / d v.
// Pure streaming passes: 16-byte loads when per_sample % 4 == 0 and every base pointer is 16-byte aligned (gd_hyb_vec), else scalar.
namespace {
constexpr int GD_HYB_K = 2;

// d logvar / d v (autograd's order: d frac = g*max_log + -(g*min_log), d v = d frac / 2)
__device__ __forceinline__ float gd_learned_dlogvar(const GdCoef& c, float g) {
    if (!c.range) return g;
    const float p0 = g * c.max_log, p1 = g * c.post_logvar;
    return (p0 + -p1) / 2.0f;
}

// the means of one element: (true mean, frozen model mean)
__device__ __forceinline__ void gd_hyb_means(const GdCoef& c, float x, float xs, float m, float& tm, float& mm) {
    const float x0 = gd_x0(c, x, m);
    const float cx = c.c2 * x;
    tm = (c.c1 * xs) + cx;
    mm = (c.c1 * x0) + cx;
}

// backward of gd_cdf in autograd's order (MulBackward 0.5, TanhBackward, MulBackward sqrt(2/pi), AddBackward + PowBackward):
// d u of an upstream gradient g at cdf(u)
__device__ __forceinline__ float gd_cdf_bwd(float g, float u, float& cdf) {
    const float x3 = (u * u) * u;
    const float w = 0.7978845608028654f * (u + 0.044715f * x3);
    const float th = tanhf(w);
    cdf = 0.5f * (1.0f + th);
    const float gw = (g * 0.5f) * (1.0f - th * th);
    const float gin = gw * 0.7978845608028654f;
    return gin + (gin * 0.044715f) * (3.0f * (u * u));
}

// d logvar of -discretized_gaussian_log_likelihood(x, mean, 0.5*logvar) for an upstream gradient g_nll, as torch autograd evaluates
// the reference expression: zero where a 1e-12 clamp or a where-branch cuts the path
__device__ __forceinline__ float gd_nll_bwd(float g_nll, float x, float mean, float lv) {
    const float log_scale = 0.5f * lv;
    const float centered = x - mean;
    const float inv_stdv = expf(-log_scale);
    const float bin = (float)(1.0 / 255.0);
    const float cpb = centered + bin, cmb = centered - bin;
    const float plus_in = inv_stdv * cpb, min_in = inv_stdv * cmb;
    float cdf_plus, cdf_min;
    gd_cdf_bwd(0.0f, plus_in, cdf_plus);
    gd_cdf_bwd(0.0f, min_in, cdf_min);
    const float g_lp = -g_nll;
    float g_cp = 0.0f, g_cm = 0.0f;
    if (x < -0.999f) {
        if (cdf_plus >= 1e-12f) g_cp = g_lp / cdf_plus;
    } else if (x > 0.999f) {
        const float r = 1.0f - cdf_min;
        if (r >= 1e-12f) g_cm = -(g_lp / r);
    } else {
        const float d = cdf_plus - cdf_min;
        if (d >= 1e-12f) {
            g_cp = g_lp / d;
            g_cm = -g_cp;
        }
    }
    float c;
    const float g_inv = gd_cdf_bwd(g_cp, plus_in, c) * cpb + gd_cdf_bwd(g_cm, min_in, c) * cmb;
    const float g_ls = -(g_inv * inv_stdv);
    return g_ls * 0.5f;
}

// d lv2 of normal_kl(m1, lv1, m2, lv2) for an upstream gradient g, autograd's order:
//   g1 = g*0.5;  g1 + -(g1*exp(lv1 - lv2)) + -((g1*(m1 - m2)^2)*exp(-lv2))
__device__ __forceinline__ float gd_kl_bwd(float g, float m1, float lv1, float m2, float lv2) {
    const float g1 = g * 0.5f;
    const float d = m1 - m2;
    const float a = g1 + -(g1 * expf(lv1 - lv2));
    return a + -((g1 * (d * d)) * expf(-lv2));
}

// mean((target - m)^2) and the selected VLB term of one element pair
__device__ __forceinline__ void gd_hyb_fwd_elem(const GdCoef& c, float x, float xs, float tg, float m, float v, double (&acc)[GD_HYB_K]) {
    const float d = tg - m;
    acc[0] += (double)(d * d);
    float tm, mm;
    gd_hyb_means(c, x, xs, m, tm, mm);
    const float lv2 = gd_learned_logvar(c, v);
    if (c.t0) acc[1] -= (double)gd_dgll(xs, mm, 0.5f * lv2);
    else acc[1] += (double)gd_normal_kl(tm, c.post_logvar, mm, lv2);
}

// (d mean-half, d variance-half) of one element pair; gm = d loss / d mse[b] / n, gv = d loss / d vb[b] * scale / ln2 / n
__device__ __forceinline__ void gd_hyb_bwd_elem(const GdCoef& c, float x, float xs, float tg, float m, float v, float gm, float gv, float& dm,
                                                float& dv) {
    const float d = tg - m;
    const float p = gm * (2.0f * d);
    dm = -p;
    float tm, mm;
    gd_hyb_means(c, x, xs, m, tm, mm);
    const float lv2 = gd_learned_logvar(c, v);
    const float dlv = c.t0 ? gd_nll_bwd(gv, xs, mm, lv2) : gd_kl_bwd(gv, tm, c.post_logvar, mm, lv2);
    dv = gd_learned_dlogvar(c, dlv);
}
}  // namespace

template <int V>
__global__ __launch_bounds__(GD_THREADS) void k_gd_hybrid_partial(const float* __restrict__ xs, const float* __restrict__ xt,
                                                                  const float* __restrict__ tgt, const float* __restrict__ mo,
                                                                  const int64_t* __restrict__ t, const float* __restrict__ tab, int64_t len,
                                                                  int eps_mode, int range, double* __restrict__ ws, int64_t n, int32_t* err_flag) {
    const int b = blockIdx.y;
    const GdCoef c = gd_coef<true>(t, tab, len, b, eps_mode, range, err_flag);
    double acc[GD_HYB_K] = {0.0, 0.0};
    const int64_t off = (int64_t)b * n;
    const float* mb = mo + 2 * off;
    const float* vb = mb + n;
    const float* xsb = xs + off;
    const float* xtb = xt + off;
    const float* tgb = tgt + off;
    for (int64_t i = ((int64_t)blockIdx.x * GD_THREADS + threadIdx.x) * V; i < n; i += (int64_t)gridDim.x * GD_THREADS * V) {
        if constexpr (V == 4) {
            const float4 x = *reinterpret_cast<const float4*>(xtb + i), s = *reinterpret_cast<const float4*>(xsb + i);
            const float4 g = *reinterpret_cast<const float4*>(tgb + i), m = *reinterpret_cast<const float4*>(mb + i);
            const float4 v = *reinterpret_cast<const float4*>(vb + i);
            gd_hyb_fwd_elem(c, x.x, s.x, g.x, m.x, v.x, acc);
            gd_hyb_fwd_elem(c, x.y, s.y, g.y, m.y, v.y, acc);
            gd_hyb_fwd_elem(c, x.z, s.z, g.z, m.z, v.z, acc);
            gd_hyb_fwd_elem(c, x.w, s.w, g.w, m.w, v.w, acc);
        } else {
            gd_hyb_fwd_elem(c, xtb[i], xsb[i], tgb[i], mb[i], vb[i], acc);
        }
    }
    gd_block_sum<GD_HYB_K>(acc);
    if (threadIdx.x == 0) {
        double* w = ws + ((int64_t)b * gridDim.x + blockIdx.x) * GD_HYB_K;
        w[0] = acc[0];
        w[1] = acc[1];
    }
}

// stage 2: mse = mean, vb = mean / ln 2 (* vb_scale), loss = mse + vb (float32, as the reference's tensors)
__global__ __launch_bounds__(GD_THREADS) void k_gd_hybrid_final(const double* __restrict__ ws, int64_t chunks, int64_t n, int rescale,
                                                                float vb_scale, float* __restrict__ loss, float* __restrict__ mse,
                                                                float* __restrict__ vb) {
    const int b = blockIdx.x;
    double acc[GD_HYB_K];
    gd_sum_partials<GD_HYB_K>(ws, chunks, b, acc);
    if (threadIdx.x != 0) return;
    const float ln2 = (float)0.69314718055994530942;
    const float m = (float)(acc[0] / (double)n);
    float v = (float)(acc[1] / (double)n) / ln2;
    if (rescale) v = v * vb_scale;
    loss[b] = m + v;
    if (mse != nullptr) mse[b] = m;
    if (vb != nullptr) vb[b] = v;
}

template <int V>
__global__ __launch_bounds__(GD_THREADS) void k_gd_hybrid_bwd(const float* __restrict__ xs, const float* __restrict__ xt,
                                                              const float* __restrict__ tgt, const float* __restrict__ mo,
                                                              const int64_t* __restrict__ t, const float* __restrict__ tab, int64_t len,
                                                              int eps_mode, int range, int rescale, float vb_scale,
                                                              const float* __restrict__ g_loss, const float* __restrict__ g_mse,
                                                              const float* __restrict__ g_vb, float* __restrict__ grad, int64_t n,
                                                              int32_t* err_flag) {
    const int b = blockIdx.y;
    const GdCoef c = gd_coef<true>(t, tab, len, b, eps_mode, range, err_flag);
    // autograd: loss = mse + vb hands g_loss to both; the reference's ops in order: (vb * scale), / ln2, mean over n
    const float gl = g_loss != nullptr ? g_loss[b] : 0.0f;
    const float gms = g_mse != nullptr ? gl + g_mse[b] : gl;
    float gvs = g_vb != nullptr ? gl + g_vb[b] : gl;
    if (rescale) gvs = gvs * vb_scale;
    const float gm = gms / (float)n;
    const float gv = (gvs / (float)0.69314718055994530942) / (float)n;
    const int64_t off = (int64_t)b * n;
    const float* mb = mo + 2 * off;
    const float* vb = mb + n;
    float* dmb = grad + 2 * off;
    float* dvb = dmb + n;
    const float* xsb = xs + off;
    const float* xtb = xt + off;
    const float* tgb = tgt + off;
    for (int64_t i = ((int64_t)blockIdx.x * GD_THREADS + threadIdx.x) * V; i < n; i += (int64_t)gridDim.x * GD_THREADS * V) {
        if constexpr (V == 4) {
            const float4 x = *reinterpret_cast<const float4*>(xtb + i), s = *reinterpret_cast<const float4*>(xsb + i);
            const float4 g = *reinterpret_cast<const float4*>(tgb + i), m = *reinterpret_cast<const float4*>(mb + i);
            const float4 v = *reinterpret_cast<const float4*>(vb + i);
            float4 dm, dv;
            gd_hyb_bwd_elem(c, x.x, s.x, g.x, m.x, v.x, gm, gv, dm.x, dv.x);
            gd_hyb_bwd_elem(c, x.y, s.y, g.y, m.y, v.y, gm, gv, dm.y, dv.y);
            gd_hyb_bwd_elem(c, x.z, s.z, g.z, m.z, v.z, gm, gv, dm.z, dv.z);
            gd_hyb_bwd_elem(c, x.w, s.w, g.w, m.w, v.w, gm, gv, dm.w, dv.w);
            *reinterpret_cast<float4*>(dmb + i) = dm;
            *reinterpret_cast<float4*>(dvb + i) = dv;
        } else {
            gd_hyb_bwd_elem(c, xtb[i], xsb[i], tgb[i], mb[i], vb[i], gm, gv, dmb[i], dvb[i]);
        }
    }
}

namespace {
int64_t gd_hyb_chunks(int64_t batch, int64_t per_sample, int v) { return gd_chunks(batch, (per_sample + v - 1) / v); }
// the 16-byte path: per_sample % 4 == 0 (then every row of both halves is as aligned as its base) and every base 16-byte aligned
bool gd_hyb_vec(int64_t per_sample, std::initializer_list<const void*> bases) {
    if ((per_sample & 3) != 0) return false;
    for (const void* p : bases)
        if (((uintptr_t)p & 15) != 0) return false;
    return true;
}
}  // namespace

extern "C" int rho_gd_hybrid_loss(const float* x_start, const float* x_t, const float* target, const float* model_out, const int64_t* t,
                                  const float* tab, int64_t table_len, int mean_type, int var_type, int rescaled, float vb_scale, float* loss,
                                  float* mse, float* vb, void* workspace, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream) {
    if (!x_start || !x_t || !target || !model_out || !t || !tab || !loss || !workspace) return RHO_E_ARG;
    if (batch <= 0 || per_sample <= 0 || table_len <= 0 || !gd_lv_ok(mean_type, var_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    const int v = gd_hyb_vec(per_sample, {x_start, x_t, target, model_out}) ? 4 : 1;
    const int64_t chunks = gd_hyb_chunks(batch, per_sample, v);      // <= gd_chunks(batch, per_sample): the workspace of the VLB pass fits
    hipStream_t st = as_stream(stream);
    dim3 grid((unsigned)chunks, (unsigned)batch);
    const int em = mean_type == RHO_GD_EPSILON ? 1 : 0, rg = var_type == RHO_GD_LEARNED_RANGE ? 1 : 0;
    if (v == 4)
        hipLaunchKernelGGL(k_gd_hybrid_partial<4>, grid, dim3(GD_THREADS), 0, st, x_start, x_t, target, model_out, t, tab, table_len, em, rg,
                           (double*)workspace, per_sample, err_flag);
    else
        hipLaunchKernelGGL(k_gd_hybrid_partial<1>, grid, dim3(GD_THREADS), 0, st, x_start, x_t, target, model_out, t, tab, table_len, em, rg,
                           (double*)workspace, per_sample, err_flag);
    hipLaunchKernelGGL(k_gd_hybrid_final, dim3((unsigned)batch), dim3(GD_THREADS), 0, st, (const double*)workspace, chunks, per_sample,
                       rescaled ? 1 : 0, vb_scale, loss, mse, vb);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_gd_hybrid_loss_bwd(const float* x_start, const float* x_t, const float* target, const float* model_out, const int64_t* t,
                                      const float* tab, int64_t table_len, int mean_type, int var_type, int rescaled, float vb_scale,
                                      const float* g_loss, const float* g_mse, const float* g_vb, float* grad, int64_t batch, int64_t per_sample,
                                      int32_t* err_flag, void* stream) {
    if (!x_start || !x_t || !target || !model_out || !t || !tab || !grad) return RHO_E_ARG;
    if (batch <= 0 || per_sample <= 0 || table_len <= 0 || !gd_lv_ok(mean_type, var_type)) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    const int v = gd_hyb_vec(per_sample, {x_start, x_t, target, model_out, grad}) ? 4 : 1;
    dim3 grid((unsigned)gd_hyb_chunks(batch, per_sample, v), (unsigned)batch);
    hipStream_t st = as_stream(stream);
    const int em = mean_type == RHO_GD_EPSILON ? 1 : 0, rg = var_type == RHO_GD_LEARNED_RANGE ? 1 : 0;
    if (v == 4)
        hipLaunchKernelGGL(k_gd_hybrid_bwd<4>, grid, dim3(GD_THREADS), 0, st, x_start, x_t, target, model_out, t, tab, table_len, em, rg,
                           rescaled ? 1 : 0, vb_scale, g_loss, g_mse, g_vb, grad, per_sample, err_flag);
    else
        hipLaunchKernelGGL(k_gd_hybrid_bwd<1>, grid, dim3(GD_THREADS), 0, st, x_start, x_t, target, model_out, t, tab, table_len, em, rg,
                           rescaled ? 1 : 0, vb_scale, g_loss, g_mse, g_vb, grad, per_sample, err_flag);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- per-sample MSE
// training_losses (:861-934), MSE: mean_flat((target - out)^2) -> loss[b]; backward of the same:
//   d out = -((g[b] / n) * (2 * (target - out)))    (MeanBackward, PowBackward, SubBackward in that order)
__global__ __launch_bounds__(GD_THREADS) void k_gd_mse_partial(const float* __restrict__ target, const float* __restrict__ out,
                                                               double* __restrict__ ws, int64_t n) {
    const int b = blockIdx.y;
    double acc[1] = {0.0};
    const int64_t off = (int64_t)b * n;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float d = target[i] - out[i];
        acc[0] += (double)(d * d);
    }
    gd_block_sum<1>(acc);
    if (threadIdx.x == 0) ws[(int64_t)b * gridDim.x + blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(GD_THREADS) void k_gd_mse_final(const double* __restrict__ ws, int64_t chunks, int64_t n, float* __restrict__ loss) {
    double acc[1];
    gd_sum_partials<1>(ws, chunks, blockIdx.x, acc);
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)(acc[0] / (double)n);
}

extern "C" int rho_gd_mse_per_sample(const float* target, const float* out, float* loss, void* workspace, int64_t batch, int64_t per_sample,
                                     void* stream) {
    if (!target || !out || !loss || !workspace || batch <= 0 || per_sample <= 0) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    const int64_t chunks = gd_chunks(batch, per_sample);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_gd_mse_partial, dim3((unsigned)chunks, (unsigned)batch), dim3(GD_THREADS), 0, st, target, out, (double*)workspace,
                       per_sample);
    hipLaunchKernelGGL(k_gd_mse_final, dim3((unsigned)batch), dim3(GD_THREADS), 0, st, (const double*)workspace, chunks, per_sample, loss);
    RHO_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(GD_THREADS) void k_gd_mse_bwd(const float* __restrict__ target, const float* __restrict__ out,
                                                           const float* __restrict__ g, float* __restrict__ grad, int64_t n) {
    const int b = blockIdx.y;
    const float gn = g[b] / (float)n;
    const int64_t off = (int64_t)b * n;
    for (int64_t i = off + (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < off + n; i += (int64_t)gridDim.x * GD_THREADS) {
        const float d = target[i] - out[i];
        const float p = gn * (2.0f * d);
        grad[i] = -p;
    }
}

extern "C" int rho_gd_mse_per_sample_bwd(const float* target, const float* out, const float* g, float* grad, int64_t batch, int64_t per_sample,
                                         void* stream) {
    if (!target || !out || !g || !grad || batch <= 0 || per_sample <= 0) return RHO_E_ARG;
    if (batch > 65535) return RHO_E_SHAPE;
    dim3 grid((unsigned)gd_chunks(batch, per_sample), (unsigned)batch);
    hipLaunchKernelGGL(k_gd_mse_bwd, grid, dim3(GD_THREADS), 0, as_stream(stream), target, out, g, grad, per_sample);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- metrics (losses.py)
// Operands: full [batch, per_sample] (mode 0), per-sample [batch] (mode 1) or a scalar kernel argument (mode 2); 2 bits per operand.
__device__ __forceinline__ float gd_operand(const float* __restrict__ p, float s, int mode, int64_t i, int64_t n) {
    return mode == 2 ? s : (mode == 1 ? p[i / n] : p[i]);
}

__global__ __launch_bounds__(GD_THREADS) void k_gd_normal_kl(const float* __restrict__ m1, const float* __restrict__ lv1, const float* __restrict__ m2,
                                                             const float* __restrict__ lv2, float s_m1, float s_lv1, float s_m2, float s_lv2, int modes,
                                                             float* __restrict__ out, int64_t n, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * GD_THREADS) {
        out[i] = gd_normal_kl(gd_operand(m1, s_m1, modes & 3, i, n), gd_operand(lv1, s_lv1, (modes >> 2) & 3, i, n),
                              gd_operand(m2, s_m2, (modes >> 4) & 3, i, n), gd_operand(lv2, s_lv2, (modes >> 6) & 3, i, n));
    }
}

__global__ __launch_bounds__(GD_THREADS) void k_gd_dgll(const float* __restrict__ x, const float* __restrict__ means, const float* __restrict__ ls,
                                                        float s_x, float s_means, float s_ls, int modes, float* __restrict__ out, int64_t n,
                                                        int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * GD_THREADS) {
        out[i] = gd_dgll(gd_operand(x, s_x, modes & 3, i, n), gd_operand(means, s_means, (modes >> 2) & 3, i, n),
                         gd_operand(ls, s_ls, (modes >> 4) & 3, i, n));
    }
}

__global__ __launch_bounds__(GD_THREADS) void k_gd_cdf(const float* __restrict__ x, float* __restrict__ out, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * GD_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * GD_THREADS) out[i] = gd_cdf(x[i]);
}

namespace {
bool gd_modes_ok(const float* const* p, int count, int modes) {
    for (int k = 0; k < count; ++k) {
        const int m = (modes >> (2 * k)) & 3;
        if (m == 3 || (m != 2 && p[k] == nullptr)) return false;
    }
    return (modes >> (2 * count)) == 0;
}
unsigned gd_flat_grid(int64_t total) {
    int64_t g = (total + GD_THREADS - 1) / GD_THREADS;
    return (unsigned)(g > 4096 ? 4096 : g);
}
}  // namespace

extern "C" int rho_normal_kl(const float* mean1, const float* logvar1, const float* mean2, const float* logvar2, float s_mean1, float s_logvar1,
                             float s_mean2, float s_logvar2, int modes, float* out, int64_t batch, int64_t per_sample, void* stream) {
    const float* p[4] = {mean1, logvar1, mean2, logvar2};
    if (!out || batch <= 0 || per_sample <= 0 || !gd_modes_ok(p, 4, modes)) return RHO_E_ARG;
    const int64_t total = batch * per_sample;
    hipLaunchKernelGGL(k_gd_normal_kl, dim3(gd_flat_grid(total)), dim3(GD_THREADS), 0, as_stream(stream), mean1, logvar1, mean2, logvar2,
                       s_mean1, s_logvar1, s_mean2, s_logvar2, modes, out, per_sample, total);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_discretized_gaussian_ll(const float* x, const float* means, const float* log_scales, float s_x, float s_means,
                                           float s_log_scales, int modes, float* out, int64_t batch, int64_t per_sample, void* stream) {
    const float* p[3] = {x, means, log_scales};
    if (!out || batch <= 0 || per_sample <= 0 || !gd_modes_ok(p, 3, modes)) return RHO_E_ARG;
    const int64_t total = batch * per_sample;
    hipLaunchKernelGGL(k_gd_dgll, dim3(gd_flat_grid(total)), dim3(GD_THREADS), 0, as_stream(stream), x, means, log_scales, s_x, s_means,
                       s_log_scales, modes, out, per_sample, total);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_approx_normal_cdf(const float* x, float* out, int64_t n, void* stream) {
    if (!x || !out || n <= 0) return RHO_E_ARG;
    hipLaunchKernelGGL(k_gd_cdf, dim3(gd_flat_grid(n)), dim3(GD_THREADS), 0, as_stream(stream), x, out, n);
    RHO_LAUNCH_CHECK();
    return 0;
}
