// HBM-bound kernels: the DDPM loops, the small embedding GEMVs, the input packing and the pointwise / resampling helpers of
// the backward pass (weight preparation and weight-gradient finalize live in weight_tables.hip).
// Each kernel is a grid-stride loop over 16-byte-per-lane accesses (coalesced 1 KiB per wave
// instruction), grid capped at 256 CUs x 8 blocks.
#include <cstdlib>

#include "common.h"

static inline int grid_for(int64_t work_items, int block) {
    int64_t g = (work_items + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" int rho_abi_version(void) { return RHO_ABI_VERSION; }

// Process-wide reproducibility switch (RHO_DETERMINISTIC=1, or rho_set_deterministic): kernels that combine partial sums with
// fp32 atomics (linear backward, label-embedding backward) take an ordered path instead; the weight gradient's ordered flush
// needs a workspace and is chosen by the caller (rho_conv_nd_wgrad_ws), who reads this flag.
static int g_deterministic = -1;
extern "C" int rho_get_deterministic(void) {
    if (g_deterministic < 0) {
        const char* e = getenv("RHO_DETERMINISTIC");
        const char* e2 = getenv("RHO_WGRAD_DETERMINISTIC");
        g_deterministic = ((e && atoi(e) != 0) || (e2 && atoi(e2) != 0)) ? 1 : 0;
    }
    return g_deterministic;
}
extern "C" int rho_set_deterministic(int on) {
    const int old = rho_get_deterministic();
    g_deterministic = on ? 1 : 0;
    return old;
}
#ifndef RHO_BUILD_ID
#define RHO_BUILD_ID "unstamped"
#endif
extern "C" const char* rho_build_info(void) {
    return "librho_hip gfx950 (CDNA4) hipcc -O3; MFMA 16x16x32 + 32x32x16 bf16 / 32x32x2 f32; build " RHO_BUILD_ID;
}

// ----------------------------------------------------------------------------- q_sample
// ddpm.py:122-129: x_t = sqrt(abar_t)*x0 + sqrt(1-abar_t)*eps, abar gathered per batch element.
// The contraction is written out (left to the compiler, the 16-byte kernel fused sa * x0 into the sum and the scalar kernel did
// not): the scalar kernel that serves ragged or 4-byte-aligned operands gives the bits of the 16-byte one.
__device__ __forceinline__ float q_mix(float sa, float x, float sb, float e) { return __fmaf_rn(sa, x, sb * e); }
__global__ __launch_bounds__(256) void k_q_sample(const float4* __restrict__ x0, const float4* __restrict__ eps,
                                                  float4* __restrict__ xt, const float* __restrict__ abar,
                                                  const int64_t* __restrict__ t, int64_t per4, int64_t total4,
                                                  int64_t table_len, int32_t* nan_flag) {
    bool bad = false, oob = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / per4;
        int64_t tb = t[b];
        if (tb < 0 || tb >= table_len) { oob = true; tb = tb < 0 ? 0 : table_len - 1; }   // the reference raises IndexError
        const float ab = abar[tb];
        const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
        const float4 a = x0[i], e = eps[i];
        float4 r;
        r.x = q_mix(sa, a.x, sb, e.x);
        r.y = q_mix(sa, a.y, sb, e.y);
        r.z = q_mix(sa, a.z, sb, e.z);
        r.w = q_mix(sa, a.w, sb, e.w);
        bad |= (r.x != r.x) | (r.y != r.y) | (r.z != r.z) | (r.w != r.w);
        xt[i] = r;
    }
    const int any_bad = __any(bad), any_oob = __any(oob);
    if (nan_flag != nullptr && (any_bad || any_oob)) {
        if ((threadIdx.x & 63) == 0) atomicOr(nan_flag, (any_bad ? 1 : 0) | (any_oob ? 4 : 0));
    }
}

__global__ void k_q_sample_tail(const float* x0, const float* eps, float* xt, const float* abar, const int64_t* t,
                                int64_t per_sample, int64_t batch, int64_t table_len, int32_t* nan_flag) {
    // scalar path for per_sample % 4 != 0 (only tiny test shapes)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < batch * per_sample; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t tb = t[i / per_sample];
        if (tb < 0 || tb >= table_len) {
            if (nan_flag) atomicOr(nan_flag, 4);
            tb = tb < 0 ? 0 : table_len - 1;
        }
        const float ab = abar[tb];
        const float r = q_mix(sqrtf(ab), x0[i], sqrtf(1.0f - ab), eps[i]);
        if (r != r && nan_flag) atomicOr(nan_flag, 1);
        xt[i] = r;
    }
}

extern "C" int rho_q_sample(const float* x0, const float* eps, float* x_t, const float* alpha_bar, const int64_t* t,
                            int64_t batch, int64_t per_sample, int64_t table_len, int32_t* nan_flag, void* stream) {
    if (!x0 || !eps || !x_t || !alpha_bar || !t || batch <= 0 || per_sample <= 0 || table_len <= 0) return RHO_E_ARG;
    if (per_sample % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)x_t) & 15) == 0) {
        const int64_t total4 = batch * per_sample / 4;
        hipLaunchKernelGGL(k_q_sample, dim3(grid_for(total4, 256)), dim3(256), 0, as_stream(stream), (const float4*)x0,
                           (const float4*)eps, (float4*)x_t, alpha_bar, t, per_sample / 4, total4, table_len, nan_flag);
    } else {
        hipLaunchKernelGGL(k_q_sample_tail, dim3(grid_for(batch * per_sample, 256)), dim3(256), 0, as_stream(stream), x0, eps,
                           x_t, alpha_bar, t, per_sample, batch, table_len, nan_flag);
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- the element walk of the reverse-process updates
// rho_p_sample_step[_cfg], rho_p_sample_step_spaced[_pred] and rho_dpmpp_2m_step stream the same operands and differ in the
// per-element expression (an update functor Op) and in how the kernel loads its coefficient row.  step_walk owns the rest:
//   * the grid-stride 16-byte body (vec, granted by step_launch) and the scalar loop behind it - the tail of the body, or every
//     element where vec == 0.  Both call op(), a written-out contraction, so all forms give the same bits;
//   * GUIDED: x and ph hold [2, n] - row 0 is x_t / the conditional prediction, row 1 its copy (the 2B batch the engine reads) / the
//     null-condition prediction.  p = p_u + s * (p_c - p_u) (cfg_mix: the difference, one fma) enters op, the result is stored to
//     BOTH rows of x: no guided prediction and no duplicate of x_t in between;
//   * the side operand, one row of n also under guidance: read only under read_side (z where noise enters, hist where the row is
//     second order; else op sees 0 and the buffer may be NULL or uninitialised) and written where Op::WRITES_SIDE (hist).  One
//     pointer serves the read and the write of an element, so it alone carries __restrict__.
// Every launch has STEP_BLOCK threads per block (step_launch), and the walk counts with the constant: blockDim.x read inside a
// __device__ function compiles to a vector load from the dispatch packet in front of the first element.
constexpr int STEP_BLOCK = 256;
__device__ __forceinline__ float cfg_mix(float s, float ec, float eu) { return __fmaf_rn(s, ec - eu, eu); }
template <bool GUIDED, class Op, class Side>
__device__ __forceinline__ void step_walk(const Op& op, float* __restrict__ x, const float* __restrict__ ph, Side* __restrict__ side,
                                          bool read_side, float s, int64_t n, int vec) {
    const int64_t stride = (int64_t)gridDim.x * STEP_BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * STEP_BLOCK + threadIdx.x;
    int64_t done = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        float4* xa = (float4*)x;
        float4* xb = (float4*)(x + n);
        const float4* pa = (const float4*)ph;
        const float4* pb = (const float4*)(ph + n);
        for (int64_t i = tid; i < n4; i += stride) {
            float4 a = xa[i];
            float4 p = pa[i];
            if (GUIDED) {
                const float4 pu = pb[i];
                p.x = cfg_mix(s, p.x, pu.x), p.y = cfg_mix(s, p.y, pu.y), p.z = cfg_mix(s, p.z, pu.z), p.w = cfg_mix(s, p.w, pu.w);
            }
            float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
            if (read_side) h = ((const float4*)side)[i];
            float4 o;
            a.x = op(a.x, p.x, h.x, o.x);
            a.y = op(a.y, p.y, h.y, o.y);
            a.z = op(a.z, p.z, h.z, o.z);
            a.w = op(a.w, p.w, h.w, o.w);
            if constexpr (Op::WRITES_SIDE) ((float4*)side)[i] = o;
            xa[i] = a;
            if (GUIDED) xb[i] = a;
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += stride) {
        const float xi = x[i];
        const float p = GUIDED ? cfg_mix(s, ph[i], ph[n + i]) : ph[i];
        const float h = read_side ? side[i] : 0.0f;
        float o;
        const float r = op(xi, p, h, o);
        if constexpr (Op::WRITES_SIDE) side[i] = o;
        x[i] = r;
        if (GUIDED) x[n + i] = r;
    }
}

// The 16-byte form needs 16-byte aligned bases and, under guidance, n % 4 == 0 (row 1 starts n elements behind row 0); the plain form
// takes any n and finishes with the scalar tail.  Any other n or pointer takes the scalar loop alone, one thread per element.
struct StepLaunch {
    int vec;
    dim3 grid, block;
};
static StepLaunch step_launch(const void* x, const void* pred, const void* side, int64_t n, int guided) {
    const bool aligned = (((uintptr_t)x | (uintptr_t)pred | (uintptr_t)side) & 15) == 0;
    const int vec = (aligned && (!guided || n % 4 == 0)) ? 1 : 0;
    return {vec, dim3(grid_for(vec ? (n + 3) / 4 : n, STEP_BLOCK)), dim3(STEP_BLOCK)};
}

// ----------------------------------------------------------------------------- p_sample_step, plain and with classifier-free guidance
// ddpm.py:210-218.  coef row = {1/sqrt(alpha), beta/sqrt(1-abar), 0.8*sqrt(beta)}; t read on device so
// that one captured graph serves every step; t == 0 => no update (q3), t <= 1 => z ignored.
// rho_p_sample_step_cfg: x2 / eps2 = [2, n] as step_walk's GUIDED form takes them; 4n floats read (3n when z is ignored), 2n written.
struct PSampleOp {
    static constexpr bool WRITES_SIDE = false;
    float c0, c1, c2;
    __device__ __forceinline__ float operator()(float x, float e, float z, float&) const {
        return fminf(fmaxf(__fmaf_rn(c0, __fmaf_rn(-c1, e, x), c2 * z), -1.0f), 1.0f);
    }
};
template <bool GUIDED>
__device__ __forceinline__ void p_sample_rows(float* __restrict__ x, const float* __restrict__ eh, const float* __restrict__ z,
                                              const float* __restrict__ coef, const int32_t* __restrict__ t_dev, float s, int64_t n,
                                              int vec) {
    const int t = *t_dev;
    if (t <= 0) return;
    PSampleOp c;
    c.c0 = coef[3 * t + 0], c.c1 = coef[3 * t + 1], c.c2 = (t > 1 && z != nullptr) ? coef[3 * t + 2] : 0.0f;
    step_walk<GUIDED>(c, x, eh, z, c.c2 != 0.0f, s, n, vec);
}
__global__ __launch_bounds__(STEP_BLOCK) void k_p_sample(float* __restrict__ x, const float* __restrict__ eh,
                                                  const float* __restrict__ z, const float* __restrict__ coef,
                                                  const int32_t* __restrict__ t_dev, int64_t n, int vec) {
    p_sample_rows<false>(x, eh, z, coef, t_dev, 0.0f, n, vec);
}
__global__ __launch_bounds__(STEP_BLOCK) void k_p_sample_cfg(float* __restrict__ x2, const float* __restrict__ e2,
                                                      const float* __restrict__ z, const float* __restrict__ coef,
                                                      const int32_t* __restrict__ t_dev, float s, int64_t n, int vec) {
    p_sample_rows<true>(x2, e2, z, coef, t_dev, s, n, vec);
}

extern "C" int rho_p_sample_step(float* x, const float* eps_hat, const float* z, const float* coef_table,
                                 const int32_t* t_dev, int64_t n, void* stream) {
    if (!x || !eps_hat || !coef_table || !t_dev || n <= 0) return RHO_E_ARG;
    const StepLaunch l = step_launch(x, eps_hat, z, n, 0);
    hipLaunchKernelGGL(k_p_sample, l.grid, l.block, 0, as_stream(stream), x, eps_hat, z, coef_table, t_dev, n, l.vec);
    RHO_LAUNCH_CHECK();
    return 0;
}

extern "C" int rho_p_sample_step_cfg(float* x2, const float* eps2, const float* z, const float* coef_table, const int32_t* t_dev,
                                     float scale, int64_t n, void* stream) {
    if (!x2 || !eps2 || !coef_table || !t_dev || n <= 0) return RHO_E_ARG;
    const StepLaunch l = step_launch(x2, eps2, z, n, 1);
    hipLaunchKernelGGL(k_p_sample_cfg, l.grid, l.block, 0, as_stream(stream), x2, eps2, z, coef_table, t_dev, scale, n, l.vec);
    RHO_LAUNCH_CHECK();
    return 0;
}

// t <- t - 1 and philox offset += delta: keeps the sampling loop's step state on the device
__global__ void k_step_advance(int32_t* t_dev, uint64_t* offset_dev, uint64_t delta) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (t_dev) *t_dev -= 1;
        if (offset_dev) *offset_dev += delta;
    }
}
extern "C" int rho_step_advance(int32_t* t_dev, uint64_t* offset_dev, uint64_t delta, void* stream) {
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(64), 0, as_stream(stream), t_dev, offset_dev, delta);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- p_sample_step on a spaced timestep sequence
// Few-step sampling (DDIM with eta; the reference's DDPM has no such sampler).  rows = float32 [S, 8], row k for t = tau_k:
// {sqrt(1/ab), sqrt(1/ab - 1), sqrt(ab), 1/sqrt(1 - ab), sqrt(ab_prev), sigma, sqrt(1 - ab_prev - sigma^2), 0}; k read on the device
// so that one captured graph serves every step, k outside [0, S) => nothing is written.  Noise enters iff z != NULL and the row's
// sigma != 0, else z is not read.  The guided [2, n] operands and the 16-byte form are step_walk's.
//   x0 = fma(c_recip, x, -(c_recipm1 * e));   clip: x0 = clamp(x0, -1, 1), ep = fma(-sqrt_ab, x0, x) * inv_sqrt_1mab;   else ep = e
//   r  = fma(sqrt_abp, x0, fma(coef_eps, ep, sigma * z))
// and r = sqrt_abp * x0 where the row has coef_eps == 0 and sigma == 0 (row 0 always; ep is not formed: at alpha_bar == 1 it is 0/0).
struct SpacedOp {
    static constexpr bool WRITES_SIDE = false;
    float c_recip, c_recipm1, sqrt_ab, inv_sqrt_1mab, sqrt_abp, sigma, coef_eps;
    int clip, x0_only;
    __device__ __forceinline__ float operator()(float x, float e, float z, float&) const {
        float x0 = __fmaf_rn(c_recip, x, -(c_recipm1 * e));
        if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        if (x0_only) return sqrt_abp * x0;
        const float ep = clip ? __fmaf_rn(-sqrt_ab, x0, x) * inv_sqrt_1mab : e;
        return __fmaf_rn(sqrt_abp, x0, __fmaf_rn(coef_eps, ep, sigma * z));
    }
};
template <bool GUIDED>
__global__ __launch_bounds__(STEP_BLOCK) void k_p_sample_spaced(float* __restrict__ x, const float* __restrict__ eh,
                                                         const float* __restrict__ z, const float* __restrict__ rows,
                                                         const int32_t* __restrict__ k_dev, int32_t S, float s, int64_t n, int clip,
                                                         int vec) {
    const int k = *k_dev;
    if (k < 0 || k >= S) return;
    const float* row = rows + 8 * (int64_t)k;
    // the whole row up front, unconditionally: one scalar load behind k instead of a chain of dependent ones behind each test
    const float r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4], r5 = row[5], r6 = row[6];
    SpacedOp c;
    c.c_recip = r0, c.c_recipm1 = r1, c.sqrt_ab = r2, c.inv_sqrt_1mab = r3, c.sqrt_abp = r4;
    c.coef_eps = r6;
    c.clip = clip;
    c.x0_only = ((r6 == 0.0f) & (r5 == 0.0f)) ? 1 : 0;
    const bool noisy = (z != nullptr) & (r5 != 0.0f);
    c.sigma = noisy ? r5 : 0.0f;
    step_walk<GUIDED>(c, x, eh, z, noisy, s, n, vec);
}

extern "C" int rho_p_sample_step_spaced(float* x, const float* eps_hat, const float* z, const float* rows, const int32_t* k_dev,
                                        int32_t S, int64_t n, int guided, float scale, int clip, void* stream) {
    if (!x || !eps_hat || !rows || !k_dev || S <= 0 || n <= 0) return RHO_E_ARG;
    const StepLaunch l = step_launch(x, eps_hat, z, n, guided);
    const dim3 grid = l.grid, block = l.block;
    if (guided)
        hipLaunchKernelGGL(k_p_sample_spaced<true>, grid, block, 0, as_stream(stream), x, eps_hat, z, rows, k_dev, S, scale, n,
                           clip ? 1 : 0, l.vec);
    else
        hipLaunchKernelGGL(k_p_sample_spaced<false>, grid, block, 0, as_stream(stream), x, eps_hat, z, rows, k_dev, S, 0.0f, n,
                           clip ? 1 : 0, l.vec);
    RHO_LAUNCH_CHECK();
    return 0;
}

// k <- k - 1, t <- taus[k] while k >= 0 (taus[-1] is never read; t keeps its last value), philox offset += delta
__global__ void k_spaced_advance(int32_t* k_dev, int32_t* t_dev, const int32_t* taus, uint64_t* offset_dev, uint64_t delta) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int32_t k = *k_dev - 1;
        *k_dev = k;
        if (k >= 0) *t_dev = taus[k];
        if (offset_dev) *offset_dev += delta;
    }
}
extern "C" int rho_spaced_advance(int32_t* k_dev, int32_t* t_dev, const int32_t* taus, uint64_t* offset_dev, uint64_t delta,
                                  void* stream) {
    if (!k_dev || !t_dev || !taus) return RHO_E_ARG;
    hipLaunchKernelGGL(k_spaced_advance, dim3(1), dim3(64), 0, as_stream(stream), k_dev, t_dev, taus, offset_dev, delta);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- the spaced walk for v- and x0-prediction
// rho_p_sample_step_spaced for a backbone that predicts v = sqrt(ab) eps - sqrt(1 - ab) x0 (RHO_PRED_V) or x0 itself
// (RHO_PRED_SAMPLE).  rows = float32 [S, 8], row k for t = tau_k: {sqrt(ab), sqrt(1 - ab), 1/sqrt(1 - ab) (0 where 1 - ab == 0),
// sqrt(ab_prev), sigma, sqrt(1 - ab_prev - sigma^2), 0, 0}.  Nothing is divided by sqrt(ab), so a row with ab == 0 is a row like any
// other.  k, z and clip follow k_p_sample_spaced; guidance mixes the predictions (both conversions below are affine in p at fixed x,
// so this is the mix of the two noise estimates).
//   v: x0 = fma(sqrt_ab, x, -(sqrt_1mab * p))     sample: x0 = p                    clip: x0 = clamp(x0, -1, 1)
//   ep = fma(-sqrt_ab, x0, x) * inv_sqrt_1mab;     v without clip: ep = fma(sqrt_1mab, x, sqrt_ab * p)
//   r  = fma(sqrt_abp, x0, fma(coef_eps, ep, sigma * z))
// and r = sqrt_abp * x0, ep not formed, where the row has coef_eps == 0 and sigma == 0 (row 0 always).
template <bool V>
struct PredOp {
    static constexpr bool WRITES_SIDE = false;
    float sqrt_ab, sqrt_1mab, inv_sqrt_1mab, sqrt_abp, sigma, coef_eps;
    int clip, x0_only;
    __device__ __forceinline__ float operator()(float x, float p, float z, float&) const {
        float x0 = V ? __fmaf_rn(sqrt_ab, x, -(sqrt_1mab * p)) : p;
        if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        if (x0_only) return sqrt_abp * x0;
        const float ep = (V && !clip) ? __fmaf_rn(sqrt_1mab, x, sqrt_ab * p) : __fmaf_rn(-sqrt_ab, x0, x) * inv_sqrt_1mab;
        return __fmaf_rn(sqrt_abp, x0, __fmaf_rn(coef_eps, ep, sigma * z));
    }
};
template <bool GUIDED, bool V>
__global__ __launch_bounds__(STEP_BLOCK) void k_p_sample_spaced_pred(float* __restrict__ x, const float* __restrict__ ph,
                                                              const float* __restrict__ z, const float* __restrict__ rows,
                                                              const int32_t* __restrict__ k_dev, int32_t S, float s, int64_t n,
                                                              int clip, int vec) {
    const int k = *k_dev;
    if (k < 0 || k >= S) return;
    const float* row = rows + 8 * (int64_t)k;
    const float r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4], r5 = row[5];
    PredOp<V> c;
    c.sqrt_ab = r0, c.sqrt_1mab = r1, c.inv_sqrt_1mab = r2, c.sqrt_abp = r3;
    c.coef_eps = r5;
    c.clip = clip;
    c.x0_only = ((r5 == 0.0f) & (r4 == 0.0f)) ? 1 : 0;
    const bool noisy = (z != nullptr) & (r4 != 0.0f);
    c.sigma = noisy ? r4 : 0.0f;
    step_walk<GUIDED>(c, x, ph, z, noisy, s, n, vec);
}

extern "C" int rho_p_sample_step_spaced_pred(float* x, const float* pred, const float* z, const float* rows, const int32_t* k_dev,
                                             int32_t S, int64_t n, int guided, float scale, int clip, int pred_type, void* stream) {
    if (!x || !pred || !rows || !k_dev || S <= 0 || n <= 0) return RHO_E_ARG;
    if (pred_type != RHO_PRED_V && pred_type != RHO_PRED_SAMPLE) return RHO_E_ARG;     // epsilon: rho_p_sample_step_spaced
    const StepLaunch l = step_launch(x, pred, z, n, guided);
    const dim3 grid = l.grid, block = l.block;
    const int cl = clip ? 1 : 0, vec = l.vec;
    const float s = guided ? scale : 0.0f;
    hipStream_t st = as_stream(stream);
    if (guided && pred_type == RHO_PRED_V)
        hipLaunchKernelGGL((k_p_sample_spaced_pred<true, true>), grid, block, 0, st, x, pred, z, rows, k_dev, S, s, n, cl, vec);
    else if (guided)
        hipLaunchKernelGGL((k_p_sample_spaced_pred<true, false>), grid, block, 0, st, x, pred, z, rows, k_dev, S, s, n, cl, vec);
    else if (pred_type == RHO_PRED_V)
        hipLaunchKernelGGL((k_p_sample_spaced_pred<false, true>), grid, block, 0, st, x, pred, z, rows, k_dev, S, s, n, cl, vec);
    else
        hipLaunchKernelGGL((k_p_sample_spaced_pred<false, false>), grid, block, 0, st, x, pred, z, rows, k_dev, S, s, n, cl, vec);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- DPM-Solver++(2M) on the spaced walk
// The second-order multistep update (Lu et al. 2022; the reference has no few-step sampler) in place of the DDIM one, for all three
// prediction types.  rows = float32 [S, 8], row k for the step from tau_k: {a_x, a_p, c_x, c_d0, c_d1, 0, 0, 0}
// (dpmpp_2m_coefficients).  hist float32 [n], step_walk's side operand: the x0 estimate the step before left behind, read only
// where c_d1 != 0 (the first step of a walk has none: the buffer may be uninitialised) and always overwritten with this step's.
// k and clip follow k_p_sample_spaced; no noise enters.
//   x0 = fma(a_x, x, -(a_p * p))   (sample: x0 = p)        clip: x0 = clamp(x0, -1, 1)
//   c_d1 != 0: r = fma(c_x, x, fma(c_d0, x0, c_d1 * hist))     c_d1 == 0: r = fma(c_x, x, c_d0 * x0), or c_d0 * x0 where c_x == 0
struct Dpm2mRow {
    float a_x, a_p, c_x, c_d0, c_d1;
    int clip;
};
// ORDER 2: the row has c_d1 != 0; ORDER 1: c_d1 == 0, h is not used; ORDER 0: c_d1 == 0 and c_x == 0, the x0 estimate scaled
template <int TYPE, int ORDER>
struct Dpm2mOp : Dpm2mRow {
    static constexpr bool WRITES_SIDE = true;
    __device__ __forceinline__ float operator()(float x, float p, float h, float& e) const {
        float x0 = TYPE == RHO_PRED_SAMPLE ? p : __fmaf_rn(a_x, x, -(a_p * p));
        if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        e = x0;
        if (ORDER == 2) return __fmaf_rn(c_x, x, __fmaf_rn(c_d0, x0, c_d1 * h));
        if (ORDER == 1) return __fmaf_rn(c_x, x, c_d0 * x0);
        return c_d0 * x0;
    }
};
template <bool GUIDED, int TYPE>
__global__ __launch_bounds__(STEP_BLOCK) void k_dpmpp_2m_step(float* __restrict__ x, const float* __restrict__ ph, float* __restrict__ hist,
                                                       const float* __restrict__ rows, const int32_t* __restrict__ k_dev, int32_t S,
                                                       float s, int64_t n, int clip, int vec) {
    const int k = *k_dev;
    if (k < 0 || k >= S) return;
    const float* row = rows + 8 * (int64_t)k;
    // the whole row up front, unconditionally, as k_p_sample_spaced loads it
    const float r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4];
    Dpm2mRow c;
    c.a_x = r0, c.a_p = r1, c.c_x = r2, c.c_d0 = r3, c.c_d1 = r4;
    c.clip = clip;
    // uniform: the row is the same for every lane of the launch
    if (r4 != 0.0f)
        step_walk<GUIDED>(Dpm2mOp<TYPE, 2>{c}, x, ph, hist, true, s, n, vec);
    else if (r2 != 0.0f)
        step_walk<GUIDED>(Dpm2mOp<TYPE, 1>{c}, x, ph, hist, false, s, n, vec);
    else
        step_walk<GUIDED>(Dpm2mOp<TYPE, 0>{c}, x, ph, hist, false, s, n, vec);
}

template <bool GUIDED>
static void dpmpp_2m_launch(int pred_type, dim3 grid, dim3 block, hipStream_t st, float* x, const float* pred, float* hist,
                            const float* rows, const int32_t* k_dev, int32_t S, float s, int64_t n, int cl, int vec) {
    if (pred_type == RHO_PRED_EPSILON)
        hipLaunchKernelGGL((k_dpmpp_2m_step<GUIDED, RHO_PRED_EPSILON>), grid, block, 0, st, x, pred, hist, rows, k_dev, S, s, n, cl, vec);
    else if (pred_type == RHO_PRED_V)
        hipLaunchKernelGGL((k_dpmpp_2m_step<GUIDED, RHO_PRED_V>), grid, block, 0, st, x, pred, hist, rows, k_dev, S, s, n, cl, vec);
    else
        hipLaunchKernelGGL((k_dpmpp_2m_step<GUIDED, RHO_PRED_SAMPLE>), grid, block, 0, st, x, pred, hist, rows, k_dev, S, s, n, cl, vec);
}

extern "C" int rho_dpmpp_2m_step(float* x, const float* pred, float* hist, const float* rows, const int32_t* k_dev, int32_t S,
                                 int64_t n, int guided, float scale, int clip, int pred_type, void* stream) {
    if (!x || !pred || !hist || !rows || !k_dev || S <= 0 || n <= 0) return RHO_E_ARG;
    if (pred_type != RHO_PRED_EPSILON && pred_type != RHO_PRED_V && pred_type != RHO_PRED_SAMPLE) return RHO_E_ARG;
    const StepLaunch l = step_launch(x, pred, hist, n, guided);
    const dim3 grid = l.grid, block = l.block;
    const int cl = clip ? 1 : 0, vec = l.vec;
    hipStream_t st = as_stream(stream);
    if (guided)
        dpmpp_2m_launch<true>(pred_type, grid, block, st, x, pred, hist, rows, k_dev, S, scale, n, cl, vec);
    else
        dpmpp_2m_launch<false>(pred_type, grid, block, st, x, pred, hist, rows, k_dev, S, 0.0f, n, cl, vec);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- Philox4x32-10 normals
__device__ __forceinline__ void box_muller(uint32_t u0, uint32_t u1, float& a, float& b) {
    const float f0 = ((float)(u0 >> 8) + 0.5f) * (1.0f / 16777216.0f);  // (0,1)
    const float f1 = ((float)(u1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * __logf(f0));
    float s, c;
    __sincosf(6.283185307179586f * f1, &s, &c);
    a = r * c;
    b = r * s;
}

__global__ __launch_bounds__(256) void k_philox_normal(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset,
                                                       const uint64_t* __restrict__ offset_dev) {
    const uint64_t base = offset_dev ? *offset_dev : offset;
    const int64_t n4 = (n + 3) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10(base + (uint64_t)i, seed, r);
        float v[4];
        box_muller(r[0], r[1], v[0], v[1]);
        box_muller(r[2], r[3], v[2], v[3]);
        const int64_t e = i << 2;
        if (e + 3 < n && (((uintptr_t)out & 15) == 0)) {
            *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (e + k < n) out[e + k] = v[k];
        }
    }
}

extern "C" int rho_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream) {
    if (!out || n <= 0) return RHO_E_ARG;
    hipLaunchKernelGGL(k_philox_normal, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), out, n, seed, offset,
                       offset_dev);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- MSE (+grad)
// Block b stores its partial to partials[b]; one wave adds them in index order -> the loss is bit-reproducible.
__global__ __launch_bounds__(256) void k_mse_part(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ partials,
                                                  float* __restrict__ grad, int64_t n, float inv_n, int vec) {
    __shared__ float red[4];
    float acc = 0.0f;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (vec) {                                   // 16-byte pieces (all three pointers 16-byte aligned): the HBM-rate path
        const int64_t n4 = n >> 2;
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        float4* g4 = reinterpret_cast<float4*>(grad);
        const float k2 = 2.0f * inv_n;
        for (int64_t i = tid; i < n4; i += nthr) {
            const float4 x = a4[i], y = b4[i];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
            if (grad) g4[i] = make_float4(k2 * d0, k2 * d1, k2 * d2, k2 * d3);
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nthr) {
        const float d = a[i] - b[i];
        acc += d * d;
        if (grad) grad[i] = 2.0f * d * inv_n;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}
__global__ __launch_bounds__(64) void k_mse_final(const float* __restrict__ partials, int np, float* __restrict__ loss) {
    float acc = 0.0f;
    for (int i = threadIdx.x; i < np; i += 64) acc += partials[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) *loss = acc;
}

extern "C" int rho_mse_ws(const float* a, const float* b, float* loss, float* grad_a, int64_t n, float* partials, int64_t n_partials,
                          void* stream) {
    if (!a || !b || !loss || !partials || n <= 0 || n_partials < 1) return RHO_E_ARG;
    int64_t g = grid_for(n, 256 * 8);
    if (g > n_partials) g = n_partials;
    const int vec = ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad_a) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_mse_part, dim3((unsigned)g), dim3(256), 0, as_stream(stream), a, b, partials, grad_a, n, 1.0f / (float)n, vec);
    hipLaunchKernelGGL(k_mse_final, dim3(1), dim3(64), 0, as_stream(stream), partials, (int)g, loss);
    RHO_LAUNCH_CHECK();
    return 0;
}

// The same reduction with the partials allocated and freed in stream order.  (Until ABI 7's rho_mse_ws this entry added one fp32
// atomic per block in arrival order: from about a thousand blocks on - two million elements - the half-ulp lost by each atomic
// summed to more than 1e-6 of a loss near 2, differently from run to run.)
extern "C" int rho_mse(const float* a, const float* b, float* loss, float* grad_a, int64_t n, void* stream) {
    if (!a || !b || !loss || n <= 0) return RHO_E_ARG;
    const int64_t g = grid_for(n, 256 * 8);
    float* partials = nullptr;
    hipError_t e = hipMallocAsync((void**)&partials, (size_t)g * sizeof(float), as_stream(stream));
    if (e != hipSuccess) return (int)e;
    const int rc = rho_mse_ws(a, b, loss, grad_a, n, partials, g, stream);
    e = hipFreeAsync(partials, as_stream(stream));
    return rc != 0 ? rc : (int)e;
}

// ----------------------------------------------------------------------------- training loss for eps / v / x0 prediction, min-SNR weights
// pred, x0, eps float32 [batch, per_sample]; per sample b: ab = alpha_bar[t_b], sa = sqrtf(ab), sb = sqrtf(1 - ab) as k_q_sample
// forms them, wb = w[t_b] (1 when w == NULL).  The regression target is formed on the fly and never stored:
//   RHO_PRED_EPSILON: g = eps      RHO_PRED_SAMPLE: g = x0      RHO_PRED_V: g = fma(sa, eps, -(sb * x0))
//   d = pred - g      acc = fma(wb * d, d, acc)      grad = (wb * (2 / n)) * d          (n = batch * per_sample; 2 / n = 2 * (1.0f / n))
// One written-out contraction for the 16-byte body, its tail and the scalar form: grad has the same bits in all of them (and, for
// epsilon with wb == 1, those of k_mse_part); the loss differs between the forms only by which thread adds which element.
// Geometry and reduction are k_mse_part's: thread sums in element order of its grid-stride walk, wave_sum, the four waves of the block as
// (r0 + r1) + (r2 + r3), times 1 / n -> partials[block]; k_mse_final adds the partials in index order.  No atomics on the sum.
// The 16-byte body keeps (sample, offset in the sample) of its piece and advances both by the grid stride, so no division runs in
// the loop; a piece that straddles a sample boundary (per_sample % 4 != 0) takes its coefficients element by element.
struct LossCoef {
    float sa, sb, w, kw;
};
template <int TYPE>
__device__ __forceinline__ LossCoef loss_coef(int64_t b, const float* __restrict__ abar, const float* __restrict__ w,
                                              const int64_t* __restrict__ t, int64_t table_len, float k2, bool& oob) {
    int64_t tb = t[b];
    if (tb < 0 || tb >= table_len) { oob = true; tb = tb < 0 ? 0 : table_len - 1; }
    LossCoef c;
    c.sa = c.sb = 0.0f;
    if (TYPE == RHO_PRED_V) {
        const float ab = abar[tb];
        c.sa = sqrtf(ab), c.sb = sqrtf(1.0f - ab);
    }
    c.w = w != nullptr ? w[tb] : 1.0f;
    c.kw = c.w * k2;
    return c;
}
template <int TYPE>
__device__ __forceinline__ float loss_term(const LossCoef& c, float p, float x, float e, float& acc) {
    const float g = TYPE == RHO_PRED_EPSILON ? e : (TYPE == RHO_PRED_SAMPLE ? x : __fmaf_rn(c.sa, e, -(c.sb * x)));
    const float d = p - g;
    acc = __fmaf_rn(c.w * d, d, acc);
    return c.kw * d;
}
template <int TYPE>
__global__ __launch_bounds__(256) void k_pred_loss_part(const float* __restrict__ pred, const float* __restrict__ x0,
                                                        const float* __restrict__ eps, const float* __restrict__ abar,
                                                        const float* __restrict__ w, const int64_t* __restrict__ t,
                                                        float* __restrict__ partials, float* __restrict__ grad, int64_t per_sample,
                                                        int64_t n, int64_t table_len, float inv_n, int vec,
                                                        int32_t* err_flag) {
    __shared__ float red[4];
    float acc = 0.0f;
    bool oob = false;
    const float k2 = 2.0f * inv_n;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    int64_t done = 0;
    if (vec) {                                   // per_sample >= 4 here: a piece touches at most two samples
        const int64_t n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(pred);
        const float4* x4 = reinterpret_cast<const float4*>(x0);
        const float4* e4 = reinterpret_cast<const float4*>(eps);
        float4* g4 = reinterpret_cast<float4*>(grad);
        const int64_t step = 4 * nthr, step_b = step / per_sample, step_r = step % per_sample;
        int64_t b = (4 * tid) / per_sample, r = (4 * tid) % per_sample;           // element 4 i is element r of sample b
        for (int64_t i = tid; i < n4; i += nthr) {
            const float4 p = p4[i], x = x4[i], e = e4[i];
            const LossCoef c = loss_coef<TYPE>(b, abar, w, t, table_len, k2, oob);
            float4 g;
            if (r + 3 < per_sample) {
                g.x = loss_term<TYPE>(c, p.x, x.x, e.x, acc);
                g.y = loss_term<TYPE>(c, p.y, x.y, e.y, acc);
                g.z = loss_term<TYPE>(c, p.z, x.z, e.z, acc);
                g.w = loss_term<TYPE>(c, p.w, x.w, e.w, acc);
            } else {                             // elements r + j >= per_sample belong to sample b + 1 (which exists: 4 i + j < n)
                const LossCoef c1 = loss_coef<TYPE>(b + 1, abar, w, t, table_len, k2, oob);
                g.x = loss_term<TYPE>(c, p.x, x.x, e.x, acc);
                g.y = loss_term<TYPE>(r + 1 < per_sample ? c : c1, p.y, x.y, e.y, acc);
                g.z = loss_term<TYPE>(r + 2 < per_sample ? c : c1, p.z, x.z, e.z, acc);
                g.w = loss_term<TYPE>(c1, p.w, x.w, e.w, acc);
            }
            if (grad) g4[i] = g;
            b += step_b, r += step_r;
            if (r >= per_sample) { r -= per_sample; b += 1; }
        }
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < n; i += nthr) {
        const LossCoef c = loss_coef<TYPE>(i / per_sample, abar, w, t, table_len, k2, oob);
        const float g = loss_term<TYPE>(c, pred[i], x0[i], eps[i], acc);
        if (grad) grad[i] = g;
    }
    if (err_flag != nullptr && __any(oob)) {
        if ((threadIdx.x & 63) == 0) atomicOr(err_flag, 4);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}

extern "C" int rho_pred_loss_ws(const float* pred, const float* x0, const float* eps, const float* alpha_bar, const float* w,
                                const int64_t* t, int64_t batch, int64_t per_sample, int64_t table_len, int pred_type, float* loss,
                                float* grad, float* partials, int64_t n_partials, int32_t* err_flag, void* stream) {
    if (!pred || !x0 || !eps || !alpha_bar || !t || !loss || !partials || batch <= 0 || per_sample <= 0 || table_len <= 0 ||
        n_partials < 1)
        return RHO_E_ARG;
    if (pred_type != RHO_PRED_EPSILON && pred_type != RHO_PRED_V && pred_type != RHO_PRED_SAMPLE) return RHO_E_ARG;
    if (batch > INT64_MAX / per_sample) return RHO_E_ARG;
    const int64_t n = batch * per_sample;
    int64_t g = grid_for(n, 256 * 8);
    if (g > n_partials) g = n_partials;
    const int vec = (per_sample >= 4 && (((uintptr_t)pred | (uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)grad) & 15) == 0) ? 1 : 0;
    const dim3 grid((unsigned)g), block(256);
    const float inv_n = 1.0f / (float)n;
    hipStream_t st = as_stream(stream);
    if (pred_type == RHO_PRED_EPSILON)
        hipLaunchKernelGGL(k_pred_loss_part<RHO_PRED_EPSILON>, grid, block, 0, st, pred, x0, eps, alpha_bar, w, t, partials, grad,
                           per_sample, n, table_len, inv_n, vec, err_flag);
    else if (pred_type == RHO_PRED_V)
        hipLaunchKernelGGL(k_pred_loss_part<RHO_PRED_V>, grid, block, 0, st, pred, x0, eps, alpha_bar, w, t, partials, grad,
                           per_sample, n, table_len, inv_n, vec, err_flag);
    else
        hipLaunchKernelGGL(k_pred_loss_part<RHO_PRED_SAMPLE>, grid, block, 0, st, pred, x0, eps, alpha_bar, w, t, partials, grad,
                           per_sample, n, table_len, inv_n, vec, err_flag);
    hipLaunchKernelGGL(k_mse_final, dim3(1), dim3(64), 0, as_stream(stream), partials, (int)g, loss);
    RHO_LAUNCH_CHECK();
    return 0;
}

// mean over all non-batch axes (layers.py:105-110, mean_flat): one workgroup per sample, fp32 in a fixed order
__global__ __launch_bounds__(256) void k_mean_flat(const float* __restrict__ x, float* __restrict__ out, int64_t per_sample) {
    __shared__ float red[4];
    const float* xs = x + (int64_t)blockIdx.x * per_sample;
    float acc = 0.0f;
    for (int64_t i = threadIdx.x; i < per_sample; i += 256) acc += xs[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)per_sample;
}
extern "C" int rho_mean_flat(const float* x, float* out, int64_t batch, int64_t per_sample, void* stream) {
    if (!x || !out || batch <= 0 || per_sample <= 0 || batch > 0x7FFFFFFF) return RHO_E_ARG;
    hipLaunchKernelGGL(k_mean_flat, dim3((unsigned)batch), dim3(256), 0, as_stream(stream), x, out, per_sample);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- AdamW
__global__ __launch_bounds__(256) void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                               float wd, float bc1, float rsqrt_bc2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i];
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        const float denom = sqrtf(vi) * rsqrt_bc2 + eps;
        pi -= (lr / bc1) * (mi / denom);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
    }
}

extern "C" int rho_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int32_t step, void* stream) {
    if (!p || !g || !m || !v || n <= 0 || step < 1) return RHO_E_ARG;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(k_adamw, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)));
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- embeddings
// One wave per output feature: the weight row stays in registers while the wave walks the batch.
// (B <= a few hundred, in_dim <= 1024: launch-latency bound)
template <int MAXK>  // in_dim <= 64*MAXK
__global__ __launch_bounds__(256) void k_linear(const float* __restrict__ x, const float* __restrict__ w,
                                                const float* __restrict__ bias, const float* __restrict__ add,
                                                float* __restrict__ out, int batch, int in_dim, int out_dim, int act_in,
                                                int act_out) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= out_dim) return;
    float wr[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        const int k = lane + 64 * j;
        wr[j] = (k < in_dim) ? w[(int64_t)o * in_dim + k] : 0.0f;
    }
    const float bo = bias ? bias[o] : 0.0f;
    for (int b = 0; b < batch; ++b) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXK; ++j) {
            const int k = lane + 64 * j;
            if (k < in_dim) {
                float xv = x[(int64_t)b * in_dim + k];
                if (act_in) xv = act_in == 1 ? xv / (1.0f + expf(-xv)) : act_other_f(xv, act_in);
                acc = fmaf(xv, wr[j], acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            float r = acc + bo;
            if (add) r += add[(int64_t)b * out_dim + o];
            if (act_out) r = act_out == 1 ? r / (1.0f + expf(-r)) : act_other_f(r, act_out);
            out[(int64_t)b * out_dim + o] = r;
        }
    }
}

extern "C" int rho_linear(const float* x, const float* w, const float* bias, const float* add, float* out, int64_t batch,
                          int64_t in_dim, int64_t out_dim, int act_in, int act_out, void* stream) {
    if (!x || !w || !out || batch <= 0 || in_dim <= 0 || out_dim <= 0 || in_dim > 2048) return RHO_E_ARG;
    dim3 grid((unsigned)((out_dim + 3) / 4)), block(256);
    if (in_dim <= 256)
        hipLaunchKernelGGL(k_linear<4>, grid, block, 0, as_stream(stream), x, w, bias, add, out, (int)batch, (int)in_dim,
                           (int)out_dim, act_in, act_out);
    else if (in_dim <= 1024)
        hipLaunchKernelGGL(k_linear<16>, grid, block, 0, as_stream(stream), x, w, bias, add, out, (int)batch, (int)in_dim,
                           (int)out_dim, act_in, act_out);
    else
        hipLaunchKernelGGL(k_linear<32>, grid, block, 0, as_stream(stream), x, w, bias, add, out, (int)batch, (int)in_dim,
                           (int)out_dim, act_in, act_out);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- layout
template <typename T>
__global__ __launch_bounds__(256) void k_pack_input(const float* __restrict__ x, T* __restrict__ y, int64_t n, int64_t c,
                                                    int64_t s, int64_t cpad) {
    // thread per (sample, position, 16-byte piece): consecutive lanes write consecutive 16-byte pieces of the
    // channels-last rows (one scalar 2-byte store per channel ran at 0.49 TB/s); the reads of channel ch are
    // coalesced across the lanes that share a piece index
    constexpr int PE = 16 / (int)sizeof(T);
    const int64_t ppr = cpad / PE;                      // pieces per row (cpad is a multiple of 32)
    const int64_t total = n * s * ppr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t piece = i % ppr, pos = i / ppr;
        const int64_t b = pos / s, p = pos % s;
        float v[PE];
#pragma unroll
        for (int j = 0; j < PE; ++j) {
            const int64_t ch = piece * PE + j;
            v[j] = ch < c ? x[(b * c + ch) * s + p] : 0.0f;
        }
        uint4 o;
        if constexpr (sizeof(T) == 2) {
            o = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
        } else {
            o = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
        }
        reinterpret_cast<uint4*>(y)[i] = o;
    }
}

extern "C" int rho_pack_input(const float* x, void* y, int dtype, int64_t n, int64_t c, int64_t s, int64_t cpad, void* stream) {
    if (!x || !y || n <= 0 || c <= 0 || s <= 0 || cpad < c) return RHO_E_ARG;
    if (cpad % 8 != 0) return RHO_E_ALIGN;
    dim3 grid(grid_for(n * s * (cpad / (dtype == RHO_BF16 ? 8 : 4)), 256)), block(256);
    if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_pack_input<bf16_raw>, grid, block, 0, as_stream(stream), x, (bf16_raw*)y, n, c, s, cpad);
    else if (dtype == RHO_F32)
        hipLaunchKernelGGL(k_pack_input<float>, grid, block, 0, as_stream(stream), x, (float*)y, n, c, s, cpad);
    else
        return RHO_E_ARG;
    RHO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The two convolutions at the ends of the UNet have one channel on one side (1 -> mc stem, mc -> 1 head): as 3x3x3
// implicit GEMMs they pad that side to 32 and waste 31/32 of the matrix work (1.2 + 1.6 ms of a 137 ms step).  Both are
// 1x1x1 GEMMs in disguise:
//   stem:  y[pos][co] = sum_k W[co][k] * X27[pos][k],  X27[pos][ci * taps + tap] = x[ci][pos + off(tap)]   (k_im2col_taps)
//   head:  out[pos]   = bias + sum_tap T[pos + off(tap)][tap],  T[q][tap] = sum_c W[tap][c] * act[q][c]     (k_tap_gather_sum)
// so the engine's inference plans run them through the 1x1x1 path with these two HBM-rate helpers around it.
// (kernel extents are template parameters: with run-time extents the tap -> (dz, dy, dx) divisions of the 32 columns cost 3000
//  VALU instructions per position, 0.5 ms for 8.4 M positions instead of the 0.15 ms the bytes take)
// Round 4: the 1-channel 3x3x3 case (also the GEMM-shaped backward of the stem / head in training plans) with FOUR threads per
// position, one 16-byte piece (8 taps) each: consecutive threads write consecutive 16 bytes - 1 KB per wave store instead of four
// 64-byte-strided stores per thread (1.5 -> ~3 TB/s on the 0.54 GB operand).
__global__ __launch_bounds__(256) void k_im2col_333_c1(const float* __restrict__ x, bf16_raw* __restrict__ out, int D, int H, int W,
                                                       int64_t total) {
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gi >> 2;                        // output position
    const int piece = (int)(gi & 3);
    if (i >= total) return;
    const int64_t S = (int64_t)D * H * W;
    const int64_t n = i / S;
    const int64_t ps = i - n * S;
    const int w_ = (int)(ps % W), h_ = (int)((ps / W) % H), d_ = (int)(ps / ((int64_t)W * H));
    const float* xs = x + n * S + ps;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int kk = piece * 8 + j;
        float val = 0.0f;
        if (kk < 27) {
            const int dz = kk / 9 - 1, dy = (kk / 3) % 3 - 1, dx = kk % 3 - 1;
            const int z = d_ + dz, y = h_ + dy, xx = w_ + dx;
            if (z >= 0 && z < D && y >= 0 && y < H && xx >= 0 && xx < W) val = xs[((int64_t)dz * H + dy) * W + dx];
        }
        v[j] = val;
    }
    *reinterpret_cast<uint4*>(out + i * 32 + piece * 8) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                                                     pack_bf16x2(v[6], v[7]));
}

template <int KD, int KH, int KW>
__global__ __launch_bounds__(256) void k_im2col_taps(const float* __restrict__ x, bf16_raw* __restrict__ out, int cin, int D, int H,
                                                     int W, int cpad, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one output position
    if (i >= total) return;
    constexpr int TAPS = KD * KH * KW;
    const int64_t S = (int64_t)D * H * W;
    const int64_t n = i / S;
    const int64_t ps = i - n * S;
    const int w_ = (int)(ps % W), h_ = (int)((ps / W) % H), d_ = (int)(ps / ((int64_t)W * H));
    bf16_raw* o = out + i * cpad;
    const float* xs = x + n * cin * S + ps;
    for (int k0 = 0; k0 < cpad; k0 += 8) {
        float v[8];
        if (cin == 1 && k0 + 8 <= 32) {                 // the common case, fully unrolled: compile-time tap offsets
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.0f;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                if (kk >= k0 && kk < k0 + 8 && kk < TAPS) {
                    const int dz = kk / (KH * KW) - KD / 2, dy = (kk / KW) % KH - KH / 2, dx = kk % KW - KW / 2;
                    const int z = d_ + dz, y = h_ + dy, xx = w_ + dx;
                    if (z >= 0 && z < D && y >= 0 && y < H && xx >= 0 && xx < W) v[kk & 7] = xs[((int64_t)dz * H + dy) * W + dx];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                float val = 0.0f;
                if (k < cin * TAPS) {
                    const int ci = k / TAPS, tap = k - ci * TAPS;
                    const int dz = tap / (KH * KW) - KD / 2, dy = (tap / KW) % KH - KH / 2, dx = tap % KW - KW / 2;
                    const int z = d_ + dz, y = h_ + dy, xx = w_ + dx;
                    if (z >= 0 && z < D && y >= 0 && y < H && xx >= 0 && xx < W) val = xs[ci * S + ((int64_t)dz * H + dy) * W + dx];
                }
                v[j] = val;
            }
        }
        *reinterpret_cast<uint4*>(o + k0) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                                                       pack_bf16x2(v[6], v[7]));
    }
}

extern "C" int rho_im2col_taps(const float* x, void* out, int dtype, int64_t n, int64_t cin, int64_t d, int64_t h, int64_t w,
                               int kd, int kh, int kw, int64_t cpad, void* stream) {
    if (!x || !out || n <= 0 || cin <= 0 || d <= 0 || h <= 0 || w <= 0) return RHO_E_ARG;
    if (dtype != RHO_BF16) return RHO_E_ARG;
    if (cpad % 8 != 0 || cpad < cin * kd * kh * kw) return RHO_E_ALIGN;
    const int64_t total = n * d * h * w;
    dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (kd == 3 && kh == 3 && kw == 3 && cin == 1 && cpad == 32 && total < (1LL << 40))
        hipLaunchKernelGGL(k_im2col_333_c1, dim3((unsigned)((total * 4 + 255) / 256)), block, 0, as_stream(stream), x, (bf16_raw*)out, (int)d,
                           (int)h, (int)w, total);
    else if (kd == 3 && kh == 3 && kw == 3)
        hipLaunchKernelGGL((k_im2col_taps<3, 3, 3>), grid, block, 0, as_stream(stream), x, (bf16_raw*)out, (int)cin, (int)d, (int)h, (int)w,
                           (int)cpad, total);
    else if (kd == 1 && kh == 3 && kw == 3)
        hipLaunchKernelGGL((k_im2col_taps<1, 3, 3>), grid, block, 0, as_stream(stream), x, (bf16_raw*)out, (int)cin, (int)d, (int)h, (int)w,
                           (int)cpad, total);
    else if (kd == 1 && kh == 1 && kw == 3)
        hipLaunchKernelGGL((k_im2col_taps<1, 1, 3>), grid, block, 0, as_stream(stream), x, (bf16_raw*)out, (int)cin, (int)d, (int)h, (int)w,
                           (int)cpad, total);
    else
        return RHO_E_SHAPE;
    RHO_LAUNCH_CHECK();
    return 0;
}

template <int KD, int KH, int KW>
__global__ __launch_bounds__(256) void k_tap_gather_sum(const bf16_raw* __restrict__ t, const float* __restrict__ bias,
                                                        float* __restrict__ out, int D, int H, int W, int cpad, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one output position
    if (i >= total) return;
    const int64_t S = (int64_t)D * H * W;
    const int64_t n = i / S;
    const int64_t ps = i - n * S;
    const int w_ = (int)(ps % W), h_ = (int)((ps / W) % H), d_ = (int)(ps / ((int64_t)W * H));
    const bf16_raw* tp = t + i * cpad;
    float v[KD * KH * KW];
#pragma unroll
    for (int tap = 0; tap < KD * KH * KW; ++tap) {          // all loads first (independent), then the ordered fp32 sum
        const int dz = tap / (KH * KW) - KD / 2, dy = (tap / KW) % KH - KH / 2, dx = tap % KW - KW / 2;
        const int z = d_ + dz, y = h_ + dy, xx = w_ + dx;
        const bool in = z >= 0 && z < D && y >= 0 && y < H && xx >= 0 && xx < W;
        v[tap] = in ? bf16_to_f32(tp[(((int64_t)dz * H + dy) * W + dx) * cpad + tap]) : 0.0f;
    }
    float acc = bias ? bias[0] : 0.0f;
#pragma unroll
    for (int tap = 0; tap < KD * KH * KW; ++tap) acc += v[tap];
    out[i] = acc;
}

extern "C" int rho_tap_gather_sum(const void* t, int dtype, int64_t n, int64_t d, int64_t h, int64_t w, int kd, int kh, int kw,
                                  int64_t cpad, const float* bias, float* out, void* stream) {
    if (!t || !out || n <= 0 || d <= 0 || h <= 0 || w <= 0) return RHO_E_ARG;
    if (dtype != RHO_BF16) return RHO_E_ARG;
    if (cpad < kd * kh * kw) return RHO_E_ALIGN;
    const int64_t total = n * d * h * w;
    dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (kd == 3 && kh == 3 && kw == 3)
        hipLaunchKernelGGL((k_tap_gather_sum<3, 3, 3>), grid, block, 0, as_stream(stream), (const bf16_raw*)t, bias, out, (int)d, (int)h,
                           (int)w, (int)cpad, total);
    else if (kd == 1 && kh == 3 && kw == 3)
        hipLaunchKernelGGL((k_tap_gather_sum<1, 3, 3>), grid, block, 0, as_stream(stream), (const bf16_raw*)t, bias, out, (int)d, (int)h,
                           (int)w, (int)cpad, total);
    else if (kd == 1 && kh == 1 && kw == 3)
        hipLaunchKernelGGL((k_tap_gather_sum<1, 1, 3>), grid, block, 0, as_stream(stream), (const bf16_raw*)t, bias, out, (int)d, (int)h,
                           (int)w, (int)cpad, total);
    else
        return RHO_E_SHAPE;
    RHO_LAUNCH_CHECK();
    return 0;
}

// ================================================================================================ backward helpers

// nearest x2 on H and/or W of a channels-last tensor, 16-byte pieces (materialised only for the wgrad of Upsample.conv)
__global__ __launch_bounds__(256) void k_upsample2x(const uint4* __restrict__ x, uint4* __restrict__ y, int64_t nd, int h, int w,
                                                    int cpieces, int uh, int uw) {
    const int ho = uh ? 2 * h : h, wo = uw ? 2 * w : w;
    const int64_t total = nd * ho * wo * cpieces;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cp = (int)(i % cpieces);
        int64_t r = i / cpieces;
        const int ow = (int)(r % wo); r /= wo;
        const int oh = (int)(r % ho); r /= ho;
        const int ih = uh ? oh >> 1 : oh, iw = uw ? ow >> 1 : ow;
        y[i] = x[((r * h + ih) * w + iw) * cpieces + cp];
    }
}

extern "C" int rho_upsample2x(const void* x, void* y, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int up_h,
                              int up_w, void* stream) {
    const int esz = dtype == RHO_BF16 ? 2 : 4;
    if (!x || !y || n_times_d <= 0 || h <= 0 || w <= 0 || c <= 0 || (c * esz) % 16) return RHO_E_ARG;
    const int cp = (int)(c * esz / 16);
    const int64_t total = n_times_d * (up_h ? 2 * h : h) * (up_w ? 2 * w : w) * cp;
    hipLaunchKernelGGL(k_upsample2x, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), (const uint4*)x, (uint4*)y, n_times_d,
                       (int)h, (int)w, cp, up_h, up_w);
    RHO_LAUNCH_CHECK();
    return 0;
}

// dx[.., h, w, c] (+)= sum over the 2x2 (or 1x2) children of dy: backward of the nearest upsample
template <typename T>
__global__ __launch_bounds__(256) void k_pool2x_sum(const T* __restrict__ dy, T* __restrict__ dx, int64_t nd, int h, int w, int c,
                                                    int uh, int uw, int accumulate) {
    // one 16-byte channel piece per thread (the scalar form ran at 1.8 TB/s)
    constexpr int PE = 16 / (int)sizeof(T);
    const int ho = uh ? 2 * h : h, wo = uw ? 2 * w : w;
    const int cp = c / PE;
    const int64_t total = nd * h * w * cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pc = (int)(i % cp);
        int64_t r = i / cp;
        const int iw = (int)(r % w); r /= w;
        const int ih = (int)(r % h); r /= h;
        float acc[PE];
#pragma unroll
        for (int e = 0; e < PE; ++e) acc[e] = 0.0f;
        for (int a = 0; a <= uh; ++a)
            for (int b = 0; b <= uw; ++b) {
                const int64_t o = ((r * ho + (uh ? 2 * ih + a : ih)) * wo + (uw ? 2 * iw + b : iw)) * c + pc * PE;
                const uint4 u = *reinterpret_cast<const uint4*>(dy + o);
                if constexpr (sizeof(T) == 2) {
                    acc[0] += __uint_as_float(u.x << 16); acc[1] += __uint_as_float(u.x & 0xFFFF0000u);
                    acc[2] += __uint_as_float(u.y << 16); acc[3] += __uint_as_float(u.y & 0xFFFF0000u);
                    acc[4] += __uint_as_float(u.z << 16); acc[5] += __uint_as_float(u.z & 0xFFFF0000u);
                    acc[6] += __uint_as_float(u.w << 16); acc[7] += __uint_as_float(u.w & 0xFFFF0000u);
                } else {
                    acc[0] += __uint_as_float(u.x); acc[1] += __uint_as_float(u.y); acc[2] += __uint_as_float(u.z); acc[3] += __uint_as_float(u.w);
                }
            }
        T* dst = dx + (i / cp) * c + pc * PE;
        if (accumulate) {
            const uint4 u = *reinterpret_cast<const uint4*>(dst);
            if constexpr (sizeof(T) == 2) {
                acc[0] += __uint_as_float(u.x << 16); acc[1] += __uint_as_float(u.x & 0xFFFF0000u);
                acc[2] += __uint_as_float(u.y << 16); acc[3] += __uint_as_float(u.y & 0xFFFF0000u);
                acc[4] += __uint_as_float(u.z << 16); acc[5] += __uint_as_float(u.z & 0xFFFF0000u);
                acc[6] += __uint_as_float(u.w << 16); acc[7] += __uint_as_float(u.w & 0xFFFF0000u);
            } else {
                acc[0] += __uint_as_float(u.x); acc[1] += __uint_as_float(u.y); acc[2] += __uint_as_float(u.z); acc[3] += __uint_as_float(u.w);
            }
        }
        if constexpr (sizeof(T) == 2)
            *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]),
                                                        pack_bf16x2(acc[6], acc[7]));
        else
            *reinterpret_cast<uint4*>(dst) = make_uint4(__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]),
                                                        __float_as_uint(acc[3]));
    }
}

extern "C" int rho_pool2x_sum(const void* dy, void* dx, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int up_h,
                              int up_w, int accumulate, void* stream) {
    if (!dy || !dx || n_times_d <= 0 || h <= 0 || w <= 0 || c <= 0) return RHO_E_ARG;
    if (c % 8 != 0) return RHO_E_ALIGN;
    dim3 grid(grid_for(n_times_d * h * w * (c / (dtype == RHO_BF16 ? 8 : 4)), 256)), block(256);
    if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_pool2x_sum<bf16_raw>, grid, block, 0, as_stream(stream), (const bf16_raw*)dy, (bf16_raw*)dx, n_times_d, (int)h,
                           (int)w, (int)c, up_h, up_w, accumulate);
    else if (dtype == RHO_F32)
        hipLaunchKernelGGL(k_pool2x_sum<float>, grid, block, 0, as_stream(stream), (const float*)dy, (float*)dx, n_times_d, (int)h, (int)w,
                           (int)c, up_h, up_w, accumulate);
    else
        return RHO_E_ARG;
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- average pooling (K12)
// avg_pool_nd(dims, kernel_size = stride, stride = stride), stride 2 (3-D: (1, 2, 2)), layers.py:91-102 / unet_v2.py:165: the
// Downsample of conv_resample = False and of ResBlock(down = True).  Channels-last, one 16-byte channel piece per thread;
// output extent floor(h / 2) (PyTorch's ceil_mode = False: an odd last row / column is dropped).
template <typename T>
__global__ __launch_bounds__(256) void k_avgpool2x(const T* __restrict__ x, T* __restrict__ y, int64_t nd, int h, int w, int c, int fh,
                                                   int fw) {
    constexpr int PE = 16 / (int)sizeof(T);
    const int ho = fh ? h >> 1 : h, wo = fw ? w >> 1 : w;
    const int cp = c / PE;
    const float scale = 1.0f / (float)((fh ? 2 : 1) * (fw ? 2 : 1));
    const int64_t total = nd * ho * wo * cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pc = (int)(i % cp);
        int64_t r = i / cp;
        const int ow = (int)(r % wo); r /= wo;
        const int oh = (int)(r % ho); r /= ho;
        float acc[PE];
#pragma unroll
        for (int e = 0; e < PE; ++e) acc[e] = 0.0f;
        for (int a = 0; a <= fh; ++a)
            for (int b = 0; b <= fw; ++b) {
                const int64_t o = ((r * h + (fh ? 2 * oh + a : oh)) * w + (fw ? 2 * ow + b : ow)) * c + pc * PE;
                const uint4 u = *reinterpret_cast<const uint4*>(x + o);
                if constexpr (sizeof(T) == 2) {
                    acc[0] += __uint_as_float(u.x << 16); acc[1] += __uint_as_float(u.x & 0xFFFF0000u);
                    acc[2] += __uint_as_float(u.y << 16); acc[3] += __uint_as_float(u.y & 0xFFFF0000u);
                    acc[4] += __uint_as_float(u.z << 16); acc[5] += __uint_as_float(u.z & 0xFFFF0000u);
                    acc[6] += __uint_as_float(u.w << 16); acc[7] += __uint_as_float(u.w & 0xFFFF0000u);
                } else {
                    acc[0] += __uint_as_float(u.x); acc[1] += __uint_as_float(u.y); acc[2] += __uint_as_float(u.z); acc[3] += __uint_as_float(u.w);
                }
            }
        T* dst = y + (i / cp) * c + pc * PE;
        if constexpr (sizeof(T) == 2)
            *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(acc[0] * scale, acc[1] * scale), pack_bf16x2(acc[2] * scale, acc[3] * scale),
                                                        pack_bf16x2(acc[4] * scale, acc[5] * scale), pack_bf16x2(acc[6] * scale, acc[7] * scale));
        else
            *reinterpret_cast<uint4*>(dst) = make_uint4(__float_as_uint(acc[0] * scale), __float_as_uint(acc[1] * scale),
                                                        __float_as_uint(acc[2] * scale), __float_as_uint(acc[3] * scale));
    }
}

extern "C" int rho_avgpool2x(const void* x, void* y, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int pool_h, int pool_w,
                             void* stream) {
    if (!x || !y || n_times_d <= 0 || h <= 0 || w <= 0 || c <= 0 || (pool_h && h < 2) || (pool_w && w < 2)) return RHO_E_ARG;
    if (dtype != RHO_BF16 && dtype != RHO_F32) return RHO_E_ARG;
    const int pe = dtype == RHO_BF16 ? 8 : 4;
    if (c % pe != 0) return RHO_E_ALIGN;
    const int64_t total = n_times_d * (pool_h ? h / 2 : h) * (pool_w ? w / 2 : w) * (c / pe);
    dim3 grid(grid_for(total, 256)), block(256);
    if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_avgpool2x<bf16_raw>, grid, block, 0, as_stream(stream), (const bf16_raw*)x, (bf16_raw*)y, n_times_d, (int)h, (int)w,
                           (int)c, pool_h, pool_w);
    else
        hipLaunchKernelGGL(k_avgpool2x<float>, grid, block, 0, as_stream(stream), (const float*)x, (float*)y, n_times_d, (int)h, (int)w, (int)c,
                           pool_h, pool_w);
    RHO_LAUNCH_CHECK();
    return 0;
}

// backward: dx[.., ih, iw, :] (+)= dy[.., ih / 2, iw / 2, :] / (window size); rows / columns the pooling dropped receive 0
template <typename T>
__global__ __launch_bounds__(256) void k_avgpool2x_bwd(const T* __restrict__ dy, T* __restrict__ dx, int64_t nd, int h, int w, int c, int fh,
                                                       int fw, int accumulate) {
    constexpr int PE = 16 / (int)sizeof(T);
    const int ho = fh ? h >> 1 : h, wo = fw ? w >> 1 : w;
    const int cp = c / PE;
    const float scale = 1.0f / (float)((fh ? 2 : 1) * (fw ? 2 : 1));
    const int64_t total = nd * h * w * cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int pc = (int)(i % cp);
        int64_t r = i / cp;
        const int iw = (int)(r % w); r /= w;
        const int ih = (int)(r % h); r /= h;
        const int oh = fh ? ih >> 1 : ih, ow = fw ? iw >> 1 : iw;
        float acc[PE];
#pragma unroll
        for (int e = 0; e < PE; ++e) acc[e] = 0.0f;
        if (oh < ho && ow < wo) {
            const uint4 u = *reinterpret_cast<const uint4*>(dy + ((r * ho + oh) * wo + ow) * c + pc * PE);
            if constexpr (sizeof(T) == 2) {
                acc[0] = __uint_as_float(u.x << 16) * scale; acc[1] = __uint_as_float(u.x & 0xFFFF0000u) * scale;
                acc[2] = __uint_as_float(u.y << 16) * scale; acc[3] = __uint_as_float(u.y & 0xFFFF0000u) * scale;
                acc[4] = __uint_as_float(u.z << 16) * scale; acc[5] = __uint_as_float(u.z & 0xFFFF0000u) * scale;
                acc[6] = __uint_as_float(u.w << 16) * scale; acc[7] = __uint_as_float(u.w & 0xFFFF0000u) * scale;
            } else {
                acc[0] = __uint_as_float(u.x) * scale; acc[1] = __uint_as_float(u.y) * scale;
                acc[2] = __uint_as_float(u.z) * scale; acc[3] = __uint_as_float(u.w) * scale;
            }
        }
        T* dst = dx + (i / cp) * c + pc * PE;
        if (accumulate) {
            const uint4 u = *reinterpret_cast<const uint4*>(dst);
            if constexpr (sizeof(T) == 2) {
                acc[0] += __uint_as_float(u.x << 16); acc[1] += __uint_as_float(u.x & 0xFFFF0000u);
                acc[2] += __uint_as_float(u.y << 16); acc[3] += __uint_as_float(u.y & 0xFFFF0000u);
                acc[4] += __uint_as_float(u.z << 16); acc[5] += __uint_as_float(u.z & 0xFFFF0000u);
                acc[6] += __uint_as_float(u.w << 16); acc[7] += __uint_as_float(u.w & 0xFFFF0000u);
            } else {
                acc[0] += __uint_as_float(u.x); acc[1] += __uint_as_float(u.y); acc[2] += __uint_as_float(u.z); acc[3] += __uint_as_float(u.w);
            }
        }
        if constexpr (sizeof(T) == 2)
            *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]),
                                                        pack_bf16x2(acc[6], acc[7]));
        else
            *reinterpret_cast<uint4*>(dst) = make_uint4(__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]),
                                                        __float_as_uint(acc[3]));
    }
}

extern "C" int rho_avgpool2x_bwd(const void* dy, void* dx, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int pool_h,
                                 int pool_w, int accumulate, void* stream) {
    if (!dy || !dx || n_times_d <= 0 || h <= 0 || w <= 0 || c <= 0 || (pool_h && h < 2) || (pool_w && w < 2)) return RHO_E_ARG;
    if (dtype != RHO_BF16 && dtype != RHO_F32) return RHO_E_ARG;
    const int pe = dtype == RHO_BF16 ? 8 : 4;
    if (c % pe != 0) return RHO_E_ALIGN;
    dim3 grid(grid_for(n_times_d * h * w * (c / pe), 256)), block(256);
    if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_avgpool2x_bwd<bf16_raw>, grid, block, 0, as_stream(stream), (const bf16_raw*)dy, (bf16_raw*)dx, n_times_d, (int)h,
                           (int)w, (int)c, pool_h, pool_w, accumulate);
    else
        hipLaunchKernelGGL(k_avgpool2x_bwd<float>, grid, block, 0, as_stream(stream), (const float*)dy, (float*)dx, n_times_d, (int)h, (int)w,
                           (int)c, pool_h, pool_w, accumulate);
    RHO_LAUNCH_CHECK();
    return 0;
}

// Backward of rho_linear (out = W act(x) + b [+ add]):  dW[o,k] (+)= sum_b dout[b,o] act(x[b,k]),  db[o] (+)= sum_b dout[b,o]
__global__ __launch_bounds__(256) void k_linear_bwd_w(const float* __restrict__ dout, const float* __restrict__ x,
                                                      float* __restrict__ dw, float* __restrict__ db, int batch, int in_dim,
                                                      int out_dim, int act_in, int accumulate, int64_t dstride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)out_dim * in_dim) return;
    const int o = (int)(i / in_dim), k = (int)(i % in_dim);
    float acc = 0.0f, accb = 0.0f;
    for (int b = 0; b < batch; ++b) {
        float xv = x[(int64_t)b * in_dim + k];
        if (act_in) xv = act_in == 1 ? xv / (1.0f + expf(-xv)) : act_other_f(xv, act_in);
        const float g = dout[(int64_t)b * dstride + o];
        acc = fmaf(g, xv, acc);
        accb += g;
    }
    dw[i] = accumulate ? dw[i] + acc : acc;
    if (k == 0 && db) db[o] = accumulate ? db[o] + accb : accb;
}

// db alone (dw == NULL): the bias sum of k_linear_bwd_w in the same batch order, one thread per output feature
__global__ __launch_bounds__(256) void k_linear_bwd_b(const float* __restrict__ dout, float* __restrict__ db, int batch, int out_dim,
                                                      int accumulate, int64_t dstride) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= out_dim) return;
    float accb = 0.0f;
    for (int b = 0; b < batch; ++b) accb += dout[(int64_t)b * dstride + o];
    db[o] = accumulate ? db[o] + accb : accb;
}

// dx[b,k] += act'(x[b,k]) * sum_o dout[b,o] W[o,k], the o range dealt to gridDim.y slices of 64 that add with fp32 atomics
// (a thread per (b,k) walking all of out_dim was 32 workgroups x 1024 dependent iterations: 0.2-0.4 ms per FiLM linear,
// 4.7 ms per training step for 4 MFLOP of work).  dx must hold the value to accumulate onto (zeroed by the caller side).
__global__ __launch_bounds__(256) void k_linear_bwd_x(const float* __restrict__ dout, const float* __restrict__ w,
                                                      const float* __restrict__ x, float* __restrict__ dx, int batch, int in_dim,
                                                      int out_dim, int act_in, int64_t dstride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)batch * in_dim) return;
    const int b = (int)(i / in_dim), k = (int)(i % in_dim);
    const int o0 = blockIdx.y * 64, o1 = min(o0 + 64, out_dim);
    float acc = 0.0f;
#pragma unroll 8
    for (int o = o0; o < o1; ++o) acc = fmaf(dout[(int64_t)b * dstride + o], w[(int64_t)o * in_dim + k], acc);
    if (act_in == 1) {
        const float u = x[i];
        const float s = 1.0f / (1.0f + expf(-u));
        acc *= s * (1.0f + u * (1.0f - s));
    } else if (act_in) {
        acc *= dact_other_f(x[i], act_in);
    }
    atomicAdd(dx + i, acc);
}

// ordered form (rho_get_deterministic): one thread walks all of out_dim in index order - no atomics, 0.2-0.4 ms per FiLM linear
__global__ __launch_bounds__(256) void k_linear_bwd_x_det(const float* __restrict__ dout, const float* __restrict__ w,
                                                          const float* __restrict__ x, float* __restrict__ dx, int batch, int in_dim,
                                                          int out_dim, int act_in, int64_t dstride, int acc_dx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)batch * in_dim) return;
    const int b = (int)(i / in_dim), k = (int)(i % in_dim);
    float acc = 0.0f;
#pragma unroll 8
    for (int o = 0; o < out_dim; ++o) acc = fmaf(dout[(int64_t)b * dstride + o], w[(int64_t)o * in_dim + k], acc);
    if (act_in == 1) {
        const float u = x[i];
        const float s = 1.0f / (1.0f + expf(-u));
        acc *= s * (1.0f + u * (1.0f - s));
    } else if (act_in) {
        acc *= dact_other_f(x[i], act_in);
    }
    dx[i] = acc_dx ? dx[i] + acc : acc;
}

extern "C" int rho_linear_bwd(const float* dout, int64_t dout_stride, const float* x, const float* w, float* dw, float* db,
                              float* dx, int64_t batch, int64_t in_dim, int64_t out_dim, int act_in, int acc_params, int acc_dx,
                              void* stream) {
    if (!dout || !x || !w || batch <= 0 || in_dim <= 0 || out_dim <= 0) return RHO_E_ARG;
    const int64_t dstride = dout_stride > 0 ? dout_stride : out_dim;
    if (dw) {
        hipLaunchKernelGGL(k_linear_bwd_w, dim3((unsigned)((out_dim * in_dim + 255) / 256)), dim3(256), 0, as_stream(stream), dout, x, dw,
                           db, (int)batch, (int)in_dim, (int)out_dim, act_in, acc_params, dstride);
    } else if (db) {
        hipLaunchKernelGGL(k_linear_bwd_b, dim3((unsigned)((out_dim + 255) / 256)), dim3(256), 0, as_stream(stream), dout, db, (int)batch,
                           (int)out_dim, acc_params, dstride);
    }
    if (dx && rho_get_deterministic()) {
        hipLaunchKernelGGL(k_linear_bwd_x_det, dim3((unsigned)((batch * in_dim + 255) / 256)), dim3(256), 0, as_stream(stream), dout, w, x,
                           dx, (int)batch, (int)in_dim, (int)out_dim, act_in, dstride, acc_dx);
    } else if (dx) {
        if (!acc_dx) {
            hipError_t e = hipMemsetAsync(dx, 0, (size_t)batch * in_dim * sizeof(float), as_stream(stream));
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(k_linear_bwd_x, dim3((unsigned)((batch * in_dim + 255) / 256), (unsigned)((out_dim + 63) / 64)), dim3(256), 0,
                           as_stream(stream), dout, w, x, dx, (int)batch, (int)in_dim, (int)out_dim, act_in, dstride);
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

// ExponentialMovingAverage.update (rho_diffusion/ema.py:41-60): shadow -= (1 - frac) * (shadow - param), float32, in the
// reference's operation order (sub, mul, sub; no contraction) so a parameter-by-parameter comparison is bit-exact.
__global__ __launch_bounds__(256) void k_ema_update(float* __restrict__ shadow, const float* __restrict__ param, int64_t n, float omf) {
#pragma clang fp contract(off)
    const int64_t n4 = n >> 2;
    const bool vec = ((((uintptr_t)shadow | (uintptr_t)param) & 15) == 0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (vec) {
        float4* s4 = reinterpret_cast<float4*>(shadow);
        const float4* p4 = reinterpret_cast<const float4*>(param);
        for (int64_t i = tid; i < n4; i += stride) {
            float4 a = s4[i];
            const float4 b = p4[i];
            float d;
            d = a.x - b.x; d = omf * d; a.x = a.x - d;
            d = a.y - b.y; d = omf * d; a.y = a.y - d;
            d = a.z - b.z; d = omf * d; a.z = a.z - d;
            d = a.w - b.w; d = omf * d; a.w = a.w - d;
            s4[i] = a;
        }
        for (int64_t i = (n4 << 2) + tid; i < n; i += stride) {
            float d = shadow[i] - param[i];
            d = omf * d;
            shadow[i] = shadow[i] - d;
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) {
            float d = shadow[i] - param[i];
            d = omf * d;
            shadow[i] = shadow[i] - d;
        }
    }
}

extern "C" int rho_ema_update(float* shadow, const float* param, int64_t n, float one_minus_frac, void* stream) {
    if (!shadow || !param || n <= 0) return RHO_E_ARG;
    hipLaunchKernelGGL(k_ema_update, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, as_stream(stream), shadow, param, n, one_minus_frac);
    RHO_LAUNCH_CHECK();
    return 0;
}

// dst += src (channels-last activations / gradients), 16-byte pieces
template <typename T>
__global__ __launch_bounds__(256) void k_add_inplace(T* __restrict__ dst, const T* __restrict__ src, int64_t n) {
    constexpr int PE = 16 / (int)sizeof(T);
    const int64_t np = n / PE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
        uint4 a = reinterpret_cast<const uint4*>(dst)[i];
        const uint4 b = reinterpret_cast<const uint4*>(src)[i];
        if constexpr (sizeof(T) == 2) {
            a.x = pack_bf16x2(__uint_as_float(a.x << 16) + __uint_as_float(b.x << 16), __uint_as_float(a.x & 0xFFFF0000u) + __uint_as_float(b.x & 0xFFFF0000u));
            a.y = pack_bf16x2(__uint_as_float(a.y << 16) + __uint_as_float(b.y << 16), __uint_as_float(a.y & 0xFFFF0000u) + __uint_as_float(b.y & 0xFFFF0000u));
            a.z = pack_bf16x2(__uint_as_float(a.z << 16) + __uint_as_float(b.z << 16), __uint_as_float(a.z & 0xFFFF0000u) + __uint_as_float(b.z & 0xFFFF0000u));
            a.w = pack_bf16x2(__uint_as_float(a.w << 16) + __uint_as_float(b.w << 16), __uint_as_float(a.w & 0xFFFF0000u) + __uint_as_float(b.w & 0xFFFF0000u));
        } else {
            a.x = __float_as_uint(__uint_as_float(a.x) + __uint_as_float(b.x));
            a.y = __float_as_uint(__uint_as_float(a.y) + __uint_as_float(b.y));
            a.z = __float_as_uint(__uint_as_float(a.z) + __uint_as_float(b.z));
            a.w = __float_as_uint(__uint_as_float(a.w) + __uint_as_float(b.w));
        }
        reinterpret_cast<uint4*>(dst)[i] = a;
    }
}

extern "C" int rho_add_inplace(void* dst, const void* src, int dtype, int64_t n, void* stream) {
    const int pe = dtype == RHO_BF16 ? 8 : 4;
    if (!dst || !src || n <= 0 || n % pe) return RHO_E_ARG;
    if (dtype == RHO_BF16)
        hipLaunchKernelGGL(k_add_inplace<bf16_raw>, dim3(grid_for(n / pe, 256)), dim3(256), 0, as_stream(stream), (bf16_raw*)dst, (const bf16_raw*)src, n);
    else if (dtype == RHO_F32)
        hipLaunchKernelGGL(k_add_inplace<float>, dim3(grid_for(n / pe, 256)), dim3(256), 0, as_stream(stream), (float*)dst, (const float*)src, n);
    else
        return RHO_E_ARG;
    RHO_LAUNCH_CHECK();
    return 0;
}

// x *= *scale_dev  (upstream scalar of loss.backward(), read on the device: no host sync)
__global__ __launch_bounds__(256) void k_scale_dev(float* __restrict__ x, const float* __restrict__ scale_dev, int64_t n) {
    const float sc = *scale_dev;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= sc;
}
extern "C" int rho_scale_by_device_scalar(float* x, const float* scale_dev, int64_t n, void* stream) {
    if (!x || !scale_dev || n <= 0) return RHO_E_ARG;
    hipLaunchKernelGGL(k_scale_dev, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), x, scale_dev, n);
    RHO_LAUNCH_CHECK();
    return 0;
}
