// Fused optimizer updates over flat float32 arenas (torch.optim's single-tensor paths, one launch per arena) and the ordered
// sum-of-squares reduction behind gradient-norm clipping.  House style of the DDPM-loop kernels (elementwise.hip): grid-stride loop,
// grid capped at 2048 x 256, 16-byte body when every pointer is 16-byte aligned, scalar tail, scalar fallback otherwise.
//
// One update expression per kind serves the 16-byte body, its tail and the fallback, with contraction switched off inside it: every
// product and sum rounds on its own, so the three paths give the same bits and the error bound of tests/test_gpu_optim.py can count the
// roundings from the text below.  Step-dependent scalars (bias corrections, NAdam's mu terms, RAdam's rectification, Adagrad's clr) are
// computed by the host entry in double from the float32 hyperparameters and passed by value.
#include <math.h>

#include "common.h"

namespace {

constexpr uint32_t F_WD = 1u << 8;      // weight_decay != 0            (internal flags sit above the ABI's RHO_OPT_* bits)
constexpr uint32_t F_MOM = 1u << 9;     // SGD / RMSprop: momentum != 0
constexpr uint32_t F_FIRST = 1u << 10;  // SGD: step 1 seeds the buffer with the gradient
constexpr uint32_t F_RECT = 1u << 11;   // RAdam: rho_t > 5, the rectified branch

struct OptK {
    float lr;      // the factor in front of the update: lr, lr / bc1 (Adam, Adamax, RAdam), clr (Adagrad), NAdam's gradient factor
    float wd;      // weight_decay, or 1 - lr * weight_decay when the decay is decoupled
    float eps;
    float a, b, c, d, e;   // per kind, see opt_update
    uint32_t flags;
};

inline int grid_for(int64_t work_items, int block) {
    int64_t g = (work_items + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// self.lerp_(g, w) for w < 0.5 and self.mul_(b).addcmul_(g, g, value = w), as ATen's CPU kernels write them
__device__ __forceinline__ float lerp_f(float s, float g, float w) {
#pragma clang fp contract(off)
    return s + w * (g - s);
}
__device__ __forceinline__ float ema_sq_f(float s, float g, float b, float w) {
#pragma clang fp contract(off)
    return s * b + (w * g) * g;
}

template <int KIND>
__device__ __forceinline__ void opt_update(const OptK& k, float& p, float g, float& s0, float& s1, float& s2) {
#pragma clang fp contract(off)
    const uint32_t f = k.flags;
    if (f & RHO_OPT_MAXIMIZE) g = -g;
    const bool decoupled = (KIND == RHO_OPT_ADAMW) || (f & RHO_OPT_DECOUPLED_WD);
    if (f & F_WD) {
        if (decoupled) p = p * k.wd;          // param.mul_(1 - lr * weight_decay)
        else g = g + k.wd * p;                // grad.add(param, alpha = weight_decay)
    }
    if (KIND == RHO_OPT_ADAM || KIND == RHO_OPT_ADAMW) {
        // a = 1 - beta1, b = beta2, c = 1 - beta2, d = 1 / sqrt(bc2), lr = lr / bc1; s0 exp_avg, s1 exp_avg_sq, s2 max_exp_avg_sq
        s0 = lerp_f(s0, g, k.a);
        s1 = ema_sq_f(s1, g, k.b, k.c);
        float v = s1;
        if (f & RHO_OPT_AMSGRAD) { s2 = fmaxf(s2, s1); v = s2; }
        p = p - k.lr * (s0 / (sqrtf(v) * k.d + k.eps));
    } else if (KIND == RHO_OPT_SGD) {
        // a = momentum, b = 1 - dampening; s0 momentum_buffer
        if (f & F_MOM) {
            s0 = (f & F_FIRST) ? g : s0 * k.a + k.b * g;
            g = (f & RHO_OPT_NESTEROV) ? g + k.a * s0 : s0;
        }
        p = p - k.lr * g;
    } else if (KIND == RHO_OPT_RMSPROP) {
        // a = alpha, b = 1 - alpha, c = momentum; s0 square_avg, s1 grad_avg (centered), s2 momentum_buffer
        s0 = ema_sq_f(s0, g, k.a, k.b);
        float avg;
        if (f & RHO_OPT_CENTERED) {
            s1 = lerp_f(s1, g, k.b);
            avg = sqrtf(s0 - s1 * s1);
        } else {
            avg = sqrtf(s0);
        }
        avg = avg + k.eps;
        if (f & F_MOM) {
            s2 = s2 * k.c + g / avg;
            p = p - k.lr * s2;
        } else {
            p = p - k.lr * (g / avg);
        }
    } else if (KIND == RHO_OPT_ADAGRAD) {
        // lr = clr = lr / (1 + (step - 1) * lr_decay); s0 sum
        s0 = s0 + g * g;
        p = p - k.lr * (g / (sqrtf(s0) + k.eps));
    } else if (KIND == RHO_OPT_ADAMAX) {
        // a = 1 - beta1, b = beta2, lr = lr / bc1; s0 exp_avg, s1 exp_inf
        s0 = lerp_f(s0, g, k.a);
        s1 = fmaxf(s1 * k.b, fabsf(g) + k.eps);
        p = p - k.lr * (s0 / s1);
    } else if (KIND == RHO_OPT_NADAM) {
        // a = 1 - beta1, b = beta2, c = 1 - beta2, d = 1 / bc2, lr = lr (1 - mu) / (1 - mu_product),
        // e = lr mu_next / (1 - mu_product mu_next)
        s0 = lerp_f(s0, g, k.a);
        s1 = ema_sq_f(s1, g, k.b, k.c);
        const float denom = sqrtf(s1 * k.d) + k.eps;
        p = p - k.lr * (g / denom);
        p = p - k.e * (s0 / denom);
    } else if (KIND == RHO_OPT_RADAM) {
        // a = 1 - beta1, b = beta2, c = 1 - beta2; rectified: lr = lr sqrt(bc2) rect / bc1, else lr = lr / bc1
        s0 = lerp_f(s0, g, k.a);
        s1 = ema_sq_f(s1, g, k.b, k.c);
        if (f & F_RECT) p = p - k.lr * (s0 / (sqrtf(s1) + k.eps));
        else p = p - k.lr * s0;
    } else if (KIND == RHO_OPT_ADADELTA) {
        // a = rho, b = 1 - rho; s0 square_avg, s1 acc_delta
        s0 = ema_sq_f(s0, g, k.a, k.b);
        const float delta = sqrtf(s1 + k.eps) / sqrtf(s0 + k.eps) * g;
        s1 = ema_sq_f(s1, delta, k.a, k.b);
        p = p - k.lr * delta;
    }
}

// s0 / s1 / s2 may be null (the kind or its options do not use that slot).  SGD's first step does not read its buffer.
template <int KIND>
__global__ __launch_bounds__(256) void k_optim(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                               float* __restrict__ s1, float* __restrict__ s2, int64_t n, OptK k,
                                               const float* __restrict__ gscale) {
    const float gs = gscale ? gscale[0] : 1.0f;
    const bool has_gs = gscale != nullptr;
    const bool ld0 = s0 != nullptr && !(KIND == RHO_OPT_SGD && (k.flags & F_FIRST));
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2) & 15) == 0);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t scalar_from = 0;
    if (vec) {
        const int64_t n4 = n >> 2;
        float4* p4 = (float4*)p;
        const float4* g4 = (const float4*)g;
        float4* a4 = (float4*)s0;
        float4* b4 = (float4*)s1;
        float4* c4 = (float4*)s2;
        for (int64_t i = tid; i < n4; i += stride) {
            float4 pv = p4[i];
            float4 gv = g4[i];
            float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av, cv = av;
            if (ld0) av = a4[i];
            if (s1) bv = b4[i];
            if (s2) cv = c4[i];
            if (has_gs) { gv.x = gv.x * gs; gv.y = gv.y * gs; gv.z = gv.z * gs; gv.w = gv.w * gs; }
            opt_update<KIND>(k, pv.x, gv.x, av.x, bv.x, cv.x);
            opt_update<KIND>(k, pv.y, gv.y, av.y, bv.y, cv.y);
            opt_update<KIND>(k, pv.z, gv.z, av.z, bv.z, cv.z);
            opt_update<KIND>(k, pv.w, gv.w, av.w, bv.w, cv.w);
            p4[i] = pv;
            if (s0) a4[i] = av;
            if (s1) b4[i] = bv;
            if (s2) c4[i] = cv;
        }
        scalar_from = n4 << 2;
    }
    for (int64_t i = scalar_from + tid; i < n; i += stride) {
        float pv = p[i];
        float gv = g[i];
        float av = ld0 ? s0[i] : 0.0f;
        float bv = s1 ? s1[i] : 0.0f;
        float cv = s2 ? s2[i] : 0.0f;
        if (has_gs) gv = gv * gs;
        opt_update<KIND>(k, pv, gv, av, bv, cv);
        p[i] = pv;
        if (s0) s0[i] = av;
        if (s1) s1[i] = bv;
        if (s2) s2[i] = cv;
    }
}

template <int KIND>
void launch_optim(float* p, const float* g, float* s0, float* s1, float* s2, int64_t n, const OptK& k, const float* gscale, void* stream) {
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)s2) & 15) == 0);
    const int64_t items = vec ? (n + 3) / 4 : n;
    hipLaunchKernelGGL(k_optim<KIND>, dim3(grid_for(items, 256)), dim3(256), 0, as_stream(stream), p, g, s0, s1, s2, n, k, gscale);
}

}  // namespace

extern "C" int rho_optim_step(int32_t kind, uint32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                              const float* hp, int32_t step, const float* gscale, void* stream) {
    if (!p || !g || !hp || n <= 0 || step < 1) return RHO_E_ARG;
    if (kind < RHO_OPT_ADAM || kind > RHO_OPT_ADADELTA) return RHO_E_ARG;
    if (flags & ~(uint32_t)(RHO_OPT_MAXIMIZE | RHO_OPT_AMSGRAD | RHO_OPT_DECOUPLED_WD | RHO_OPT_NESTEROV | RHO_OPT_CENTERED))
        return RHO_E_ARG;
    const double lr = hp[0], wd = hp[1], eps = hp[2], h0 = hp[3], h1 = hp[4], h2 = hp[5], h3 = hp[6];
    const bool decoupled = kind == RHO_OPT_ADAMW || (flags & RHO_OPT_DECOUPLED_WD);
    OptK k = {};
    k.flags = flags;
    k.eps = (float)eps;
    k.lr = (float)lr;
    if (wd != 0.0) {
        k.flags |= F_WD;
        k.wd = decoupled ? (float)(1.0 - lr * wd) : (float)wd;
    }
    bool need0 = true, need1 = false, need2 = false;      // which state arenas the kind and its options use
    switch (kind) {
        case RHO_OPT_ADAM:
        case RHO_OPT_ADAMW: {
            const double bc1 = 1.0 - pow(h0, (double)step), bc2 = 1.0 - pow(h1, (double)step);
            k.a = (float)(1.0 - h0); k.b = (float)h1; k.c = (float)(1.0 - h1); k.d = (float)(1.0 / sqrt(bc2));
            k.lr = (float)(lr / bc1);
            need1 = true; need2 = (flags & RHO_OPT_AMSGRAD) != 0;
            break;
        }
        case RHO_OPT_SGD:
            k.a = (float)h0; k.b = (float)(1.0 - h1);
            need0 = h0 != 0.0;
            if (need0) k.flags |= F_MOM | (step == 1 ? F_FIRST : 0u);
            break;
        case RHO_OPT_RMSPROP:
            k.a = (float)h0; k.b = (float)(1.0 - h0); k.c = (float)h1;
            need1 = (flags & RHO_OPT_CENTERED) != 0;
            need2 = h1 > 0.0;
            if (need2) k.flags |= F_MOM;
            break;
        case RHO_OPT_ADAGRAD:
            k.lr = (float)(lr / (1.0 + (double)(step - 1) * h0));
            break;
        case RHO_OPT_ADAMAX:
            k.a = (float)(1.0 - h0); k.b = (float)h1;
            k.lr = (float)(lr / (1.0 - pow(h0, (double)step)));
            need1 = true;
            break;
        case RHO_OPT_NADAM: {
            // h2 = momentum_decay, h3 = mu_product INCLUDING this step's mu (torch keeps it as a float32 scalar: the caller owns it)
            const double mu = h0 * (1.0 - 0.5 * pow(0.96, (double)step * h2));
            const double mu_next = h0 * (1.0 - 0.5 * pow(0.96, (double)(step + 1) * h2));
            k.a = (float)(1.0 - h0); k.b = (float)h1; k.c = (float)(1.0 - h1); k.d = (float)(1.0 / (1.0 - pow(h1, (double)step)));
            k.lr = (float)(lr * (1.0 - mu) / (1.0 - h3));
            k.e = (float)(lr * mu_next / (1.0 - h3 * mu_next));
            need1 = true;
            break;
        }
        case RHO_OPT_RADAM: {
            const double b2t = pow(h1, (double)step), bc1 = 1.0 - pow(h0, (double)step), bc2 = 1.0 - b2t;
            const double rho_inf = 2.0 / (1.0 - h1) - 1.0, rho_t = rho_inf - 2.0 * (double)step * b2t / bc2;
            k.a = (float)(1.0 - h0); k.b = (float)h1; k.c = (float)(1.0 - h1);
            if (rho_t > 5.0) {
                const double rect = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
                k.flags |= F_RECT;
                k.lr = (float)(lr * sqrt(bc2) * rect / bc1);
            } else {
                k.lr = (float)(lr / bc1);
            }
            need1 = true;
            break;
        }
        case RHO_OPT_ADADELTA:
            k.a = (float)h0; k.b = (float)(1.0 - h0);
            need1 = true;
            break;
    }
    if ((need0 && !s0) || (need1 && !s1) || (need2 && !s2)) return RHO_E_ARG;
    if (!need0) s0 = nullptr;
    if (!need1) s1 = nullptr;
    if (!need2) s2 = nullptr;
    switch (kind) {
        case RHO_OPT_ADAM: launch_optim<RHO_OPT_ADAM>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_ADAMW: launch_optim<RHO_OPT_ADAMW>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_SGD: launch_optim<RHO_OPT_SGD>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_RMSPROP: launch_optim<RHO_OPT_RMSPROP>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_ADAGRAD: launch_optim<RHO_OPT_ADAGRAD>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_ADAMAX: launch_optim<RHO_OPT_ADAMAX>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_NADAM: launch_optim<RHO_OPT_NADAM>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        case RHO_OPT_RADAM: launch_optim<RHO_OPT_RADAM>(p, g, s0, s1, s2, n, k, gscale, stream); break;
        default: launch_optim<RHO_OPT_ADADELTA>(p, g, s0, s1, s2, n, k, gscale, stream); break;
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------- gradient norm
// Quad q = elements 4q .. 4q + 3 belongs to thread q % (blocks * 256), whatever the pointer's alignment (a 16-byte load when aligned,
// four bounded 4-byte loads otherwise): the partials, and so the norm, do not depend on where the arena sits.  Each thread keeps four
// running sums (one per lane of the quad), adds them pairwise, then a wave butterfly and the four waves in two levels.
extern "C" int rho_sumsq_blocks(int64_t n) {
    if (n <= 0) return RHO_E_ARG;
    return grid_for((n + 3) / 4, 256);
}

__global__ __launch_bounds__(256) void k_sumsq_partial(const float* __restrict__ x, int64_t n, float* __restrict__ partials) {
    const bool vec = (((uintptr_t)x) & 15) == 0;
    const int64_t nq = (n + 3) >> 2, full = n >> 2;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        float4 v;
        if (vec && q < full) {
            v = ((const float4*)x)[q];
        } else {
            const int64_t e = q << 2;
            v.x = x[e];
            v.y = e + 1 < n ? x[e + 1] : 0.0f;
            v.z = e + 2 < n ? x[e + 2] : 0.0f;
            v.w = e + 3 < n ? x[e + 3] : 0.0f;
        }
        a0 = __fmaf_rn(v.x, v.x, a0);
        a1 = __fmaf_rn(v.y, v.y, a1);
        a2 = __fmaf_rn(v.z, v.z, a2);
        a3 = __fmaf_rn(v.w, v.w, a3);
    }
    __shared__ float red[4];
    const float acc = wave_sum((a0 + a1) + (a2 + a3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

extern "C" int rho_sumsq_partial(const float* x, int64_t n, float* partials, void* stream) {
    if (!x || !partials || n <= 0) return RHO_E_ARG;
    hipLaunchKernelGGL(k_sumsq_partial, dim3(rho_sumsq_blocks(n)), dim3(256), 0, as_stream(stream), x, n, partials);
    RHO_LAUNCH_CHECK();
    return 0;
}

// One workgroup: thread t adds partials t, t + 256, ... in index order, then the same butterfly.  out = {norm, coef}.
__global__ __launch_bounds__(256) void k_clip_coef(const float* __restrict__ partials, int64_t n_partials, float max_norm,
                                                   float* __restrict__ out) {
    float acc = 0.0f;
    for (int64_t i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    __shared__ float red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
        out[0] = norm;
        out[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
    }
}

extern "C" int rho_clip_coef(const float* partials, int64_t n_partials, float max_norm, float* out, void* stream) {
    if (!partials || !out || n_partials <= 0 || !(max_norm >= 0.0f)) return RHO_E_ARG;
    hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(256), 0, as_stream(stream), partials, n_partials, max_norm, out);
    RHO_LAUNCH_CHECK();
    return 0;
}
