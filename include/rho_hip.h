/*
 * rho_hip.h -- C ABI of librho_hip.so: the MI355X (gfx950) kernels behind the
 * rho_diffusion DDPM / UNetv2 hot path.
 *
 * The reference (intel/rho-diffusion) has no FFI of its own: its hot path is stock
 * PyTorch ops called from Python.  Each entry point below therefore cites the reference
 * *operator* (file:line under /root/reference) whose arithmetic it replaces; the Python
 * classes in rho_diffusion_amd/ that mirror the reference's class surface call these
 * through ctypes.
 *
 * Conventions
 *  - Every function is asynchronous on the caller's hipStream_t (passed as void*),
 *    allocates nothing, never synchronises, and returns 0 on success, a negative
 *    RHO_E_* code for bad arguments, or a positive hipError_t from the launch.
 *  - Pointers are device pointers unless stated otherwise.
 *  - dtype: RHO_F32 = 0 (float), RHO_BF16 = 1 (bfloat16 storage, fp32 accumulate).
 *  - "channels-last" activations are [N, D, H, W, C] contiguous (2-D: D = 1, 1-D: D = H = 1).
 *    Tensors at the pipeline boundary (x_t, eps, eps_hat) keep the reference's
 *    [N, C, *spatial] float32 layout.
 */
#ifndef RHO_HIP_H
#define RHO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHO_F32 0
#define RHO_BF16 1

#define RHO_E_ARG (-1)      /* inconsistent or unsupported argument */
#define RHO_E_ALIGN (-2)    /* pointer / channel count not aligned as required */
#define RHO_E_SHAPE (-3)    /* tile / shape constraint violated */

/* ABI version: bumped on ANY signature / struct-layout change (2: table_len in rho_q_sample(_coef), fmt in rho_gn_bwd_finalize,
 * rho_conv_desc grew; 3: round-3 additions; 9: the rho_gd_* / metrics entry points of csrc/gaussian.hip;
 * 10: learned variances - RHO_GD_LOG_BETA, the *_lv / strided / hybrid-loss entry points; the dataset entry points added since -
 * rho_crop_resize, rho_line_profile, rho_pil_resize_taps, rho_u8_image_batch, the guidance trio rho_p_sample_step_cfg,
 * rho_cond_keep_mask, rho_cond_drop, the query rho_attention_variant, and the spaced-walk pair rho_p_sample_step_spaced,
 * rho_spaced_advance, and the prediction-type pair rho_pred_loss_ws, rho_p_sample_step_spaced_pred, and the multistep solver's rho_dpmpp_2m_step - change no existing signature or
 * struct, so by this
 * rule they leave it at 10: a binding that lacks them fails on the missing symbol).  A loader must compare rho_abi_version() with the header it was written against
 * before calling anything else (hip.py does; a build with all symbols but older signatures would be called with shifted arguments). */
#define RHO_ABI_VERSION 10
int rho_abi_version(void);
/* static string: target arch + build flags */
const char* rho_build_info(void);

/* ------------------------------------------------------------------ diffusion loops */

/* q_sample: x_t = sqrt(abar[t_b]) * x0 + sqrt(1 - abar[t_b]) * eps     (per batch element b)
 * replaces DDPM.forward_process, rho_diffusion/diffusion/ddpm.py:104-130 (+ the gather of
 * abstract_diffusion.py:171-220).  x0/eps/x_t: float32 [B, per_sample]; abar: float32 [T];
 * t: int64 [B].  nan_flag (optional, int32[1]): bit 0 is set if any x_t is NaN (the device-side form of the host check at
 * ddpm.py:268-272), bit 2 if some t[b] lies outside [0, table_len) - the reference raises IndexError there; the kernel then
 * reads the clamped row instead of out-of-bounds memory.  table_len = number of entries of alpha_bar. */
int rho_q_sample(const float* x0, const float* eps, float* x_t, const float* alpha_bar,
                 const int64_t* t, int64_t batch, int64_t per_sample, int64_t table_len, int32_t* nan_flag, void* stream);

/* p_sample_step: x <- clamp((x - beta/sqrt(1-abar) * eps_hat)/sqrt(alpha) + 0.8*sqrt(beta)*z, -1, 1)
 * replaces ddpm.py:210-218 (one reverse update, caller skips t == 0; z may be NULL => 0,
 * the t <= 1 case of ddpm.py:196-199).  coef = {1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), 0.8*sqrt(beta_t)}
 * as float32[3] on the DEVICE (row t of a [T,3] table built once per schedule) so a captured
 * HIP graph can be replayed with a different row pointer-free: the row index is read from
 * *t_dev (int32[1], device).  x updated in place; n elements. */
int rho_p_sample_step(float* x, const float* eps_hat, const float* z, const float* coef_table,
                      const int32_t* t_dev, int64_t n, void* stream);

/* p_sample_step under classifier-free guidance (Ho & Salimans 2022; adds to ddpm.py:210-218, the reference has no guided sampler:
 * its ClassifierGuidance, conditioning.py:142-155, holds no classifier).  x2 float32 [2, n]: row 0 is x_t, row 1 its copy - the
 * doubled batch the backbone reads; eps2 float32 [2, n]: row 0 the conditional, row 1 the null-condition prediction.
 * g = fma(scale, e_c - e_u, e_u), then the update of rho_p_sample_step on (row 0 of x2, g, z) with the same coef / t_dev / z rules
 * (t <= 0: nothing is written; t <= 1 or z == NULL: no noise), stored to BOTH rows of x2.  z float32 [n] or NULL.  Replaces the
 * combine pass, the update and the copy into the second half: 6n floats moved (5n without z) instead of 9n. */
int rho_p_sample_step_cfg(float* x2, const float* eps2, const float* z, const float* coef_table, const int32_t* t_dev,
                          float scale, int64_t n, void* stream);

/* Device-resident loop state of reverse_process (ddpm.py:195): *t_dev -= 1 and *offset_dev += delta,
 * so that one captured HIP graph replays every step without host involvement. Either may be NULL. */
int rho_step_advance(int32_t* t_dev, uint64_t* offset_dev, uint64_t delta, void* stream);

/* One reverse update of a few-step walk on a spaced timestep sequence tau_0 < ... < tau_{S-1} (DDIM with eta, Song et al. 2021; the
 * reference's DDPM, ddpm.py:132-229, can only walk every timestep).  rows float32 [S, 8] on the device, row k for t = tau_k with
 * ab = alpha_bar[tau_k], ab_prev = alpha_bar[tau_{k-1}] (1 for k = 0):
 *   {c_recip = sqrt(1/ab), c_recipm1 = sqrt(1/ab - 1), sqrt_ab, inv_sqrt_1mab = 1/sqrt(1 - ab) (0 where 1 - ab == 0),
 *    sqrt_abp = sqrt(ab_prev), sigma (0 where 1 - ab == 0), coef_eps = sqrt(max(1 - ab_prev - sigma^2, 0)), 0}.
 * k is read from *k_dev (int32[1], device): one captured graph serves every step; k outside [0, S) writes nothing.
 * guided == 0: x, eps_hat float32 [n], e = eps_hat.  guided != 0: both float32 [2, n] as in rho_p_sample_step_cfg,
 * e = fma(scale, e_c - e_u, e_u), the result stored to both rows of x.  z float32 [n] or NULL; noise enters iff z != NULL and the
 * row's sigma != 0, otherwise z is not read.  The arithmetic, one contraction shared by the 16-byte body, its tail and the scalar loop
 * (the 16-byte form needs 16-byte aligned x / eps_hat / z and, guided, n % 4 == 0; every other case gives the same bits):
 *   x0 = fma(c_recip, x, -(c_recipm1 * e))
 *   clip != 0:  x0 = clamp(x0, -1, 1);  ep = fma(-sqrt_ab, x0, x) * inv_sqrt_1mab        clip == 0:  ep = e
 *   x <- fma(sqrt_abp, x0, fma(coef_eps, ep, sigma * z))
 * and x <- sqrt_abp * x0, ep not formed, where the row has coef_eps == 0 and sigma == 0 (always row 0: the last step returns the
 * x0 estimate; at alpha_bar == 1 ep would be 0 * NaN). */
int rho_p_sample_step_spaced(float* x, const float* eps_hat, const float* z, const float* rows, const int32_t* k_dev, int32_t S,
                             int64_t n, int guided, float scale, int clip, void* stream);

/* Loop state of the spaced walk: k = *k_dev - 1; *k_dev = k; if k >= 0, *t_dev = taus[k] (int32 [S], device; taus[-1] is never read,
 * *t_dev keeps its last value); if offset_dev != NULL, *offset_dev += delta.  k_dev, t_dev and taus must not be NULL. */
int rho_spaced_advance(int32_t* k_dev, int32_t* t_dev, const int32_t* taus, uint64_t* offset_dev, uint64_t delta, void* stream);

/* What the backbone predicts (none of this in the reference, whose DDPM predicts the noise): with x_t = sqrt(ab) x0 + sqrt(1 - ab) eps,
 * RHO_PRED_EPSILON eps, RHO_PRED_V v = sqrt(ab) eps - sqrt(1 - ab) x0 (Salimans & Ho 2022), RHO_PRED_SAMPLE x0. */
#define RHO_PRED_EPSILON 0
#define RHO_PRED_V 1
#define RHO_PRED_SAMPLE 2

/* rho_p_sample_step_spaced for pred_type RHO_PRED_V or RHO_PRED_SAMPLE (RHO_PRED_EPSILON: RHO_E_ARG, that type stays on
 * rho_p_sample_step_spaced).  rows float32 [S, 8] on the device, row k for t = tau_k:
 *   {sqrt_ab, sqrt_1mab = sqrt(1 - ab), inv_sqrt_1mab = 1/sqrt(1 - ab) (0 where 1 - ab == 0), sqrt_abp = sqrt(ab_prev),
 *    sigma (0 where 1 - ab == 0), coef_eps = sqrt(max(1 - ab_prev - sigma^2, 0)), 0, 0}
 * Nothing is divided by sqrt(ab): a row with ab == 0 is legal.  k_dev, S, guided / scale, z, clip, the store to both rows under
 * guidance and the conditions of the 16-byte form are those of rho_p_sample_step_spaced; rho_spaced_advance serves this walk
 * unchanged.  Guidance mixes the predictions, p = fma(scale, p_c - p_u, p_u) (both conversions below are affine in p at fixed x, so
 * this equals mixing the noise estimates); guided == 0: p = pred.  One contraction shared by every form:
 *   RHO_PRED_V: x0 = fma(sqrt_ab, x, -(sqrt_1mab * p))        RHO_PRED_SAMPLE: x0 = p
 *   clip != 0:  x0 = clamp(x0, -1, 1)
 *   ep = fma(-sqrt_ab, x0, x) * inv_sqrt_1mab;   RHO_PRED_V with clip == 0:  ep = fma(sqrt_1mab, x, sqrt_ab * p)
 *   x <- fma(sqrt_abp, x0, fma(coef_eps, ep, sigma * z))
 * and x <- sqrt_abp * x0, ep not formed, where the row has coef_eps == 0 and sigma == 0 (always row 0). */
int rho_p_sample_step_spaced_pred(float* x, const float* pred, const float* z, const float* rows, const int32_t* k_dev, int32_t S,
                                  int64_t n, int guided, float scale, int clip, int pred_type, void* stream);

/* One step of DPM-Solver++(2M) (Lu et al. 2022, the data-prediction second-order multistep solver; none of this in the reference) on
 * the spaced walk, for every pred_type (RHO_PRED_EPSILON, RHO_PRED_V, RHO_PRED_SAMPLE; anything else: RHO_E_ARG).  rows float32 [S, 8]
 * on the device, row k for the step from t = tau_k to tau_{k-1} with alpha = sqrt(ab), sigma = sqrt(1 - ab), primes for ab_prev
 * (1 for k = 0), lam = log(alpha / sigma), h = lam' - lam, r = h_prev / h (h_prev: the h of row k + 1):
 *   {a_x, a_p, c_x = sigma'/sigma, c_d0 = c_0 (1 + 1/(2r)), c_d1 = -c_0 / (2r), 0, 0, 0},   c_0 = alpha' (1 - e^{-h})
 * with a_x = sqrt(1/ab), a_p = sqrt(1/ab - 1) for EPSILON, a_x = sqrt(ab), a_p = sqrt(1 - ab) for V, both unused for SAMPLE;
 * first-order rows (row S-1, row 0, a step whose h or h_prev is not finite) carry c_d1 = 0, c_d0 = c_0, and row 0 is
 * {a_x, a_p, 0, 1, 0}.  hist float32 [n] - one row, also under guidance - holds the x0 estimate of the step before; it is read only
 * where the row has c_d1 != 0 (so it may be uninitialised at the first step of a walk) and always receives this step's estimate.
 * k_dev, S, guided / scale, clip and the store to both rows of x under guidance are those of rho_p_sample_step_spaced (k outside
 * [0, S) writes nothing, neither x nor hist); guidance mixes the predictions, p = fma(scale, p_c - p_u, p_u), guided == 0: p = pred.
 * The 16-byte form needs 16-byte aligned x / pred / hist and, guided, n % 4 == 0; every other case gives the same bits.  One
 * contraction shared by every form:
 *   x0 = fma(a_x, x, -(a_p * p))        RHO_PRED_SAMPLE: x0 = p            clip != 0:  x0 = clamp(x0, -1, 1)
 *   c_d1 != 0:               x' = fma(c_x, x, fma(c_d0, x0, c_d1 * hist))
 *   c_d1 == 0:               x' = fma(c_x, x, c_d0 * x0)                   c_d1 == 0 and c_x == 0:  x' = c_d0 * x0
 *   hist <- x0 (the clamped value);   x <- x'
 * No noise is drawn: the solver is deterministic.  rho_spaced_advance serves this walk unchanged. */
int rho_dpmpp_2m_step(float* x, const float* pred, float* hist, const float* rows, const int32_t* k_dev, int32_t S, int64_t n,
                      int guided, float scale, int clip, int pred_type, void* stream);

/* Counter-based Philox4x32-10 standard normals (Box-Muller), replaces torch.randn_like at
 * ddpm.py:101-102,171,197.  out float32[n]; stream of (seed, offset) is reproducible and
 * independent of launch geometry.  offset is read from *offset_dev (uint64[1], device) when
 * offset_dev != NULL (graph-replayable), else from `offset`. */
int rho_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset,
                      const uint64_t* offset_dev, void* stream);

/* mean((a-b)^2) -> loss[0] (float32, written by this call) and optionally grad_a = 2(a-b)/n.
 * replaces nn.MSELoss at ddpm.py:280 (+ its backward).  rho_mse_ws with its scratch allocated and freed in stream order
 * (hipMallocAsync) by the call itself. */
int rho_mse(const float* a, const float* b, float* loss, float* grad_a, int64_t n, void* stream);

/* The same with an ORDERED reduction (ABI 7): block partials go to partials[n_partials] (scratch, >= 1; 1024 is plenty) and are added
 * in index order, so the loss value is bit-reproducible run to run (rho_mse used to add its blocks with an fp32 atomic, in arrival
 * order).  loss and grad_a are identical in both.  The Python binding always uses this form. */
int rho_mse_ws(const float* a, const float* b, float* loss, float* grad_a, int64_t n, float* partials, int64_t n_partials, void* stream);

/* The training loss of a backbone that predicts pred_type (RHO_PRED_*), with an optional per-timestep weight (min-SNR-gamma, Hang et
 * al. 2023); in place of nn.MSELoss at ddpm.py:280 and its backward, the target never materialised.  pred, x0, eps float32
 * [batch, per_sample]; alpha_bar float32 [table_len]; w float32 [table_len] or NULL (weight 1); t int64 [batch] on the device.  Per
 * sample b: ab = alpha_bar[t_b], sa = sqrtf(ab), sb = sqrtf(1 - ab) (as rho_q_sample forms them), wb = w[t_b].  Per element, one
 * contraction shared by the 16-byte body (pred / x0 / eps / grad 16-byte aligned, per_sample >= 4), its tail and the scalar form:
 *   target g = eps (EPSILON) | x0 (SAMPLE) | fma(sa, eps, -(sb * x0)) (V);   d = pred - g
 *   sum <- fma(wb * d, d, sum);   grad = (wb * k2) * d,  k2 = 2 * (1.0f / (float)(batch * per_sample))       grad may be NULL
 * loss[0] = sum_b wb sum_i d^2 / (batch * per_sample), reduced as rho_mse_ws reduces: block partials -> partials[n_partials]
 * (scratch, >= 1; 1024 is plenty), added in index order, no atomics, bit-reproducible run to run.  grad has the same bits in every
 * form and, for EPSILON with wb == 1, those of rho_mse_ws(pred, eps).  A t_b outside [0, table_len) sets *err_flag |= 4 (optional
 * flag, int32[1]) and reads the clamped row, as rho_q_sample does. */
int rho_pred_loss_ws(const float* pred, const float* x0, const float* eps, const float* alpha_bar, const float* w, const int64_t* t,
                     int64_t batch, int64_t per_sample, int64_t table_len, int pred_type, float* loss, float* grad, float* partials,
                     int64_t n_partials, int32_t* err_flag, void* stream);

/* mean over all non-batch axes of a float32 [batch, per_sample] tensor -> out[batch]: mean_flat of layers.py:105-110 (ABI 7). */
int rho_mean_flat(const float* x, float* out, int64_t batch, int64_t per_sample, void* stream);

/* Reproducibility switch (ABI 7).  The reference's CPU path is deterministic; here three backward kernels combine partial sums
 * with fp32 atomics by default (weight gradient, the dx of rho_linear_bwd, rho_multi_embed_bwd), so gradients differ in the last
 * bits run to run.  rho_set_deterministic(1) (or RHO_DETERMINISTIC=1 / RHO_WGRAD_DETERMINISTIC=1 in the environment) makes the
 * latter two take ordered paths and tells callers to use rho_conv_nd_wgrad_ws for the weight gradient; returns the old value. */
int rho_set_deterministic(int on);
int rho_get_deterministic(void);

/* Fused multi-tensor-free AdamW over one flat float32 parameter arena
 * (torch.optim.AdamW built at abstract_diffusion.py:103-119): decoupled weight decay,
 * bias correction from `step` (1-based).  p, g, m, v: float32[n]. */
int rho_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
              float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* The other registry optimizers (rho_diffusion/registry.py:177-193) as ONE fused update over a flat float32 arena: the single-tensor
 * paths of torch 2.10's torch/optim/{adam,adamw,sgd,rmsprop,adagrad,adamax,nadam,radam,adadelta}.py (_single_tensor_*), one launch
 * instead of a dozen ATen calls per parameter.  p, g and the state arenas s0 / s1 / s2 are float32[n]; g is only read.
 *   kind              hp[3..]                                   s0            s1            s2
 *   RHO_OPT_ADAM      beta1, beta2                              exp_avg       exp_avg_sq    max_exp_avg_sq (AMSGRAD)
 *   RHO_OPT_ADAMW     the same with decoupled weight decay
 *   RHO_OPT_SGD       momentum, dampening                       momentum_buffer (momentum != 0; step 1 seeds it with the gradient)
 *   RHO_OPT_RMSPROP   alpha, momentum                           square_avg    grad_avg (CENTERED)   momentum_buffer (momentum > 0)
 *   RHO_OPT_ADAGRAD   lr_decay                                  sum
 *   RHO_OPT_ADAMAX    beta1, beta2                              exp_avg       exp_inf
 *   RHO_OPT_NADAM     beta1, beta2, momentum_decay, mu_product  exp_avg       exp_avg_sq
 *   RHO_OPT_RADAM     beta1, beta2                              exp_avg       exp_avg_sq
 *   RHO_OPT_ADADELTA  rho                                       square_avg    acc_delta
 * hp: float32[8] on the HOST, read during the call: {lr, weight_decay, eps, then the kind's own as listed, rest ignored}.  NAdam's
 * mu_product is the running product INCLUDING this step's mu (torch keeps it as a float32 scalar per parameter; the caller owns
 * it).  step is 1-based; bias corrections, NAdam's mu / mu_next, RAdam's rho_t and rectification and Adagrad's clr are computed
 * here in double and passed to the kernel by value.  flags: RHO_OPT_* bits; a slot the kind and its options do not use may be NULL
 * and is not touched.  gscale (optional, float32[1] on the device): g is multiplied by gscale[0] as it is loaded - the clip
 * coefficient of rho_clip_coef - and the gradient arena is not rewritten.  RHO_E_ARG: NULL p / g / hp / a needed slot, n <= 0,
 * unknown kind or flag, step < 1. */
#define RHO_OPT_ADAM 0
#define RHO_OPT_ADAMW 1
#define RHO_OPT_SGD 2
#define RHO_OPT_RMSPROP 3
#define RHO_OPT_ADAGRAD 4
#define RHO_OPT_ADAMAX 5
#define RHO_OPT_NADAM 6
#define RHO_OPT_RADAM 7
#define RHO_OPT_ADADELTA 8
#define RHO_OPT_MAXIMIZE 1
#define RHO_OPT_AMSGRAD 2
#define RHO_OPT_DECOUPLED_WD 4
#define RHO_OPT_NESTEROV 8
#define RHO_OPT_CENTERED 16
int rho_optim_step(int32_t kind, uint32_t flags, float* p, const float* g, float* s0, float* s1, float* s2, int64_t n,
                   const float* hp, int32_t step, const float* gscale, void* stream);

/* Global gradient norm for clipping (torch.nn.utils.clip_grad_norm_, called at rho_diffusion/diffusion/diffusers.py:134), without
 * atomics or a host round trip.  rho_sumsq_partial writes rho_sumsq_blocks(n) per-workgroup sums of x[i]^2 to partials[0 ..) in a
 * fixed order that does not depend on x's alignment; the caller lays the partials of all its arenas side by side.  rho_clip_coef
 * (one workgroup) adds them in index order and writes out = {norm, coef = min(1, max_norm / (norm + 1e-6))} (float32[2], device). */
int rho_sumsq_blocks(int64_t n);
int rho_sumsq_partial(const float* x, int64_t n, float* partials, void* stream);
int rho_clip_coef(const float* partials, int64_t n_partials, float max_norm, float* out, void* stream);

/* ------------------------------------------------------------------ embeddings */

/* Timestep embedding of UNet.forward (unet_v2.py:699-701): the interleaved sinusoid of models/common.py:27-43 for ANY integer
 * t (no table, no range limit) followed by time_embed = Linear(dim -> edim), SiLU, Linear(edim -> edim) (unet_v2.py:521-525) and
 * the label-embedding add (:702-719), one workgroup per sample:
 *   pe[b, 2i] = sin(t_b / omega[i]), pe[b, 2i+1] = cos(t_b / omega[i])      omega: float32 [dim / 2] = wavelength^(2i / dim)
 *   h = w0 pe + b0;   emb = w2 silu(h) + b2 (+ cond[b, :])
 * t is int64[B]; when t_scalar_dev != NULL every b uses *t_scalar_dev (int32[1], device) instead (graph-replayable sampling
 * step).  pe_out [B, dim] / h_out [B, edim] (optional) keep what the backward needs.  w0 == NULL: sinusoid only into pe_out
 * (the registry layer SinusoidalPositionEmbedding, common.py:46-80).  act (ABI 7): the activation between the two linears, an
 * ACTIVATION CODE - 0 identity, 1 SiLU, 2 ReLU, 3 GELU (erf), 4 Tanh, 5 Sigmoid, 6 ELU(1) - the elementwise, parameter-free entries
 * of the reference's activation registry (registry.py:162-170, resolved at unet_v2.py:518-519).  The same codes are what the `pre_silu`
 * argument of rho_gn_apply / rho_gn_bwd_reduce / rho_gn_bwd_apply and the `act_in` / `act_out` arguments of rho_linear / rho_linear_bwd
 * take (0 / 1 keep their old meaning); the conv loaders (rho_conv_desc.pre_silu, gnb_silu) and rho_head_conv3d know 0 / 1 only - a
 * network with another activation materialises its activated conv inputs with rho_gn_apply. */
int rho_timestep_embed(const float* omega, const int64_t* t, const int32_t* t_scalar_dev, const float* w0, const float* b0,
                       const float* w2, const float* b2, const float* cond, float* pe_out, float* h_out, float* emb_out,
                       int64_t batch, int64_t dim, int64_t edim, int act, void* stream);

/* MultiEmbeddings.forward (models/conditioning.py:115-139): out[b, :] = sum over keys i of tables[i][j, :] with j the position
 * of y[b, i] in that key's value list (exact float equality, conditioning.py:132).  y float32 [B, nkeys] with row stride
 * y_stride (y_stride == 1: one label per sample, shared by all keys as in the reference's 1-D branch); space = the value lists
 * concatenated (float32), key i owning space[key_off[i] .. key_off[i+1]); tables = device array of nkeys float32 [n_i, dim]
 * pointers.  idx_out (optional int32 [B, nkeys]) keeps the categories for the backward.  A label found in no list sets
 * *err_flag |= 2 (the reference fails with a shape error there).  No host synchronisation (the reference's torch.where is one). */
int rho_multi_embed(const float* y, int64_t y_stride, const float* space, const int32_t* key_off, const float* const* tables,
                    int64_t nkeys, int64_t batch, int64_t dim, float* out, int32_t* idx_out, int32_t* err_flag, void* stream);

/* Backward of rho_multi_embed: dtables[i][idx[b, i], :] += demb[b, :] (autograd of nn.Embedding, conditioning.py:58-60). */
int rho_multi_embed_bwd(const float* demb, const int32_t* idx, float* const* dtables, int64_t nkeys, int64_t batch, int64_t dim,
                        void* stream);

/* random_timesteps (abstract_diffusion.py:163-169: randint(0, timesteps, (B,)) with replacement) on the device:
 * out int64[n] uniform on [0, high), Philox4x32-10 stream (seed, offset) as rho_philox_normal (offset read from *offset_dev
 * when given).  Removes the CPU draw + H2D copy of every training step. */
int rho_randint(int64_t* out, int64_t n, int64_t high, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream);

/* Label dropout of classifier-free guidance training (adds to DDPM.training_step, ddpm.py:231-288; the reference always feeds the
 * labels).  keep uint8 [n]: keep[b] = (u_b >= p) with one uniform per sample from the Philox4x32-10 stream (seed, offset) in
 * rho_randint's counter layout (u_b = word b & 3 of counter offset + (b >> 2), over 2^32; offset read from *offset_dev when given).
 * 0 <= p < 1; p = 0 keeps every sample. */
int rho_cond_keep_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream);

/* Applies a keep mask to what rho_multi_embed wrote: for keep[b] == 0, cond[b, :] = 0 (the null condition is the zero row: the
 * timestep embedding stands alone) and cond_idx[b, 0 .. nkeys) = -1, which rho_multi_embed_bwd skips - the tables get no gradient
 * from a dropped sample.  cond float32 [batch, dim]; cond_idx int32 [batch, nkeys] or NULL (pre-embedded conditions); rows with
 * keep[b] != 0 are not touched. */
int rho_cond_drop(float* cond, int32_t* cond_idx, const uint8_t* keep, int64_t batch, int64_t dim, int64_t nkeys, void* stream);

/* out[b, o] = bias[o] + sum_k act(x[b, k]) * w[o, k] (+ add[b, o])   all float32.
 * act_in / act_out: activation codes as in rho_timestep_embed - 0 identity, 1 SiLU, 2 ReLU, 3 GELU (erf), 4 Tanh, 5 Sigmoid,
 * 6 ELU(1); act_out applies to the whole sum, after bias and add.  bias and add may be NULL.  in_dim <= 2048 (else RHO_E_ARG).
 * replaces the nn.Linear / SiLU chains of unet_v2.py:521-525 (time_embed), :229-235
 * (emb_layers of every ResBlock, batched by concatenating their weights) and the label
 * embedding add of :702-719. */
int rho_linear(const float* x, const float* w, const float* bias, const float* add, float* out,
               int64_t batch, int64_t in_dim, int64_t out_dim, int act_in, int act_out, void* stream);

/* ------------------------------------------------------------------ layout */

/* [N, C, S] float32 (reference layout) -> channels-last [N, S, Cpad] dtype, channels >= C zeroed. */
int rho_pack_input(const float* x, void* y, int dtype, int64_t n, int64_t c, int64_t s, int64_t cpad, void* stream);

/* Stem convolution with Cin * taps <= Cpad (conv_nd(dims, in_channels = 1, mc, 3), unet_v2.py:535) as a 1x1x1 GEMM: the
 * im2col operand  out[n][pos][ci * taps + tap] = x[n][ci][pos + offset(tap)]  (zero outside the volume and for k >= Cin * taps),
 * channels-last bf16; taps are ordered (kd, kh, kw) as the rows of weight.reshape(Cout, Cin * taps). */
int rho_im2col_taps(const float* x, void* out, int dtype, int64_t n, int64_t cin, int64_t d, int64_t h, int64_t w,
                    int kd, int kh, int kw, int64_t cpad, void* stream);

/* Head convolution with Cout = 1 (zero_module(conv_nd(dims, mc, out_channels = 1, 3)), unet_v2.py:679-683) as a 1x1x1 GEMM
 * T[n][q][tap] = sum_c W[0][c][tap] * act[n][q][c] followed by  out[n][pos] = bias[0] + sum_tap T[n][pos + offset(tap)][tap]
 * (fp32 sum in tap order, out-of-volume taps skipped = zero padding).  t: channels-last bf16 [N, D, H, W, Cpad]. */
int rho_tap_gather_sum(const void* t, int dtype, int64_t n, int64_t d, int64_t h, int64_t w, int kd, int kh, int kw,
                       int64_t cpad, const float* bias, float* out, void* stream);

/* Conv weight [Cout, Cin, kd, kh, kw] float32 (PyTorch layout) -> [taps][CoutP][CinP] dtype,
 * zero padded.  Optional row permutation `row_src` (int32[CoutP], device; -1 = zero row) lets
 * the qkv projection be re-ordered (legacy vs new attention order, unet_v2.py:384,419-431); with it CoutP may be below Cout.
 * (Here, in rho_prep_conv_weight_dgrad and in rho_wgrad_finalize a tap count beyond INT32_MAX is RHO_E_ARG.) */
int rho_prep_conv_weight(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int64_t taps,
                         int64_t coutp, int64_t cinp, const int32_t* row_src, void* stream);

/* ------------------------------------------------------------------ GroupNorm (32 groups) */

/* Pass 1: per-(sample, block, channel-octet) partial sums over channels-last input that may be
 * the virtual concat of two tensors (torch.cat at unet_v2.py:729 is never materialised).
 * partials: float32 [N][nblk][C/8][16] (8 sums, 8 sums of squares).  Returns required nblk via
 * rho_gn_nblk.  replaces the statistics half of GroupNorm32.forward, layers.py:71-74. */
int rho_gn_nblk(int64_t s);
int rho_gn_partial(const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype,
                   int64_t n, int64_t s, float* partials, void* stream);

/* Pass 2: mean / rstd per (n, group) (eps 1e-5, biased variance) and the folded per-(n, channel)
 * affine used by the conv prologue:   y = a*x + b  with
 *   a = rstd*gamma*(1+scale),  b = (beta - mean*rstd*gamma)*(1+scale) + shift
 * where scale/shift ([N, C] each, row stride film_stride floats) are the FiLM halves of
 * unet_v2.py:285-289 (NULL => no FiLM: plain GroupNorm affine).  stats: float32 [N][32][2]. */
int rho_gn_finalize(const float* partials, int64_t n, int64_t c, int64_t s, int64_t nblk,
                    const float* gamma, const float* beta, const float* scale, const float* shift,
                    int64_t film_stride, float* stats, float* a, float* b, void* stream);

/* ------------------------------------------------------------------ convolution */

typedef struct rho_conv_desc {
    const void* x1;        /* channels-last input, c1 channels */
    const void* x2;        /* optional second input (virtual concat after x1), c2 channels */
    const float* pre_a;    /* optional prologue y = act(a*x+b), [N, c1+c2]; NULL = raw input */
    const float* pre_b;
    const void* w;         /* prepared weights [taps][coutp][c1+c2] */
    const float* bias;     /* [coutp] float32 */
    const void* res;       /* optional residual, channels-last [.., split], added in the epilogue */
    const float* res_add;  /* optional per-(n, co) float32 added in the epilogue (additive timestep embedding,
                              unet_v2.py:291): element (n, co) at res_add[n * res_add_stride + co] */
    void* y;               /* channels-last output for co < split: [N, Do, Ho, Wo, split] */
    void* y2;              /* channel-major output for split <= co < cout: [N, cout-split, Do*Ho*Wo] */
    int32_t dtype;         /* of x1, x2, w, res, y */
    int32_t y2_f32;        /* 1: y2 is float32 regardless of dtype */
    int32_t c1, c2;
    int32_t cout, coutp, split;
    int32_t n, d, h, w_;   /* input extents (pre-upsample) */
    int32_t kd, kh, kw;    /* 1 or 3 each; allowed: (3,3,3) (1,3,3) (1,1,3) (1,1,1) */
    int32_t sh, sw;        /* stride on H / W (1 or 2); depth stride is always 1 (unet_v2.py:153) */
    int32_t up_h, up_w;    /* nearest x2 upsample folded into the loader (unet_v2.py:122-131) */
    int32_t pre_silu;      /* apply SiLU after the affine prologue */
    int32_t res_add_stride;
    /* --- backward-data use of the same kernel (dgrad = conv of dY with flipped, transposed weights) */
    int32_t y2_cl;         /* 1: y2 is channels-last [.., cout-split] (gradient of the 2nd concat source) */
    int32_t zs_h, zs_w;    /* input is dY of a stride-2 conv, read zero-stuffed: virtual extent out_h/out_w */
    int32_t out_h, out_w;  /* forward-conv input extents (only with zs_*) */
    const void* res2;      /* optional residual for the y2 region (channels-last): in-place grad accumulation */
    /* --- GroupNorm statistics of the OUTPUT, fused into the epilogue (saves the separate read of rho_gn_partial) */
    float* stats;          /* optional: per-tile channel sums of the stored (rounded) output, float32
                              [N][tiles][2][split] with tiles = rho_conv_stats_tiles(desc): row 0 = sum, row 1 = sum of
                              squares over the tile's positions; combined in fixed order by rho_gn_finalize2 */
    /* --- sub-pixel phases of a conv behind a nearest x2 upsample (Upsample, unet_v2.py:122-134): on an upsampled axis the three
     * taps of output row 2i + a read only two source rows (a = 0: rows i-1, i with weights w0, w1 + w2; a = 1: rows i, i+1 with
     * w0 + w1, w2), so one launch per parity runs a 2-tap axis (kh / kw = 2, weights from rho_prep_conv_weight_phase) on the
     * SOURCE tensor and writes every second output row / column: 12 instead of 27 taps in 3-D.  ph_h / ph_w: 0 = axis not
     * upsampled, 1 / 2 = parity 0 / 1.  y (and res, stats) describe the full-resolution output [N, D, 2H, 2W, cout].
     * A 1-tap phased axis (kh / kw = 1, taps start at the output row) is the even parity of a stride-2 conv's data gradient, see
     * rho_prep_conv_weight_sel. */
    int32_t ph_h, ph_w;
    /* data gradient of such a phase: the input (dY of the full-resolution output) is read at parity phd - 1 of the phased axis
     * (d.h / d.w_ are the source-resolution extents, the tensor has twice as many rows / columns), 2-tap axis, taps start
     * phd - 1 rows before the output position, dense output; the four launches accumulate into dX through `res`.  With kh / kw
     * = 1 (one tap at the output row) or 2 this is also the forward of a stride-2 conv split by input parity
     * (rho_prep_conv_weight_sel). */
    int32_t phd_h, phd_w;
    /* --- GroupNorm BACKWARD reduction fused into a dgrad launch (the output is d act(a * x + b), x the forward input): with
     * gnb_x1 set, `stats` receives per tile and channel  row 0 = sum of dz,  row 1 = sum of dz * x  (dz = output * act'(a x + b),
     * the output as stored) instead of the output's own moments: what rho_gn_bwd_reduce reads two tensors to compute
     * (rho_gn_bwd_finalize with fmt = 1 takes this layout).  Replaces the reductions of GroupNorm32's autograd backward. */
    const void* gnb_x1;    /* forward input, channels-last, first gnb_c1 channels of the output's `split` */
    const void* gnb_x2;    /* second concat source (split - gnb_c1 channels) or NULL */
    int32_t gnb_c1;
    int32_t gnb_silu;      /* act = SiLU (else identity) */
    const float* gnb_a;    /* [N][split] folded affine of the forward prologue (pre_a / pre_b of the forward conv) */
    const float* gnb_b;
    /* --- k-split of launches too small to fill the chip (2-D / 1-D layers at low resolution: 1024 positions x 512 couts are 16
     * workgroups on 256 CUs).  With a workspace the launch is split over the input-channel chunks into up to 16 partial launches
     * (grid z) whose fp32 tiles land in `ws` and are added in split order, with bias / residuals / rounding, by a second kernel
     * (reproducible; the partial sums are fp32 either way).  ws = NULL: never split.  rho_conv_workspace_bytes(desc) is the size
     * the preferred split wants (0: this launch is not split); a smaller workspace lowers the split count. */
    void* ws;
    int64_t ws_bytes;
    /* --- a 1x1x1 convolution of ANOTHER input folded into this launch: out = conv(x) + sk_w * cat(sk_x1, sk_x2) + sk_bias, i.e. the
     * ResBlock's `skip_connection(x) + out_layers(h)` (unet_v2.py:245-256,293) without the launch, the tensor and the residual
     * read of the skip branch.  sk_w: prepared weights [1][coutp][sk_c1 + sk_c2] (rho_prep_conv_weight of the 1x1x1 parameter),
     * sk_bias [coutp] float32 or NULL; sk_x1 / sk_x2 channels-last at the OUTPUT resolution.  bf16 3x3x3 stride-1 launches with a
     * channels-last output only (RHO_E_ARG otherwise: the caller then launches the skip conv on its own and passes it as `res`). */
    const void* sk_x1;
    const void* sk_x2;
    const void* sk_w;
    const float* sk_bias;
    int32_t sk_c1, sk_c2;
    /* --- GroupNorm BACKWARD apply pass fused into a data-gradient launch: with gna_g set the launch writes
     *     out = conv(x) [+ res / res2]  +  cA * (g * act'(a * x0 + b)) + cQ * x0 + cP
     * per channel of its (one or two) channels-last outputs - the second operand is what rho_gn_bwd_apply computes from g = the
     * gradient of act(GroupNorm(x0)), channels-last [positions][cout] over BOTH output regions, and x0 = the forward input of that
     * norm (gnb_x1 / gnb_x2 / gnb_c1, gnb_a / gnb_b = its folded affine, gnb_silu its activation 0 / 1).  cA [N][cout],
     * cP / cQ [N][32] are rho_gn_bwd_finalize's coefficients.  Used for the ResBlock whose input reaches its output through a
     * 1x1x1 skip convolution (unet_v2.py:245-256): dX = skip^T(dY) + GroupNorm-backward(in-conv path) in ONE launch instead of a
     * data-gradient launch plus an apply pass that re-reads and re-writes dX.  Needs one-sample tiles (rho_conv_stats_tiles > 0),
     * no `stats`, a second region (if any) that is channels-last (y2_cl) and a multiple of 8 (bf16) / 4 (f32) channels wide. */
    const void* gna_g;
    const float* gna_cA;
    const float* gna_cP;
    const float* gna_cQ;
} rho_conv_desc;

/* n-D convolution, zero padding k/2, as an LDS-halo-staged implicit GEMM on MFMA.
 * replaces conv_nd (layers.py:77-88) at every call site of unet_v2.py (ResBlock convs :215,
 * :241; skip 1x1 :256; Downsample :153-162; Upsample+conv :122-134; attention qkv / proj_out
 * :323,:331 with the residual of :342; stem :535; head :679-683) with the GroupNorm affine +
 * FiLM + SiLU (:212-216, :285-289) applied while the halo tile is staged.  Wide bf16 1x1x1 launches without a prologue or a
 * second input (the attention projections) run as a plain LDS-DMA GEMM, k_gemm1x1, instead (RHO_GEMM1X1=0: never). */
int rho_conv_nd_fwd(const rho_conv_desc* desc, void* stream);

/* Weights of one sub-pixel phase (see rho_conv_desc.ph_h): from the fp32 parameter [cout][cin][kd][kh][kw] (kh / kw = 3 on a
 * phased axis) to the launch layout [kd * kh' * kw' taps][coutp][cinp] with the two taps of a phased axis summed as described
 * there; ph_h / ph_w as in the descriptor.  dgrad = 1: the data-gradient layout instead, [taps][cinp rows = ceil32(cin)][coutp
 * columns] with flipped taps and transposed channels (as rho_prep_conv_weight_dgrad), for a launch with phd_h / phd_w. */
int rho_prep_conv_weight_phase(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int kd, int kh, int kw, int ph_h,
                               int ph_w, int64_t coutp, int64_t cinp, int dgrad, void* stream);

/* Parity split of a STRIDE-2 conv (Downsample, unet_v2.py:153-162), again on stride-1 launches.  Per strided axis
 * y[o] = w0 x[2o-1] + w1 x[2o] + w2 x[2o+1]:
 *   forward  = one launch per INPUT parity, accumulated through `res` (rho_conv_desc.phd_h: even rows: 1 tap {w1}; odd rows:
 *              2 taps {w0, w2} starting one row before the output row) - the loader never stages the 2x halo of a strided tile;
 *   backward = one launch per parity of dX (rho_conv_desc.ph_h: dx[2m] = w1 dy[m]; dx[2m+1] = w2 dy[m] + w0 dy[m+1]) instead of
 *              a 27-tap conv over a zero-stuffed dY in which three of four multiply-adds are zeros.
 * This packs the taps such a launch uses: new tap r of an axis is source tap (sel >> 4r) & 15 (kh2 / kw2 new taps; an axis that
 * keeps its taps passes its size and 0x210); flip_d mirrors the depth taps (data gradient); dgrad selects the data-gradient
 * layout [taps][ceil32(cin)][ceilCK(cout)] instead of [taps][coutp][cinp]. */
int rho_prep_conv_weight_sel(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int kd, int kh, int kw, int kh2, int kw2,
                             int sel_h, int sel_w, int flip_d, int64_t coutp, int64_t cinp, int dgrad, void* stream);

/* Number of output tiles per sample the launch of `desc` uses (the middle extent of desc->stats), or 0 when fused
 * statistics are not available for this geometry (channel-major outputs, tiles that straddle samples: 1-D / 2-D
 * kernels, 1x1x1 with positions-per-sample not a multiple of 256); callers then fall back to rho_gn_partial. */
int64_t rho_conv_stats_tiles(const rho_conv_desc* desc);

/* The 1-channel ends of the 3-D UNet as single launches (bf16 inference plans; contraction over the 27 taps / taps as output rows,
 * intermediates in LDS - see csrc/ends.hip).
 *   rho_stem_conv3d: y[n, d, h, w, co] = bias[co] + sum_tap W[co][tap] x[n, 0, (d, h, w) + off(tap)]   (zero padding 1), the stem
 *     `conv_nd(3, 1, mc, 3, padding=1)` (unet_v2.py:535).  x float32 [N, 1, D, H, W]; w = the prepared 1x1x1 weights of the im2col form
 *     [coutp][32] bf16 (rho_prep_conv_weight of the parameter reshaped [cout, 27, 1, 1, 1]); y bf16 channels-last; cout 32 or 64.
 *     stats: optional fused GroupNorm statistics of the stored output, float32 [N][rho_stem_conv3d_tiles(d, h, w)][2][cout]
 *     (the layout of rho_conv_desc.stats, read by rho_gn_finalize2).
 *   rho_head_conv3d: out[n, 0, d, h, w] = bias + sum_tap sum_c W[tap][c] act(a[n, c] x[(d, h, w) + off(tap)][c] + b[n, c]), the head
 *     `GroupNorm32 -> SiLU -> conv_nd(3, mc, 1, 3, padding=1)` (unet_v2.py:679-683).  x bf16 channels-last [N, D, H, W, C], C in
 *     {32, 64, 96, 128}; pre_a / pre_b [N, C] float32 (NULL: raw input), pre_silu; w = prepared [32][C] bf16 (rows = taps, 27 used);
 *     out float32 [N, 1, D, H, W] (the reference layout). */
int64_t rho_stem_conv3d_tiles(int64_t d, int64_t h, int64_t w);
int rho_stem_conv3d(const float* x, const void* w, const float* bias, void* y, float* stats, int64_t n, int64_t d, int64_t h, int64_t w_,
                    int64_t cout, void* stream);
int rho_head_conv3d(const void* x, const float* pre_a, const float* pre_b, int pre_silu, const void* w, const float* bias, float* out,
                    int64_t n, int64_t d, int64_t h, int64_t w_, int64_t c, void* stream);

/* Batched form of rho_wgrad_finalize / rho_wgrad_finalize_phase (ABI 7): a device table of ops, op j on launch blocks
 * [blk0, blk0 + nblk) (ascending, contiguous from 0).  rho_wgrad_finalize is the same device code (csrc/weight_tables.hip: one
 * element map, one LDS walk) on ONE kind-0 op passed by value, with or without accumulation; rho_wgrad_finalize_phase adds one phase
 * per call where kind 1 sums all phases first - another floating-point order - and is a kernel of its own over the same tap map.  total = cout * cin * kd * kh * kw (elements of the parameter gradient walked,
 * in buffer-row order).  kind 0: grad[row_src ? row_src[r] : r][ci][tap] += dw[tap][r][ci] (dw rows coutp, row width cinb; a bias
 * gradient is cin = kd = kh = kw = cinb = 1 with coutp = the width of the channel-sum vector).  kind 1: all sub-pixel phases of a conv
 * behind a nearest x2 upsample (up_h / up_w say which axes are phased; the phase buffers lie phase_stride floats apart in the order
 * of rho_prep_conv_weight_phase's phases) summed into the 3-tap gradient.  kind 2: grad[ci][taps - 1 - r] += dw[r][ci] for r < cout
 * rows (cout = the tap count kd * kh * kw, `cin` channels, buffer row width cinb): the weight gradient of a one-output-channel conv
 * computed as a GEMM against the im2col of its output gradient (taps-as-rows, mirrored).  Always accumulates; no two ops of a launch may
 * share a gradient. */
typedef struct rho_wfin_op {
    const float* dw;
    float* grad;
    const int32_t* row_src;
    int64_t cout, cin, coutp, cinb, total, phase_stride;
    int32_t kind, kd, kh, kw, up_h, up_w;
    int32_t blk0, nblk;
} rho_wfin_op;
int rho_wgrad_finalize_batch(const rho_wfin_op* ops_dev, int64_t n_ops, int64_t n_blocks, void* stream);

/* Batched weight preparation (ABI 7): ONE launch writes every prepared layout a model needs after an optimizer step - what the
 * per-tensor rho_prep_conv_weight / _dgrad / _phase / _sel calls above write, the zero-padded (and, for the qkv projection,
 * row-gathered) fp32 bias vectors, and plain fp32 copies (the batched FiLM matrix of ResBlock.emb_layers, unet_v2.py:225-232) -
 * from a table of rho_prep_op in DEVICE memory.  Op j owns launch blocks [blk0, blk0 + nblk) (blk0 ascending, contiguous, op 0 at 0;
 * n_blocks = their sum).  The per-tensor calls run the same device code (csrc/weight_tables.hip: one element map, one LDS walk): each
 * fills one rho_prep_op from its arguments, checks it and passes it by value to a launch of max(1, min(ceil(total / 256), 2048))
 * blocks, so a layout has the same bits either way.  Field meanings per kind are those of the per-tensor call of the same name:
 *   RHO_PREP_FWD   out[kd*kh*kw][d1 = coutp][d2 = cinp], perm = row_src;   RHO_PREP_DGRAD  out[taps][d1 = rowsp][d2 = colsp], perm = col_src;
 *   RHO_PREP_PHASE ph_h / ph_w / dgrad, d1 x d2 as rho_prep_conv_weight_phase;   RHO_PREP_SEL kh2 / kw2 / sel_h / sel_w / flip_d / dgrad;
 *   RHO_PREP_VEC   out[d1] (a general gather): out[i] = w[perm ? perm[i] : i] for i < cout (source length cin; perm[i] < 0: zero), 0 beyond -
 *                  the padded bias vectors, plain copies, and layouts no other kind describes (the head conv's taps-as-rows form).
 * total = elements of `out`; dtype = RHO_BF16 / RHO_F32 of `out`. */
enum { RHO_PREP_FWD = 0, RHO_PREP_DGRAD = 1, RHO_PREP_PHASE = 2, RHO_PREP_SEL = 3, RHO_PREP_VEC = 4 };
typedef struct rho_prep_op {
    const float* w;
    void* out;
    const int32_t* perm;
    int64_t cout, cin, d1, d2, total;
    int32_t kind, dtype;
    int32_t kd, kh, kw, kh2, kw2, ph_h, ph_w, sel_h, sel_w, flip_d, dgrad;
    int32_t blk0, nblk;
    int32_t pad_;
} rho_prep_op;
int rho_prep_batch(const rho_prep_op* ops_dev, int64_t n_ops, int64_t n_blocks, void* stream);

/* Workspace the k-split of `desc` wants (rho_conv_desc.ws), in bytes; 0 when the launch would not be split: kernels with a depth
 * extent (kd = 3: the batch is grid z there), launches with fused output statistics or channel-major outputs, grids of more than
 * 128 workgroups, fewer than 4 input-channel chunks.  Every kd = 1 launch qualifies otherwise - INCLUDING 1x1x1 launches (also the
 * qkv / proj_out projections of a 3-D model on a small grid).  Size = splits (<= 16) x positions x coutp x 4 bytes; at most
 * 128 workgroups x 256 positions x 128 couts x 16 splits x 4 B = 268 MB.  Depends on geometry only: one allocation of the maximum
 * over a plan's descriptors serves all of them (launches on one stream are ordered); a plan keeps it for its lifetime (counted by
 * _Plan.nbytes(); 64 MB at BASELINE configs[0], 0 at configs[2] - every grid there fills the chip). */
int64_t rho_conv_workspace_bytes(const rho_conv_desc* desc);

/* Test / profiling aid: the name of the kernel instantiation rho_conv_nd_fwd would launch for `desc`
 * ("k_conv<bf16,3,3,3,BM=128,MAXP=5,NW=8,M16=1>"), written NUL-terminated into buf (cap >= 64).  Nothing is launched.
 * Lets the parity tests assert that the variants they check against the oracle cover every variant a benchmark
 * plan (BASELINE configs c3 / c5) launches.  Same return codes as rho_conv_nd_fwd.
 * Behind the name's terminating NUL (where cap leaves room) follows a second NUL-terminated string, "geo=1" where the launch runs
 * the compile-time 4 x 8 x 8 tile form of that instantiation (whole tiles of a stride-1 bf16 3x3x3 layer; RHO_CONV_GEO=0 turns it
 * off) and "geo=0" otherwise: the name itself does not change with the form. */
int rho_conv_variant(const rho_conv_desc* desc, char* buf, int cap);

/* ------------------------------------------------------------------ synthetic data */

/* Spherical-harmonic density fields of the reference's SphericalHarmonicDataset, evaluated on the device in float64 and
 * cast to float32 once (data/synthetic.py:45-124 compute_spherical_harmonic on the linspace(-2, 2, G)^3 grid of :172-174,
 * complex min-max normalisation :115-119, abs :124, float32 :303):  out[b] = float32 [G, G, G] for (l, m) = lm[b] (int32 [B, 2]
 * on the device; the field depends on |m| only).  workspace: rho_sph_harm_workspace_bytes(batch, grid) bytes.
 * minmax_in (optional, float64 [B, 4] = min.real, min.imag, max.real, max.imag on the device) replaces the complex (min, max)
 * pair of the normalisation - for m = 1, l >= 2 the reference's pair is decided by rounding noise of scipy (sph_harm.hip);
 * minmax_out (optional, same layout) receives the pair used. */
int64_t rho_sph_harm_workspace_bytes(int64_t batch, int64_t grid);
int rho_sph_harm_fields(const int32_t* lm, int64_t batch, int64_t grid, float* out, void* workspace, const double* minmax_in,
                        double* minmax_out, void* stream);

/* ------------------------------------------------------------------ image datasets */

/* Storage dtypes of rho_crop_resize's raw images besides RHO_F32 (additive: the engine dtype codes above are unchanged). */
#define RHO_U8 2
#define RHO_F64 3

/* HOST function (host arrays, no device memory, no stream): the taps of one axis of CenterCrop(crop) followed by a bilinear
 * resize to out_size - torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=antialias), what
 * torchvision's tensor Resize calls (antialias: the triangle filter of _upsample_bilinear2d_aa).  The index and weight arithmetic is
 * torch's CPU kernels' for a float32 image (float32 scale and source index), so every weight equals torch's.  The crop follows
 * torchvision: offset int(round((in - crop) / 2)) (half to even), or a zero padding of (crop - in) // 2 in front when the crop is
 * larger.  Output o reads pixels start[o] .. start[o] + k - 1 with weights weight[o * k + j]; taps on the padding are dropped (a
 * padded pixel is 0), every window lies inside [0, in_size) and start[] is non-decreasing.  start == weight == NULL: returns k
 * only; else fills start[out_size] and weight[out_size * k] and returns k.  RHO_E_ARG on bad sizes. */
int64_t rho_crop_resize_taps(int64_t in_size, int64_t crop, int64_t out_size, int antialias, int32_t* start, float* weight);

/* DeepGalaxyDataset's default per-item transform for a batch, one launch (rho_diffusion/data/deep_galaxy.py:79-89 CenterCrop(256),
 * Resize((128, 128)), 2 t - 1; :126 swapaxes(1, 3) + float32; :283-289 images / np.max(images)):
 *   v(y, x) = raw[index[b], x, y, ch] / rowmax[index[b]]    numpy's promotion: RHO_U8 / RHO_F64 divide in float64 and round to
 *             float32 once, RHO_F32 divides in float32 (IEEE division, no reciprocal)
 *   out[b, ch, oy, ox] = 2 * sum_j wx[ox * kx + j] * sum_i wy[oy * ky + i] * v(ys[oy] + i, xs[ox] + j) - 1
 * raw: [n, h, w, c] contiguous and 16-byte aligned, dtype RHO_U8 / RHO_F32 / RHO_F64, c <= 4.  After the swap the image rows y
 * run along the w axis and its columns x along the h axis.  index: int64 [batch] on the device; rowmax: float64 [n], the maximum
 * of the camera dataset each row came from.  (ys, wy, ky) = rho_crop_resize_taps(w, crop_h, out_h, aa, ...) and (xs, wx, kx) =
 * rho_crop_resize_taps(h, crop_w, out_w, aa, ...), copied to the device; crop_h / crop_w only bound the tile windows.  out: float32
 * [batch, c, out_h, out_w].  An index outside [0, n) sets *err_flag |= 4 (optional flag) and leaves that item's output unwritten;
 * tables wider than crop_h allows set *err_flag |= 8 and leave the tile unwritten. */
int rho_crop_resize(const void* raw, int dtype, int64_t n, int64_t h, int64_t w, int64_t c, const int64_t* index, int64_t batch,
                    const double* rowmax, const int32_t* ys, const float* wy, int64_t ky, const int32_t* xs, const float* wx, int64_t kx,
                    int64_t crop_h, int64_t crop_w, int64_t out_h, int64_t out_w, float* out, int32_t* err_flag, void* stream);

/* HOST function (host arrays, no device memory, no stream): the integer tap table of one axis of PIL.Image.resize(size, BILINEAR) on
 * an 8-bit image - what torchvision's Resize runs on the PIL.Image that MNIST / CIFAR10 hand it (rho_diffusion/data/wrappers.py:108-116
 * Resize((32, 32)), ToTensor(), 2 t - 1).  Restates Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) for
 * the bilinear filter (triangle, support 1.0) over the whole axis, in C double: scale = in / out, filterscale = max(scale, 1), support =
 * filterscale, ksize = ceil(support) * 2 + 1; output o has center = (o + 0.5) * scale and reads pixels start[o] .. start[o] +
 * count[o] - 1 with start = max((int)(center - support + 0.5), 0), start + count = min((int)(center + support + 0.5), in); weight j =
 * tri((j + start - center + 0.5) * (1 / filterscale)) normalised by the window's sum; coef[o * ksize + j] = (int)(0.5 + weight * 2^22)
 * (PRECISION_BITS = 32 - 8 - 2), 0 for j >= count[o].  Every window lies inside [0, in_size).  start == count == coef == NULL: returns
 * ksize only; else fills start[out_size], count[out_size], coef[out_size * ksize] and returns ksize.  RHO_E_ARG on bad sizes. */
int64_t rho_pil_resize_taps(int64_t in_size, int64_t out_size, int32_t* start, int32_t* count, int32_t* coef);

/* The default per-item transform of MNISTDataset / CIFAR10Dataset for a batch, one launch (wrappers.py:67-75, :108-116: the PIL.Image
 * that torchvision builds per item through Resize (MNIST) -> ToTensor -> 2 t - 1), as Pillow's ImagingResample orders it for 8-bit
 * images - horizontal pass first, each pass rounded to uint8:
 *   tmp[y, ox, ch] = clip8((2^21 + sum_j raw[index[b], y, xs[ox] + j, ch] * kx[ox * ksx + j]) >> 22)        j < xn[ox]
 *   u[oy, ox, ch]  = clip8((2^21 + sum_i tmp[ys[oy] + i, ox, ch] * ky[oy * ksy + i]) >> 22)                 i < yn[oy]
 *   out[b, ch, oy, ox] = lut[u[oy, ox, ch]]
 * raw: uint8 [n, h, w, c] contiguous, c <= 4.  index: int64 [batch] on the device.  (ys, yn, ky, ksy) and (xs, xn, kx, ksx) are
 * rho_pil_resize_taps(h, out_h, ...) and rho_pil_resize_taps(w, out_w, ...) copied to the device.  An axis that keeps its size passes
 * NULL tables and ks = 0 and its pass is skipped, as Pillow skips it (RHO_E_ARG if the sizes differ); with both skipped the call is
 * a gather, HWC -> CHW and the table lookup (CIFAR-10).  lut: float32 [256] on the device - (arange(256) / 255) * 2 - 1 for the
 * reference's transforms; the kernel itself does no floating-point arithmetic.  out: float32 [batch, c, out_h, out_w].
 * Limit: one item is staged in LDS, 1 KiB + 4 (2 + ksx) out_w + 4 (2 + ksy) out_h + h w c + h out_w c bytes (each term rounded up to
 * 16; the last only with an x pass) must not exceed 64 KiB, else RHO_E_SHAPE (MNIST: 5 KiB, CIFAR-10: 4 KiB).
 * An index outside [0, n) sets *err_flag |= 4 (optional flag) and leaves that item's output unwritten; a table window outside its
 * axis sets *err_flag |= 8 and nothing is written. */
int rho_u8_image_batch(const uint8_t* raw, int64_t n, int64_t h, int64_t w, int64_t c, const int64_t* index, int64_t batch,
                       const int32_t* ys, const int32_t* yn, const int32_t* ky, int64_t ksy, const int32_t* xs, const int32_t* xn,
                       const int32_t* kx, int64_t ksx, int64_t out_h, int64_t out_w, const float* lut, float* out, int32_t* err_flag,
                       void* stream);

/* ------------------------------------------------------------------ spectra */

/* SpectroscopyDataset's item path for a batch (rho_diffusion/data/spectroscopy.py:111-189: simulate_lineprofile :142-189 with the
 * inclusive range mask of :179-181, and the division by the row maximum of :130), float32 throughout:
 *   S_b[j]    = sum over the lines k of item index[b] with min(grid) <= c_k <= max(grid):  I_k * exp(-(grid[j] - c_k)^2 / (2 w^2))
 *   out[b, j] = S_b[j] / max_j S_b[j]        (rowmax != NULL)        or S_b[j]        (rowmax == NULL)
 * grid: float32 [grid_size] on the device, monotone (numpy's linspace, uploaded).  The lines of all n_items items are packed in CSR
 * form on the device: centers / intensity float32 [total] (intensity = 10 ** clip(log10 I, -10, -2), already applied, >= 0 when the
 * row is normalised), offsets int64 [n_items + 1], and inside an item the lines are sorted by centre - the kernel visits only the
 * lines within 13.25 w of a tile of grid points (beyond that the exponent is below -87 and the term below 1.7e-38 * I).
 * w = widths[b] (float32 [batch]); with line_width (optional, float32 [total]) each line has its own width, widths[] is ignored and
 * the window uses the item's largest.  index: int64 [batch] on the device.  out: float32 [batch, grid_size].  rowmax: float32
 * [batch] scratch that receives the row maxima (zeroed by the call; a second launch divides), NULL to skip the normalisation.  A
 * row without a line in range is 0 / 0 = NaN, as in the reference.  An index outside [0, n_items) sets *err_flag |= 4 (optional
 * flag) and leaves that row unwritten; offsets outside [0, total] set *err_flag |= 8. */
int rho_line_profile(const float* grid, int64_t grid_size, const float* centers, const float* intensity, const float* line_width,
                     int64_t total, const int64_t* offsets, int64_t n_items, const int64_t* index, const float* widths, int64_t batch,
                     float* out, float* rowmax, int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------ attention */

/* Flash-style self attention, fp32 online softmax (QKVAttentionLegacy / QKVAttention,
 * unet_v2.py:365-436, with the head order resolved at weight-prep time).
 * qk: channels-last [B, T, 2C] (q of head h at h*ch, k at C + h*ch); vt: channel-major
 * [B, C, T]; out: channels-last [B, T, C].  logits = (q.k) * ch^-0.5 (== scaling q and k by
 * ch^-0.25 each, :385,:420).  ch in {16, 32, 64, 128, 256}.  lse (optional, float32 [B, heads, T]) receives the
 * base-2 log-sum-exp of the scaled logits per query, which rho_attention_bwd recomputes from. */
int rho_attention_fwd(const void* qk, const void* vt, void* out, float* lse, int dtype, int64_t batch, int64_t t,
                      int64_t heads, int64_t ch, void* stream);

/* ExponentialMovingAverage.update, rho_diffusion/ema.py:41-60: shadow -= one_minus_frac * (shadow - param),
 * float32, element-wise over n values (a whole flat parameter arena or one tensor); one_minus_frac = 1 - decay *
 * (1 - exp(-step / 2000)) is computed by the caller as the reference does. */
int rho_ema_update(float* shadow, const float* param, int64_t n, float one_minus_frac, void* stream);

/* ================================================================== backward (training) */

/* Weight gradient of rho_conv_nd_fwd (autograd of conv_nd, layers.py:77-88): desc describes the FORWARD
 * conv (inputs + prologue, which is recomputed in the loader); dy is its output gradient, channels-last with
 * row width dy_width (>= cout, padding channels zero); dw is an fp32 buffer [taps][coutp][c1+c2] that the
 * call accumulates into with fp32 atomics (zero it first).  up_h/up_w unsupported: pass the materialised
 * upsampled input (rho_upsample2x).  dbias (optional, float32 [coutp], zeroed by the caller) additionally receives the
 * bias gradient = per-channel sums of dy over all positions (the dY tiles pass through the kernel anyway; this replaces
 * a separate rho_chan_sum read of dy). */
int rho_conv_nd_wgrad(const rho_conv_desc* desc, const void* dy, int64_t dy_width, float* dw, float* dbias, void* stream);

/* Deterministic form of rho_conv_nd_wgrad (ABI 7): every workgroup (or wave, where the waves of a workgroup split positions) STORES its
 * partial [taps][coutp][cin] (+ [coutp] channel sums) to a slab of its own in `ws`, and a second launch adds the slabs to dw / dbias
 * in slab order - the same values as the atomic flush up to the summation order, bit-identical run to run and across replicas.
 * ws: scratch of at least rho_conv_wgrad_workspace_bytes(desc, dy_width) bytes (170 - 340 MB per layer at BASELINE configs[2]);
 * costs one write + one read of it per launch (+2.1 % per training step there). */
int rho_conv_nd_wgrad_ws(const rho_conv_desc* desc, const void* dy, int64_t dy_width, float* dw, float* dbias, void* ws,
                         int64_t ws_bytes, void* stream);
int64_t rho_conv_wgrad_workspace_bytes(const rho_conv_desc* desc, int64_t dy_width);

/* As rho_conv_variant, for the kernel rho_conv_nd_wgrad would launch ("k_wgrad<bf16,3,3,3,MAXP=10>", "k_wgrad1<bf16>"). */
int rho_conv_wgrad_variant(const rho_conv_desc* desc, int64_t dy_width, char* buf, int cap);

/* dw buffer -> parameter-gradient layout [cout][cin][taps] float32 (undoing the qkv row gather). */
int rho_wgrad_finalize(const float* dw, float* grad, int64_t cout, int64_t cin, int64_t taps, int64_t coutp,
                       int64_t cin_buf, const int32_t* row_src, int accumulate, void* stream);

/* ... of one sub-pixel phase (rho_conv_desc.ph_h / ph_w; dw = [kd * kh' * kw' taps][coutp][cin_buf] from rho_conv_nd_wgrad on the
 * phase's forward descriptor): every original tap of the [cout][cin][kd * kh * kw] parameter gradient takes the phase tap its row /
 * column was summed into; call once per phase with accumulate = 1 (the phases add up). */
int rho_wgrad_finalize_phase(const float* dw, float* grad, int64_t cout, int64_t cin, int kd, int kh, int kw, int ph_h, int ph_w,
                             int64_t coutp, int64_t cin_buf, int accumulate, void* stream);

/* Weights for the data gradient: out[tap'][ci][co'] = w[src(co')][ci][taps-1-tap'] so that rho_conv_nd_fwd
 * applied to dY yields dX.  rows padded to rowsp, cols to colsp. */
int rho_prep_conv_weight_dgrad(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int64_t taps,
                               int64_t rowsp, int64_t colsp, const int32_t* col_src, void* stream);

/* Backward of act(GroupNorm32(x) * (1 + scale) + shift) (layers.py:71-74 + unet_v2.py:285-289), recomputed
 * from x, the saved stats and the folded affine (a, b):
 *   reduce  : per-(n, c) sums of g*act'(u) and g*act'(u)*xhat            (one pass over g and x)
 *   finalize: (fmt 0: the reduce pass's partials, nblk = rho_gn_nblk(s); fmt 1: the per-tile sums of dz and dz * x a dgrad
 *             launch wrote through rho_conv_desc.gnb_*, [N][nblk tiles][2][C] - the reduce pass is not run then)
 *             dgamma / dbeta (summed over samples, optionally accumulated), FiLM gradients dscale / dshift
 *             ([N, C] at row stride dfilm_stride), and the coefficients cA [N,C], cP / cQ [N,32] of pass 3;
 *             work_nc2 is float32 [2][N][C] scratch
 *   apply   : dx = cA*g*act'(u) + cP + cQ*x, written (or accumulated) into the one or two source gradients.  add1 (ABI 7, may be
 *             NULL): a further addend of dx1, same shape - the gradient that reaches x1 through a residual connection
 *             (unet_v2.py:293, :342), folded in here instead of a rho_add_inplace pass of its own. */
int rho_gn_bwd_reduce(const void* g, const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n,
                      int64_t s, const float* a, const float* b, const float* stats, int pre_silu, float* partials,
                      void* stream);
int rho_gn_bwd_finalize(const float* partials, int64_t n, int64_t c, int64_t s, int64_t nblk, int fmt, const float* gamma,
                        const float* beta, const float* scale, int64_t film_stride, const float* stats,
                        float* work_nc2, float* dgamma, float* dbeta, int accumulate, float* dscale, float* dshift,
                        int64_t dfilm_stride, float* cA, float* cP, float* cQ, void* stream);
int rho_gn_bwd_apply(const void* g, const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n,
                     int64_t s, const float* a, const float* b, int pre_silu, const float* cA, const float* cP,
                     const float* cQ, void* dx1, void* dx2, int acc1, int acc2, const void* add1, void* stream);

/* Dropout forms (ABI 7): nn.Dropout(p) of ResBlock.out_layers (unet_v2.py:239: normalization, activation, Dropout, conv) as a
 * counter-based mask over the activated tensor [N, S, C] - element e keeps its value, scaled by 1 / (1 - p), iff word (e & 3) of
 * Philox4x32-10(counter = *drop_offset_dev + (e >> 2), key = drop_seed) >= p * 2^32.  rho_gn_apply_drop writes dropout(act(a x + b));
 * the two backward passes multiply the incoming gradient by the same regenerated mask (nothing is stored).  drop_p in (0, 1);
 * drop_offset_dev: uint64[1] on the device (the caller advances it once per training forward, rho_step_advance).  rho_dropout_mask
 * writes the mask alone as bytes (test aid: lets the CPU oracle apply the very mask the kernels used). */
int rho_gn_apply_drop(const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n, int64_t s, const float* a,
                      const float* b, int pre_silu, void* y, float drop_p, uint64_t drop_seed, const uint64_t* drop_offset_dev,
                      void* stream);
int rho_gn_bwd_reduce_drop(const void* g, const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n, int64_t s,
                           const float* a, const float* b, const float* stats, int pre_silu, float* partials, float drop_p,
                           uint64_t drop_seed, const uint64_t* drop_offset_dev, void* stream);
int rho_gn_bwd_apply_drop(const void* g, const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n, int64_t s,
                          const float* a, const float* b, int pre_silu, const float* cA, const float* cP, const float* cQ, void* dx1,
                          void* dx2, int acc1, int acc2, const void* add1, float drop_p, uint64_t drop_seed,
                          const uint64_t* drop_offset_dev, void* stream);
int rho_dropout_mask(uint8_t* out, int64_t n, float drop_p, uint64_t drop_seed, const uint64_t* drop_offset_dev, void* stream);

/* rho_gn_finalize over one or two sources (the virtual concat), each with its own partial-sum format:
 *   fmt 0: rho_gn_partial's layout  [n][nblk][c/8][16]  (8 sums, 8 sums of squares per channel octet)
 *   fmt 1: a convolution's fused epilogue statistics  [n][nblk][2][c]  (rho_conv_desc.stats, nblk = tiles)
 * Source 2 is optional (p2 = NULL).  Channels of source 1 come first, c = c1 + c2, groups = 32. */
int rho_gn_finalize2(const float* p1, int fmt1, int64_t nblk1, int64_t c1, const float* p2, int fmt2, int64_t nblk2,
                     int64_t c2, int64_t n, int64_t s, const float* gamma, const float* beta, const float* scale,
                     const float* shift, int64_t film_stride, float* stats, float* a, float* b, void* stream);

/* Materialised prologue  y[n,pos,:] = act(a[n,:] * concat(x1,x2)[n,pos,:] + b[n,:])  (channels-last, dtype of x),
 * bit-identical to what the convolution loaders compute on the fly from the same a / b (GroupNorm32 + FiLM + SiLU,
 * layers.py:71-74, unet_v2.py:285-289).  Used in front of rho_conv_nd_wgrad so that the weight gradient reads
 * ready activations.  C = c1 + c2 a multiple of 8, c1 and c2 multiples of 8. */
int rho_gn_apply(const void* x1, int64_t c1, const void* x2, int64_t c2, int dtype, int64_t n, int64_t s,
                 const float* a, const float* b, int pre_silu, void* y, void* stream);

/* ---- GaussianDiffusionPipeline sampling path -------------------------------------------------
 * Dynamic thresholding, gaussian_diffusion.py:400-415: out[b] = torch.quantile(|x[b, :]|, q) ("linear"
 * interpolation, evaluated in float32 exactly as ATen does: rank = float(q) * float(n-1), floor / ceil order
 * statistics found EXACTLY by a radix select, then lerp).  x: float32 [batch, n] contiguous; workspace: at least
 * rho_abs_quantile_workspace_bytes(batch) bytes of device memory (contents undefined on entry).  x at any alignment: the
 * 16-byte loads need a 16-byte aligned x and n (and stride) % 4 == 0; every other case gives the same bits. */
int64_t rho_abs_quantile_workspace_bytes(int64_t batch);
int rho_abs_quantile(const float* x, int64_t batch, int64_t n, double q, void* workspace, float* out, void* stream);
/* The same over rows that start stride >= n elements apart (ABI 10: the mean half of a learned-variance output, stride = 2n). */
int rho_abs_quantile_strided(const float* x, int64_t batch, int64_t n, int64_t stride, double q, void* workspace, float* out, void* stream);

/* q_sample with explicit float32 coefficient tables: x_t = a[t_b] * x0 + b[t_b] * eps  (GaussianDiffusionPipeline.q_sample,
 * gaussian_diffusion.py:294-312, a = float(sqrt(abar)), b = float(sqrt(1-abar)) as _extract_into_tensor casts them).
 * x0 / eps / x_t: float32 [batch, per_sample]; t: int64 [batch] on the device; a t[b] outside [0, table_len) sets
 * *err_flag |= 4 (optional flag) and reads the clamped row, as rho_q_sample. */
int rho_q_sample_coef(const float* x0, const float* eps, float* x_t, const float* coef_a, const float* coef_b,
                      const int64_t* t, int64_t batch, int64_t per_sample, int64_t table_len, int32_t* err_flag, void* stream);

/* One DDIM update for an x0-predicting model, gaussian_diffusion.py:654-702 (+ :400-415, :462-466), float32:
 *   s = max(quantile[b], 1);  x0 = clamp(model_out, -s, s) / s;  eps = (c_recip * x_t - x0) / c_recipm1
 *   x_prev = x0 * sqrt_abar_prev + coef_eps * eps + sigma_masked * noise
 * c_recip = sqrt(1/abar_t), c_recipm1 = sqrt(1/abar_t - 1), coef_eps = sqrt(1 - abar_prev - sigma^2),
 * sigma_masked = (t != 0) * sigma, all float32 scalars prepared by the caller as the reference computes them.
 * noise may be NULL when sigma_masked == 0 (eta = 0); pred_xstart may be NULL. */
int rho_ddim_step(const float* x_t, const float* model_out, const float* quantile, const float* noise, float* x_prev,
                  float* pred_xstart, int64_t batch, int64_t per_sample, float c_recip, float c_recipm1,
                  float sqrt_abar_prev, float coef_eps, float sigma_masked, void* stream);

/* One reverse step of the diffusers-style DDPM scheduler the reference's DiffusersDDPMPipeline drives
 * (rho_diffusion/diffusion/diffusers.py:214; published DDPMScheduler.step; PARITY UNPINNED - third-party arithmetic):
 *   x0 = eps_mode ? (x_t - sqrt_beta_prod * model_out) / sqrt_alpha_prod : model_out;  clamp to +-clip when clip > 0;
 *   x_prev = c0 * x0 + c1 * x_t + sigma * noise        (noise may be NULL when sigma == 0; pred_xstart may be NULL)
 * float32, n elements, scalars prepared by the caller from the scheduler tables. */
int rho_ddpm_sched_step(const float* x_t, const float* model_out, const float* noise, float* x_prev, float* pred_xstart,
                        int64_t n, int eps_mode, float sqrt_beta_prod, float sqrt_alpha_prod, float clip, float c0, float c1,
                        float sigma, void* stream);

/* ---- GaussianDiffusionPipeline API beyond the fixed DDIM path (gaussian_diffusion.py:277-1009; csrc/gaussian.hip) --------
 * Per-sample t: every entry point gathers rows of ONE packed float32 table tab[RHO_GD_ROWS][table_len] (the pipeline's float64
 * tables cast to float32, as _extract_into_tensor does) at t[b] (int64 [batch] on the device).  A t[b] outside [0, table_len)
 * sets *err_flag |= 4 (optional flag) and reads the clamped row, as rho_q_sample_coef.  Tensors: contiguous float32
 * [batch, per_sample]; batch <= 65535.  mean_type: RHO_GD_START_X (x0-predicting model) or RHO_GD_EPSILON. */
#define RHO_GD_SQRT_RECIP 0      /* sqrt(1/abar) */
#define RHO_GD_SQRT_RECIPM1 1    /* sqrt(1/abar - 1) */
#define RHO_GD_COEF1 2           /* posterior_mean_coef1 */
#define RHO_GD_COEF2 3           /* posterior_mean_coef2 */
#define RHO_GD_MODEL_VAR 4       /* model variance: FIXED_LARGE append(posterior_variance[1], betas[1:]) or FIXED_SMALL posterior_variance */
#define RHO_GD_MODEL_LOGVAR 5    /* its log (FIXED_SMALL: posterior_log_variance_clipped) */
#define RHO_GD_POST_LOGVAR 6     /* posterior_log_variance_clipped */
#define RHO_GD_ABAR 7            /* alphas_cumprod */
#define RHO_GD_ABAR_PREV 8
#define RHO_GD_ABAR_NEXT 9
#define RHO_GD_SQRT_ABAR 10
#define RHO_GD_LOG_1M_ABAR 11    /* log(1 - abar) */
#define RHO_GD_1M_ABAR 12        /* 1 - abar */
#define RHO_GD_POST_VAR 13       /* posterior_variance */
#define RHO_GD_LOG_BETA 14       /* log(betas): LEARNED_RANGE's max_log (its min_log is RHO_GD_POST_LOGVAR) */
#define RHO_GD_ROWS 15
#define RHO_GD_START_X 0
#define RHO_GD_EPSILON 1
#define RHO_GD_LEARNED 0         /* var_type of the *_lv / hybrid entry points: logvar = v */
#define RHO_GD_LEARNED_RANGE 1   /* frac = (v + 1)/2, logvar = frac*max_log + (1 - frac)*min_log */

/* Table-coefficient elementwise forms, a = tab[row_a][t_b], b = tab[row_b][t_b]:
 *   op 0: out = a*x                q_mean_variance's mean (:277-292)
 *   op 1: out = a*x + b*y          q_posterior_mean_variance's mean (:314-336)
 *   op 2: out = a*x - b*y          _predict_xstart_from_eps (:445-450)
 *   op 3: out = (a*x - y) / b      _predict_eps_from_xstart (:462-466)
 * float32 in the reference's operation order, no contraction.  y is ignored by op 0. */
int rho_gd_affine(const float* x, const float* y, float* out, const int64_t* t, const float* tab, int64_t table_len, int row_a,
                  int row_b, int op, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);

/* p_mean_variance (:338-443, START_X / EPSILON, fixed variances) + condition_mean (:473-486) + p_sample (:512-556), one pass:
 *   x0 = START_X ? model_out : sqrt_recip*x_t - sqrt_recipm1*model_out;  quantile != NULL: s = max(q[b], 1), x0 = clamp(x0, -s, s)/s
 *   out = coef1*x0 + coef2*x_t  (+ model_var*grad)  (+ ((t != 0) * exp(0.5*model_logvar)) * noise)
 * grad, noise, quantile, pred_xstart may be NULL.  Without noise, out is p_mean_variance's "mean". */
int rho_gd_posterior_step(const float* x_t, const float* model_out, const int64_t* t, const float* tab, int64_t table_len,
                          int mean_type, const float* quantile, const float* grad, const float* noise, float* out,
                          float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);

/* ddim_sample (:654-702) with condition_score (:488-510) when grad != NULL, or (reverse = 1) ddim_reverse_sample (:704-740), per-sample t:
 *   x0 as rho_gd_posterior_step;  grad: eps = (sr*x - x0)/srm1 - sqrt(1 - abar)*grad, x0 = sr*x - srm1*eps
 *   eps = (sr*x - x0)/srm1
 *   forward: sigma = eta*sqrt((1 - abar_prev)/(1 - abar))*sqrt(1 - abar/abar_prev)
 *            sample = x0*sqrt(abar_prev) + sqrt(1 - abar_prev - sigma^2)*eps  (+ ((t != 0)*sigma)*noise; noise NULL = no noise term)
 *   reverse: sample = x0*sqrt(abar_next) + sqrt(1 - abar_next)*eps   (eta 0, no grad, no noise)
 * rho_ddim_step stays the batch-uniform form with host scalars. */
int rho_gd_ddim_step(const float* x_t, const float* model_out, const int64_t* t, const float* tab, int64_t table_len,
                     int mean_type, const float* quantile, const float* grad, const float* noise, float eta, int reverse,
                     float* sample, float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);

/* The same reading sample b's model output at model_out + b*model_stride (model_stride >= per_sample): the mean half of a
 * learned-variance [B, 2C, ...] output in place, model_stride = 2*per_sample (ABI 10). */
int rho_gd_ddim_step_strided(const float* x_t, const float* model_out, int64_t model_stride, const int64_t* t, const float* tab,
                             int64_t table_len, int mean_type, const float* quantile, const float* grad, const float* noise, float eta,
                             int reverse, float* sample, float* pred_xstart, int64_t batch, int64_t per_sample, int32_t* err_flag,
                             void* stream);

/* Learned variances (:368-383, ABI 10).  The mean half of sample b is read at model_out + b*mean_stride, its variance values v at
 * var_values + b*var_stride (an output [B, 2C, ...] read in place: var_values = model_out + per_sample, both strides 2*per_sample).
 *   var_type RHO_GD_LEARNED: logvar = v;  RHO_GD_LEARNED_RANGE: frac = (v + 1)/2, logvar = frac*log_beta + (1 - frac)*post_logvar
 * p_mean_variance / condition_mean / p_sample, one pass, the learned-variance instantiation of rho_gd_posterior_step's kernel: x0 as there,
 *   out = coef1*x0 + coef2*x_t  (+ exp(logvar)*grad)  (+ ((t != 0) * exp(0.5*logvar)) * noise)
 * variance = exp(logvar), log_variance = logvar [batch, per_sample].  Every output may be NULL (not all of them). */
int rho_gd_posterior_step_lv(const float* x_t, const float* model_out, int64_t mean_stride, const float* var_values, int64_t var_stride,
                             const int64_t* t, const float* tab, int64_t table_len, int mean_type, int var_type, const float* quantile,
                             const float* grad, const float* noise, float* out, float* pred_xstart, float* variance, float* log_variance,
                             int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);

/* Scratch of the per-sample reductions (rho_gd_vlb_terms(_lv), rho_gd_mse_per_sample, rho_gd_hybrid_loss), bytes. */
int64_t rho_gd_reduce_workspace_bytes(int64_t batch, int64_t per_sample);

/* _vb_terms_bpd (:826-859) and the per-timestep statistics of calc_bpd_loop (:936-1009), fused; per sample b, written at b*out_stride:
 *   vb = where(t == 0, mean(-discretized_gaussian_log_likelihood(x_start, model_mean, 0.5*model_logvar)),
 *                      mean(normal_kl(true_mean, post_logvar, model_mean, model_logvar))) / ln 2
 *   xstart_mse = mean((pred_xstart - x_start)^2),  mse = mean(((sr*x_t - pred_xstart)/srm1 - noise)^2)
 * raw_kl / raw_nll [batch] (optional): both bpd terms.  prior = 1: _prior_bpd (:936-951), vb = mean(normal_kl(sqrt_abar*x_start,
 * log(1-abar), 0, 0)) / ln 2 at t = table_len-1 (x_t, model_out, t, noise unused).  Two-stage fixed-order reduction (double partials,
 * no atomics): bit-reproducible.  xstart_mse, mse, pred_xstart, quantile may be NULL; noise only when mse is NULL. */
int rho_gd_vlb_terms(const float* x_start, const float* x_t, const float* model_out, const int64_t* t, const float* tab,
                     int64_t table_len, int mean_type, const float* quantile, const float* noise, int prior, float* vb,
                     float* xstart_mse, float* mse, int64_t out_stride, float* raw_kl, float* raw_nll, float* pred_xstart,
                     void* workspace, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);

/* rho_gd_vlb_terms (prior = 0) with the per-element model log-variance of rho_gd_posterior_step_lv (the other instantiation of one
 * kernel): the KL against post_logvar and the decoder NLL with log_scales = 0.5*logvar; same outputs and reduction (ABI 10). */
int rho_gd_vlb_terms_lv(const float* x_start, const float* x_t, const float* model_out, int64_t mean_stride, const float* var_values,
                        int64_t var_stride, const int64_t* t, const float* tab, int64_t table_len, int mean_type, int var_type,
                        const float* quantile, const float* noise, float* vb, float* xstart_mse, float* mse, int64_t out_stride,
                        float* raw_kl, float* raw_nll, float* pred_xstart, void* workspace, int64_t batch, int64_t per_sample,
                        int32_t* err_flag, void* stream);

/* training_losses (:893-930), MSE / RESCALED_MSE with a learned variance; model_out [batch, 2*per_sample] (mean half, variance half):
 *   mse[b] = mean((target - m)^2);  vb[b] = _vb_terms_bpd on the frozen m and v, clip_denoised = False (* vb_scale if rescaled)
 *   loss[b] = mse[b] + vb[b]        (mse, vb may be NULL; fixed-order two-stage reduction, bit-reproducible)
 * Backward, grad [batch, 2*per_sample]: the mean half -((g_m/n) * (2*(target - m))) with g_m = g_loss + g_mse (the VLB sees a detached
 * mean: exactly 0 there), the variance half (g_v*scale/ln2/n) * d term/d logvar * d logvar/d v with g_v = g_loss + g_vb; at t == 0
 * through the tanh CDF, zero where a 1e-12 clamp cuts the path.  g_loss / g_mse / g_vb [batch], each may be NULL (= 0).
 * Any alignment: the 16-byte form needs per_sample % 4 == 0 and 16-byte aligned x_start / x_t / target / model_out (/ grad); every
 * other case takes the scalar form (the same gradient bits; the per-sample sums in another fixed order). */
int rho_gd_hybrid_loss(const float* x_start, const float* x_t, const float* target, const float* model_out, const int64_t* t,
                       const float* tab, int64_t table_len, int mean_type, int var_type, int rescaled, float vb_scale, float* loss,
                       float* mse, float* vb, void* workspace, int64_t batch, int64_t per_sample, int32_t* err_flag, void* stream);
int rho_gd_hybrid_loss_bwd(const float* x_start, const float* x_t, const float* target, const float* model_out, const int64_t* t,
                           const float* tab, int64_t table_len, int mean_type, int var_type, int rescaled, float vb_scale,
                           const float* g_loss, const float* g_mse, const float* g_vb, float* grad, int64_t batch, int64_t per_sample,
                           int32_t* err_flag, void* stream);

/* training_losses' MSE term (:861-934): loss[b] = mean_flat((target - out)^2), fixed-order two-stage reduction; and its backward
 * grad = -((g[b] / per_sample) * (2 * (target - out))). */
int rho_gd_mse_per_sample(const float* target, const float* out, float* loss, void* workspace, int64_t batch, int64_t per_sample,
                          void* stream);
int rho_gd_mse_per_sample_bwd(const float* target, const float* out, const float* g, float* grad, int64_t batch, int64_t per_sample,
                              void* stream);

/* rho_diffusion/metrics/losses.py, float32 elementwise over [batch, per_sample].  Operand k has mode (modes >> 2k) & 3:
 * 0 full tensor, 1 per-sample [batch], 2 the scalar argument s_* (its pointer may be NULL).
 *   normal_kl (:28-53): 0.5*(-1 + lv2 - lv1 + exp(lv1 - lv2) + (m1 - m2)^2*exp(-lv2))
 *   discretized_gaussian_log_likelihood (:64-93): tanh CDF approximation, clamps at 1e-12, where-branches at x < -0.999 / x > 0.999
 *   approx_standard_normal_cdf (:56-61) */
int rho_normal_kl(const float* mean1, const float* logvar1, const float* mean2, const float* logvar2, float s_mean1, float s_logvar1,
                  float s_mean2, float s_logvar2, int modes, float* out, int64_t batch, int64_t per_sample, void* stream);
int rho_discretized_gaussian_ll(const float* x, const float* means, const float* log_scales, float s_x, float s_means, float s_log_scales,
                                int modes, float* out, int64_t batch, int64_t per_sample, void* stream);
int rho_approx_normal_cdf(const float* x, float* out, int64_t n, void* stream);

/* Channel sums of a channels-last tensor (conv bias gradients; additive-embedding gradients):
 * out_nc[n*nc_stride + c] (+)= sum_pos x[n,pos,c];  out_c[c] (+)= sum_n out_nc[n][c] (optional).
 * partials: scratch sized like rho_gn_partial's. */
int rho_chan_sum(const void* x, int dtype, int64_t n, int64_t s, int64_t c, float* partials, float* out_nc,
                 int64_t nc_stride, int acc_nc, float* out_c, int acc_c, void* stream);

/* Nearest x2 upsample (materialised only for the wgrad of Upsample.conv) and its backward (2x2 / 1x2 sum). */
int rho_upsample2x(const void* x, void* y, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int up_h,
                   int up_w, void* stream);
int rho_pool2x_sum(const void* dy, void* dx, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int up_h,
                   int up_w, int accumulate, void* stream);

/* avg_pool_nd with kernel = stride = 2 on H and / or W (layers.py:91-102; Downsample of conv_resample = False, unet_v2.py:165, and the
 * h_upd / x_upd of ResBlock(down = True), :221-224), channels-last, output extents floor(h / 2), floor(w / 2). */
int rho_avgpool2x(const void* x, void* y, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int pool_h, int pool_w,
                  void* stream);
/* its backward: dx [.., h, w, c] (+)= dy[.., h / 2, w / 2, c] / window; rows / columns dropped by the floor receive zero. */
int rho_avgpool2x_bwd(const void* dy, void* dx, int dtype, int64_t n_times_d, int64_t h, int64_t w, int64_t c, int pool_h, int pool_w,
                      int accumulate, void* stream);

/* Backward of rho_linear: dw[o,k] (+)= sum_b dout[b,o] act(x[b,k]); db[o] (+)= sum_b dout[b,o];
 * dx[b,k] (+)= act'(x[b,k]) sum_o dout[b,o] w[o,k].  dw/db/dx may each be NULL on its own (db without dw is computed too, in
 * the same batch order); acc_params adds onto dw and db, acc_dx onto dx.  act_in: an activation code 0..6 (see rho_timestep_embed).
 * dout rows are dout_stride floats apart (0 = out_dim) so a slice of the batched FiLM gradient can be passed in place. */
int rho_linear_bwd(const float* dout, int64_t dout_stride, const float* x, const float* w, float* dw, float* db,
                   float* dx, int64_t batch, int64_t in_dim, int64_t out_dim, int act_in, int acc_params, int acc_dx,
                   void* stream);

/* x *= *scale_dev over n float32 elements: the upstream scalar of loss.backward() applied to d(loss)/d(pred)
 * without a host round trip. */
int rho_scale_by_device_scalar(float* x, const float* scale_dev, int64_t n, void* stream);

/* dst += src over n elements of `dtype` (gradient accumulation where a tensor has several consumers). */
int rho_add_inplace(void* dst, const void* src, int dtype, int64_t n, void* stream);

/* Backward of rho_attention_fwd (recompute from lse).  o / dout channels-last [B,T,C]; delta_ws float32
 * [B,heads,T] scratch; outputs dqk [B,T,2C] (dq | dk) and dv [B,T,C], channels-last in `dtype`, with explicit row
 * strides in elements (0 = dense) so both can be column ranges of one [B,T,3C] buffer = the qkv projection's dY. */
int rho_attention_bwd(const void* qk, const void* vt, const void* o, const void* dout, const float* lse,
                      float* delta_ws, void* dqk, int64_t dqk_row_stride, void* dv, int64_t dv_row_stride, int dtype,
                      int64_t batch, int64_t t, int64_t heads, int64_t ch, void* stream);

/* Names of the kernels rho_attention_fwd (backward = 0) or rho_attention_bwd (backward != 0) launches for (dtype, ch), joined with
 * '+' in launch order and written NUL-terminated into buf (cap >= 96): "k_attn_bf16<64,64>",
 * "k_attn_delta<bf16>+k_attn_dq<64,64>+k_attn_dkv_fused<64,64>".  Answered on the host from the selection the launches themselves
 * use (RHO_ATTN_F32_VALU and RHO_ATTN_DKV_SPLIT included, as latched on first use); nothing is launched and no GPU is needed.
 * Returns what the launch would return for that (dtype, ch): 0, RHO_E_ARG (dtype) or RHO_E_SHAPE (head width). */
int rho_attention_variant(int dtype, int64_t ch, int backward, char* buf, int cap);

/* ------------------------------------------------------------------ legacy UNet ("UNet v1", rho_diffusion/models/unet.py:30-269)
 * The tail of AbstractUNetBlock.forward (unet.py:117-135) on channels-last [N, S, C] tensors of `dtype`:
 *     h = act(conv2(act(conv1 x))) + residual_conv(x) + time_pe[n, c];   out = act(GroupNorm(groups, C)(h)).
 * act: 0 identity, 1 SiLU, 2 ReLU, 3 GELU (erf form, the nn.GELU() default the registry resolves "GELU" to). */

/* out = act(x) + r + nc[n, c]   (r and nc optional): unet.py:121-129 after the two convolutions. */
int rho_act_add(const void* x, const void* r, const float* nc, void* out, int dtype, int64_t n, int64_t s, int64_t c, int act,
                void* stream);
/* dx = dout * act'(x): autograd of the activation in front of the add. */
int rho_act_bwd(const void* x, const void* dout, void* dx, int dtype, int64_t numel, int act, void* stream);
/* y = act(GroupNorm(groups, C, eps)(x) * gamma + beta), nn.GroupNorm semantics (biased variance) for ANY group count
 * (unet.py:109-112 builds GroupNorm(8, C); the UNetv2 kernels are specialised for GroupNorm32); stats [N, groups, 2] =
 * (mean, rstd) is written for the backward. */
int rho_groupnorm_act(const void* x, void* y, float* stats, const float* gamma, const float* beta, int dtype, int64_t n, int64_t s,
                      int64_t c, int64_t groups, float eps, int act, void* stream);
/* its backward: dx, and dgamma[c] / dbeta[c] ACCUMULATED (fp32 atomics over samples: zero them first). */
int rho_groupnorm_act_bwd(const void* x, const void* dy, const float* stats, const float* gamma, const float* beta, void* dx,
                          float* dgamma, float* dbeta, int dtype, int64_t n, int64_t s, int64_t c, int64_t groups, int act,
                          void* stream);

/* ------------------------------------------------------------------ VisionTransformer (rho_diffusion/models/vit.py:32-372)
 * Token rows [B, N, E] row-major are the engine's channels-last layout with N positions and E channels: every nn.Linear over tokens
 * runs as a 1x1x1 rho_conv_nd_fwd (+ rho_conv_nd_wgrad and the data-gradient form), the attention on rho_attention_fwd / _bwd.
 * What those do not cover is below (csrc/vit.hip); all of it is HBM-bound, float32 statistics, no atomics, fixed summation orders. */

/* nn.LayerNorm(embed_dim), eps 1e-5 (vit.py:145-146 norm_1 / norm_2, applied at :178 and :182), with the broadcast add of the time
 * embedding (vit.py:175-176) fused into the load:
 *     y[r, :] = LN(x[r, :] + add[r / rows_per_sample, :]) * gamma + beta
 * x, y: `dtype` [rows, e]; add: float32 [rows / rows_per_sample, e] or NULL (rows_per_sample is then ignored); gamma, beta float32 [e];
 * stats: float32 [rows, 2] = (mean, rstd) for the backward.  e % 32 == 0, 32 <= e <= rho_layernorm_max_dim() (2048), any rows >= 1.
 * A fixed fraction of a wave (4 .. 64 lanes) holds a row in registers; mean, then the centred sum of squares (two passes over the
 * registers, float32). */
int64_t rho_layernorm_max_dim(void);
int rho_layernorm_fwd(const void* x, const float* add, const float* gamma, const float* beta, void* y, float* stats, int dtype,
                      int64_t rows, int64_t rows_per_sample, int64_t e, void* stream);

/* Its backward (autograd of nn.LayerNorm at vit.py:178,182 and of the add at :176), from x, add and the saved stats:
 *     dx[r, :] (+)= rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma         (acc_dx: added to what dx holds - the
 *                                                                                           residual streams of vit.py:181,184)
 *     dadd[b, :]  = sum over the rows of sample b of the dx computed here (the time embedding's gradient; NULL: not wanted)
 *     dgamma (+)= sum_r dy * xhat,  dbeta (+)= sum_r dy                                    (acc_params: added, e.g. into p.grad)
 * The reductions over rows run as per-block partials in `workspace` (rho_layernorm_bwd_workspace_bytes) and a finalize pass that adds
 * them in block order: two runs give the same bits. */
int64_t rho_layernorm_bwd_workspace_bytes(int64_t rows, int64_t rows_per_sample, int64_t e, int dtype, int has_add);
int rho_layernorm_bwd(const void* dy, const void* x, const float* add, const float* stats, const float* gamma, void* dx, int acc_dx,
                      float* dadd, float* dgamma, float* dbeta, int acc_params, void* workspace, int64_t workspace_bytes, int dtype,
                      int64_t rows, int64_t rows_per_sample, int64_t e, void* stream);

/* Patch gather (the operand of PatchEmbedding.conv_shaper, a kernel = stride = p convolution, vit.py:73-78,123-129):
 *     tokens[b, n, k] = x[b, c, g0 p + i0, g1 p + i1, g2 p + i2]    x float32 [B, C, s0, s1, s2] (missing leading axes: extent 1)
 * with n = (g0 G1 + g1) G2 + g2 the "(h w d)" order of vit.py:99-107 and k = ((c p + i0) p + i1) p + i2, i.e. the column order of
 * conv_shaper.weight.reshape(E, K); columns K .. kp - 1 are zero (kp % 32 == 0, what the GEMM reads).  tokens: `dtype` [B, N, kp].
 * Also the backward of rho_unpatchify; dbias (optional, float32 [C]) then receives (acc_dbias: is added) the per-channel sums of x =
 * the bias gradient of output_conv (vit.py:282-288): up to 256 block partials per channel in dbias_ws (scratch of
 * rho_patchify_dbias_workspace_bytes(C) bytes, required with dbias) and a second launch that adds them in block order. */
int64_t rho_patchify_dbias_workspace_bytes(int64_t c);
int rho_patchify(const float* x, void* tokens, int dtype, int64_t batch, int64_t c, int dims, int64_t s0, int64_t s1, int64_t s2,
                 int64_t p, int64_t kp, float* dbias, int acc_dbias, float* dbias_ws, void* stream);

/* The inverse scatter [B, N, kp] -> float32 [B, C, s0, s1, s2] (+ bias[c], optional): the second half of output_conv, a ConvTranspose
 * with kernel = stride = p (vit.py:282-288,365-371), which is a GEMM over the token rows followed by this.  Also the backward of
 * rho_patchify (bias NULL). */
int rho_unpatchify(const void* tokens, const float* bias, float* out, int dtype, int64_t batch, int64_t c, int dims, int64_t s0, int64_t s1,
                   int64_t s2, int64_t p, int64_t kp, void* stream);

/* y = act(x + bias[c]) over `dtype` rows [rows, cols] (cols % 8 == 0) for all six activation codes (see rho_timestep_embed), and
 * dx = dy * act'(x + bias[c]): the activation between the two MLP linears (vit.py:157-164) and behind the time / position transforms
 * (vit.py:167-171,291-295).  bias (float32 [cols]) is optional; the model passes NULL, because its linears run as rho_conv_nd_fwd /
 * rho_linear launches whose epilogue has already added the bias - the argument serves a caller whose GEMM has no bias epilogue. */
int rho_bias_act(const void* x, const float* bias, void* y, int dtype, int64_t rows, int64_t cols, int act, void* stream);
int rho_bias_act_bwd(const void* x, const float* bias, const void* dy, void* dx, int dtype, int64_t rows, int64_t cols, int act,
                     void* stream);

/* x[b, :] += pos over `dtype` [batch, m] with pos float32 [m] (embedded_patches.add_(pos_embedding), vit.py:351-353; m = N * E), and
 * its gradient dpos[j] = sum_b dx[b, j] (b ascending). */
int rho_pos_add(void* x, const float* pos, int dtype, int64_t batch, int64_t m, void* stream);
int rho_pos_add_bwd(const void* dx, float* dpos, int dtype, int64_t batch, int64_t m, void* stream);

/* ---- Sample metrics (csrc/sinkhorn.hip): the Sinkhorn divergence behind WassersteinWrapper (metrics/geom.py:28-37: geomloss's
 * SamplesLoss("sinkhorn", p=1, blur=0.01) over flatten(1)) and PeakSignalNoiseRatio (abstract_diffusion.py:79).  x float32 [n, d],
 * y float32 [m, d], contiguous, uniform weights; 1 <= n, m <= rho_sinkhorn_max_samples() (128), d >= 1 (RHO_E_SHAPE otherwise).
 * Inputs, outputs and the streaming passes are float32; the cost sums, the diameter and the loop run in float64 (at blur 0.01 the
 * transport plan, hence the gradient, is decided by cost differences ~1e-7 of the costs).  No atomics: every sum runs in an order
 * fixed by the shapes, two runs give the same bits. */
int64_t rho_sinkhorn_max_samples(void);

/* The three cost matrices of metrics/geom.py:28-37 in one pass over z = [x; y]: d2(u, v) = sum_d (u_d - v_d)^2 as a direct sum of
 * squared differences (a self-cost is exactly 0), C = sqrt(max(d2, 1e-8)) for p = 1 and d2 / 2 for p = 2.  c_xy [n, m], c_xx [n, n],
 * c_yy [m, m] in float32, and - c64 not NULL - the same three back to back in float64 [n m + n n + m m] for rho_sinkhorn_loop.
 * d is cut into chunks of 512; one workgroup stages a chunk of all n + m rows in LDS once (16-byte loads when d % 4 == 0
 * and the bases are 16-byte aligned) and writes its partial sums to `workspace`; a second launch adds the chunks in index order.
 * d <= 65535 * 512. */
int64_t rho_pairwise_cost_workspace_bytes(int64_t n, int64_t m, int64_t d);
int rho_pairwise_cost(const float* x, const float* y, int64_t n, int64_t m, int64_t d, int p, float* c_xy, float* c_xx, float* c_yy,
                      double* c64, double* workspace, int64_t workspace_bytes, void* stream);

/* out[0] = || max_rows(z) - min_rows(z) ||_2, the diameter geomloss's epsilon schedule starts from (metrics/geom.py:28-37);
 * workspace: ceil(d / 1024) doubles (rho_pairwise_cost_workspace_bytes covers it).  out: float64 [1]. */
int rho_max_diameter(const float* x, const float* y, int64_t n, int64_t m, int64_t d, double* out, double* workspace,
                     int64_t workspace_bytes, void* stream);

/* The symmetric epsilon-scaling Sinkhorn loop of metrics/geom.py:28-37 in one launch of one workgroup (cost matrices in LDS while
 * they fit in 160 KiB, the rest read through L2), with softmin(eps, C, h)[i] = -eps logsumexp_j(h[j] - C[i, j] / eps) (evaluated
 * with the uniform log-weight folded in: -eps (max u + log1p(mean expm1(u - max))), u = (potential - C) / eps):
 *   start at eps_list[0] from the log-weights; for each of the n_eps entries all four potentials from the old ones, averaged with
 *   them; one last plain step at eps_list[n_eps - 1].
 * c_xy, c_xx, c_yy: the float64 matrices of rho_pairwise_cost; eps_list: device float64 [n_eps].  Writes float32 f_ba, f_aa, h_a [n]; g_ab, g_bb, h_b [m] (h_b = b_log + g_ab / eps and h_a = a_log +
 * f_aa / eps: what entered the last step); loss[0] = mean(f_ba - f_aa) + mean(g_ab - g_bb).  debias = 0 leaves f_aa = g_bb = 0.
 * wp [n, m], wq [n, n], rp, rq [n] (all four or all NULL): the weights of the last step's gradient, P = softmax_j(h_b - C_xy / eps)
 * and Q = softmax_k(h_a - C_xx / eps), divided by the cost for p = 1 (0 where the clamp of the cost holds), and their row sums. */
int rho_sinkhorn_loop(const double* c_xy, const double* c_xx, const double* c_yy, int64_t n, int64_t m, const double* eps_list,
                      int64_t n_eps, int p, int debias, float* f_ba, float* g_ab, float* f_aa, float* g_bb, float* h_b, float* h_a,
                      float* loss, float* wp, float* wq, float* rp, float* rq, void* stream);

/* The gradient of that loss w.r.t. x (metrics/geom.py:28-37 under autograd), one pass over x and y:
 *   grad_x[i, :] = (g_out[0] / n) ((rp[i] - rq[i]) x[i, :] - sum_j wp[i, j] y[j, :] + sum_k wq[i, k] x[k, :])
 * g_out: device float32 [1], the upstream gradient. */
int rho_rows_combine(const float* x, const float* y, int64_t n, int64_t m, int64_t d, const float* wp, const float* wq, const float* rp,
                     const float* rq, const float* g_out, float* grad_x, void* stream);

/* PeakSignalNoiseRatio (abstract_diffusion.py:79): out = {10 log10(range^2 / mse), mse, min(target), max(target)} from one fused
 * pass (sum of squared error, min and max as per-block partials, folded in block order).  data_range <= 0: max - min of this
 * target.  workspace: rho_psnr_workspace_bytes(). */
int64_t rho_psnr_workspace_bytes(void);
int rho_psnr(const float* pred, const float* target, int64_t n, float data_range, float* out, float* workspace, int64_t workspace_bytes,
             void* stream);

/* ---- Structural similarity (csrc/ssim.hip): torchmetrics' StructuralSimilarityIndexMeasure, the package the reference's pipelines
 * take their metrics from (abstract_diffusion.py:31,79), for float32 fields [batch, channels, *sizes] with ndim = 1, 2 or 3 spatial
 * dimensions, over the windows that lie wholly inside the field (prod(size_d - k_d + 1) per channel; torchmetrics' reflection
 * padding is cropped again before its reduction and never enters the value).  Per spatial dimension one float32 window on the device
 * (k_d taps, odd, 1 <= k_d <= rho_ssim_max_window() = 15); the n-D window is their outer product.  With s = target[b, c, 0, .., 0]
 * (after the clamp), a = p - s, b = t - s and W[.] the window sum:
 *   mu_p = s + W[a], mu_t = s + W[b], s_pp = max(W[a a] - W[a]^2, 0), s_tt likewise, s_pt = W[a b] - W[a] W[b],
 *   S = (2 mu_p mu_t + c1)(2 s_pt + c2) / ((mu_p^2 + mu_t^2 + c1)(s_pp + s_tt + c2)),  c1 = (k1 R)^2, c2 = (k2 R)^2.
 * All window sums run in float32 in a fixed order (taps ascending, one fma chain per pass, passes along W, H, D; the shift keeps the
 * second moments from cancelling); the sums of S run in float64: one partial per workgroup, folded in index order by a second launch.
 * No atomics, no read-back: two runs give the same bits and a call can be captured in a graph. */
int64_t rho_ssim_max_window(void);

/* Bytes of `workspace` for rho_ssim (abstract_diffusion.py:31,79) at this shape (it also covers rho_ssim_range); -1 where rho_ssim would refuse the shape.
 * sizes, window_sizes: host int64 [ndim]. */
int64_t rho_ssim_workspace_bytes(int64_t batch, int64_t channels, int ndim, const int64_t* sizes, const int64_t* window_sizes);

/* out_range[0] = max(max(pred) - min(pred), max(target) - min(target)) over all n values: torchmetrics' data_range = None
 * (abstract_diffusion.py:31,79), one pass with per-block partials folded in block order.  workspace: 16 KiB (4096 floats). */
int rho_ssim_range(const float* pred, const float* target, int64_t n, float* out_range, void* workspace, int64_t workspace_bytes,
                   void* stream);

/* The index above (abstract_diffusion.py:31,79).  sizes, window_sizes: host int64 [ndim]; windows: host array of ndim device pointers.
 * R = data_range_dev[0] (device float32, e.g. of rho_ssim_range) when data_range_dev is not NULL, else data_range (> 0).  clamp != 0:
 * both inputs are clamped to [lo, hi] as they are loaded (hi > lo).  Writes per_sample [batch] (the mean of S over the channels and
 * windows of a sample), out [2] = {mean, sum} of per_sample over the batch and - map not NULL - S itself, float32
 * [batch, channels, *(size_d - k_d + 1)].  workspace: rho_ssim_workspace_bytes(), 8-byte aligned.
 * RHO_E_SHAPE: a size below its window, a window above the cap or even; RHO_E_ARG: NULL or undersized arguments, ndim outside 1..3,
 * no positive range.  Nothing is written when a code is returned. */
int rho_ssim(const float* pred, const float* target, int64_t batch, int64_t channels, int ndim, const int64_t* sizes,
             const float* const* windows, const int64_t* window_sizes, float data_range, const float* data_range_dev, int clamp, float lo,
             float hi, float k1, float k2, float* per_sample, float* out, float* map, void* workspace, int64_t workspace_bytes,
             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RHO_HIP_H */
