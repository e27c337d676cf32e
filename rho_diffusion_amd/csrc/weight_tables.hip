// The two launch families every conv weight passes through: preparation (fp32 parameter -> the layouts the kernels read) and
// weight-gradient finalize (fp32 accumulation buffer -> parameter gradient).  Each has ONE element map (prep_elem / wfin_elem) and
// ONE block body (prep_block / wfin_block: an LDS transpose walk where both sides can be coalesced, else the element walk) under two
// launch forms: the batched kernel finds its op in a device table by bisection, the per-tensor entry points pass one op by value.
#include "common.h"

// Sub-pixel phases of a 3-tap axis behind a nearest x2 upsample (ph = 0: the axis is not phased and keeps its taps): phase tap r
// sums the source taps that land on the same source row -  ph = 1: {0}, {1, 2};  ph = 2: {0, 1}, {2}.
__device__ __forceinline__ void phase_src_taps(int ph, int r, int& lo, int& hi) {       // phase tap -> source tap range
    lo = hi = r;
    if (ph == 1) { lo = r ? 1 : 0; hi = r ? 2 : 0; }
    else if (ph) { lo = r ? 2 : 0; hi = r ? 2 : 1; }
}
__device__ __forceinline__ int phase_tap_of(int ph, int k) {                            // source tap -> the phase tap it went into
    return ph == 0 ? k : ph == 1 ? (k == 0 ? 0 : 1) : (k == 2 ? 1 : 0);
}

static inline int n_blocks_for(int64_t total, int64_t per_block, int64_t cap) {
    const int64_t g = (total + per_block - 1) / per_block;
    return (int)(g > cap ? cap : g < 1 ? 1 : g);
}
static inline bool bad_phase(int ph_h, int ph_w, int kh, int kw) {
    return ph_h < 0 || ph_h > 2 || ph_w < 0 || ph_w > 2 || (!ph_h && !ph_w) || (ph_h && kh != 3) || (ph_w && kw != 3);
}
// a tap count as the int32 extent the op records hold (0, which every check rejects, when it does not fit)
static inline int32_t taps32(int64_t taps) { return taps > 0x7FFFFFFF ? 0 : (int32_t)taps; }

// ================================================================================================ weight preparation
__device__ __forceinline__ float phase_weight(const float* __restrict__ w, int64_t co, int64_t ci, int64_t cin, int tap2, int kd, int kh,
                                              int kw, int ph_h, int ph_w) {
    const int kh2 = ph_h ? 2 : kh, kw2 = ph_w ? 2 : kw;
    const int c2 = tap2 % kw2, r2 = (tap2 / kw2) % kh2, dz = tap2 / (kw2 * kh2);
    int rlo, rhi, clo, chi;
    phase_src_taps(ph_h, r2, rlo, rhi);
    phase_src_taps(ph_w, c2, clo, chi);
    const float* base = w + (co * cin + ci) * ((int64_t)kd * kh * kw) + (int64_t)dz * kh * kw;
    float v = 0.0f;
    for (int r = rlo; r <= rhi; ++r)
        for (int c = clo; c <= chi; ++c) v += base[r * kw + c];
    return v;
}

// Element i of the op's output [taps'][d1][d2] (RHO_PREP_VEC: [d1]); field meanings per kind: rho_prep_op, include/rho_hip.h
__device__ __forceinline__ float prep_elem(const rho_prep_op& o, int64_t i, int kind) {
    const int64_t taps = (int64_t)o.kd * o.kh * o.kw;
    switch (kind) {
    case RHO_PREP_FWD: {                       // [taps][coutp = d1][cinp = d2]
        const int64_t ci = i % o.d2, co = (i / o.d2) % o.d1, tap = i / (o.d2 * o.d1);
        const int64_t src = o.perm ? (int64_t)o.perm[co] : (co < o.cout ? co : -1);
        return (src >= 0 && src < o.cout && ci < o.cin) ? o.w[(src * o.cin + ci) * taps + tap] : 0.0f;
    }
    case RHO_PREP_DGRAD: {                     // [taps'][rowsp = d1][colsp = d2], flipped taps, transposed channels
        const int64_t col = i % o.d2, row = (i / o.d2) % o.d1, tap = i / (o.d2 * o.d1);
        const int64_t src = o.perm ? (col < o.cout ? (int64_t)o.perm[col] : -1) : (col < o.cout ? col : -1);
        return (src >= 0 && src < o.cout && row < o.cin) ? o.w[(src * o.cin + row) * taps + (taps - 1 - tap)] : 0.0f;
    }
    case RHO_PREP_PHASE: {                     // dgrad = 0: [tap2][coutp][cinp];  1: [tap'][ceil32(cin)][colsp], flipped, transposed
        const int64_t taps2 = (int64_t)o.kd * (o.ph_h ? 2 : o.kh) * (o.ph_w ? 2 : o.kw);
        const int64_t i2 = i % o.d2, i1 = (i / o.d2) % o.d1;
        const int tap = (int)(i / (o.d2 * o.d1));
        if (!o.dgrad) return (i1 < o.cout && i2 < o.cin) ? phase_weight(o.w, i1, i2, o.cin, tap, o.kd, o.kh, o.kw, o.ph_h, o.ph_w) : 0.0f;
        return (i2 < o.cout && i1 < o.cin) ? phase_weight(o.w, i2, i1, o.cin, (int)(taps2 - 1 - tap), o.kd, o.kh, o.kw, o.ph_h, o.ph_w) : 0.0f;
    }
    case RHO_PREP_SEL: {                       // new tap r of an axis = source tap (sel >> 4r) & 15; flip_d mirrors the depth taps
        const int64_t i2 = i % o.d2, i1 = (i / o.d2) % o.d1;
        const int tap = (int)(i / (o.d2 * o.d1));
        const int c2 = tap % o.kw2, r2 = (tap / o.kw2) % o.kh2, dz = tap / (o.kw2 * o.kh2);
        const int ks = ((o.flip_d ? o.kd - 1 - dz : dz) * o.kh + ((o.sel_h >> (4 * r2)) & 15)) * o.kw + ((o.sel_w >> (4 * c2)) & 15);
        const int64_t co = o.dgrad ? i2 : i1, ci = o.dgrad ? i1 : i2;
        return (co < o.cout && ci < o.cin) ? o.w[(co * o.cin + ci) * taps + ks] : 0.0f;
    }
    default: {                                 // RHO_PREP_VEC: out[i] = w[perm ? perm[i] : i] for i < cout (perm < 0: zero), zero up to d1
        const int64_t src = (o.perm && i < o.cout) ? (int64_t)o.perm[i] : i;
        return (i < o.cout && src >= 0 && src < o.cin) ? o.w[src] : 0.0f;
    }
    }
}

// Block `block` of the `nblk` that share the op.  KIND: the op's kind when the caller knows it at compile time (-1: read it).
// `tile`: PREP_TILE floats of LDS, declared by the calling kernel (declared in here, k_wgrad_finalize_batch lost an unrolled loop)
constexpr int PREP_TILE = 64 * 33;
template <int KIND>
__device__ __forceinline__ void prep_block(const rho_prep_op& o, int block, int nblk, float* tile) {
    const int kind = KIND < 0 ? o.kind : KIND;
    const int taps_ = o.kd * o.kh * o.kw;
    if ((kind == RHO_PREP_FWD || kind == RHO_PREP_DGRAD) && taps_ > 1 && taps_ <= 32) {
        // [row][channel][tap] -> [tap][..][..] through LDS (the elementwise walk reads the parameter with a stride of `taps` floats
        // between consecutive threads: 0.5 TB/s).  A unit = 64 consecutive entries of the output's contiguous axis for one entry of
        // its middle axis: FWD (co, 64 ci): one contiguous read of 64 * taps floats;  DGRAD (ci, 64 co): 64 runs of `taps` floats.
        // Either way every tap is written as one run of 64 contiguous outputs.
        const bool fwd = kind == RHO_PREP_FWD;
        const int64_t mid = o.d1, inner = o.d2;                   // out [taps][d1][d2]
        const int64_t groups = (inner + 63) / 64;
        const int64_t units = mid * groups;
        for (int64_t u = block; u < units; u += nblk) {
            const int64_t m_ = u / groups;
            const int64_t i0 = (u % groups) * 64;
            for (int e = threadIdx.x; e < 64 * taps_; e += 256) {
                float v = 0.0f;
                if (fwd) {
                    // m_ = output row co (maybe permuted / padded), inner = ci: source run w[src][i0 .. i0 + 63][taps]
                    const int64_t src = o.perm ? (int64_t)o.perm[m_] : (m_ < o.cout ? m_ : -1);
                    const int64_t ci = i0 + e / taps_;
                    if (src >= 0 && src < o.cout && ci < o.cin) v = o.w[(src * o.cin + i0) * taps_ + e];
                    tile[(e / taps_) * 33 + e % taps_] = v;
                } else {
                    // m_ = row = input channel ci, inner = col = output channel (maybe permuted): run w[src(col)][m_][taps]
                    const int c = e / taps_, t = e % taps_;
                    const int64_t col = i0 + c;
                    const int64_t src = col < o.cout ? (o.perm ? (int64_t)o.perm[col] : col) : -1;
                    if (src >= 0 && src < o.cout && m_ < o.cin) v = o.w[(src * o.cin + m_) * taps_ + t];
                    tile[c * 33 + t] = v;
                }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < 64 * taps_; e += 256) {
                const int t = e >> 6, c = e & 63;
                if (i0 + c < inner) {
                    const float v = tile[c * 33 + (fwd ? t : taps_ - 1 - t)];
                    const int64_t oi = ((int64_t)t * mid + m_) * inner + i0 + c;
                    if (o.dtype == RHO_BF16) reinterpret_cast<bf16_raw*>(o.out)[oi] = f32_to_bf16(v);
                    else reinterpret_cast<float*>(o.out)[oi] = v;
                }
            }
            __syncthreads();
        }
        return;
    }
    const int64_t stride = (int64_t)nblk * 256;
    for (int64_t i = (int64_t)block * 256 + threadIdx.x; i < o.total; i += stride) {
        const float v = prep_elem(o, i, kind);
        if (o.dtype == RHO_BF16) reinterpret_cast<bf16_raw*>(o.out)[i] = f32_to_bf16(v);
        else reinterpret_cast<float*>(o.out)[i] = v;
    }
}

// rho_prep_batch: every prepared layout of every convolution of a model, the padded fp32 biases and the batched FiLM matrix in ONE
// launch after an optimizer step (one launch per layout cost ~170 launches of a few microseconds per training step at BASELINE
// configs[2], 2.7 ms, and as many again on the launch-bound 2-D configurations).  A block finds its op by bisection on blk0.
__global__ __launch_bounds__(256) void k_prep_batch(const rho_prep_op* __restrict__ ops, int nops) {
    __shared__ float tile[PREP_TILE];
    int lo = 0, hi = nops - 1;
    const int b = (int)blockIdx.x;
    while (lo < hi) {                          // last op whose first block is <= b
        const int mid = (lo + hi + 1) >> 1;
        if (ops[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const rho_prep_op o = ops[lo];
    prep_block<-1>(o, b - o.blk0, o.nblk, tile);
}

extern "C" int rho_prep_batch(const rho_prep_op* ops_dev, int64_t n_ops, int64_t n_blocks, void* stream) {
    if (!ops_dev || n_ops <= 0 || n_blocks <= 0 || n_blocks > 0x7FFFFFFF || n_ops > 0x7FFFFFFF) return RHO_E_ARG;
    hipLaunchKernelGGL(k_prep_batch, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream), ops_dev, (int)n_ops);
    RHO_LAUNCH_CHECK();
    return 0;
}

// The per-tensor entry points: one op, passed by value, on one block per 256 output elements.  One instance per kind: with the
// kind read at run time a 512 -> 1536 1x1 layout took 0.7 us longer than the kernel this replaces
template <int KIND>
__global__ __launch_bounds__(256) void k_prep_one(rho_prep_op o) {
    __shared__ float tile[KIND <= RHO_PREP_DGRAD ? PREP_TILE : 1];          // (only these two kinds have the LDS walk)
    prep_block<KIND>(o, (int)blockIdx.x, (int)gridDim.x, tile);
}

// The argument checks of the four entry points (d1 / d2 already hold the padded extents in the kind's order), then the launch
static int prep_one(rho_prep_op o, void* stream) {
    const bool transposed = o.kind == RHO_PREP_DGRAD || o.dgrad;                   // [d1][d2] = [cin][cout] instead of [cout][cin]
    const int64_t real1 = transposed ? o.cin : o.cout, real2 = transposed ? o.cout : o.cin;
    if (!o.w || !o.out || o.cout <= 0 || o.cin <= 0 || o.kd <= 0 || o.kh <= 0 || o.kw <= 0 || o.d2 < real2) return RHO_E_ARG;
    if (o.d1 < real1 && !(o.kind == RHO_PREP_FWD && o.perm)) return RHO_E_ARG;    // (a row table may gather fewer rows than the parameter has)
    if (o.dtype != RHO_BF16 && o.dtype != RHO_F32) return RHO_E_ARG;
    int64_t taps2 = (int64_t)o.kd * o.kh * o.kw;
    if (o.kind == RHO_PREP_PHASE) {
        if (bad_phase(o.ph_h, o.ph_w, o.kh, o.kw)) return RHO_E_ARG;
        taps2 = (int64_t)o.kd * (o.ph_h ? 2 : o.kh) * (o.ph_w ? 2 : o.kw);
    } else if (o.kind == RHO_PREP_SEL) {
        if (o.kh2 <= 0 || o.kw2 <= 0 || o.kh2 > 4 || o.kw2 > 4) return RHO_E_ARG;
        for (int r = 0; r < o.kh2; ++r) if (((o.sel_h >> (4 * r)) & 15) >= o.kh) return RHO_E_ARG;
        for (int c = 0; c < o.kw2; ++c) if (((o.sel_w >> (4 * c)) & 15) >= o.kw) return RHO_E_ARG;
        taps2 = (int64_t)o.kd * o.kh2 * o.kw2;
    }
    o.total = taps2 * o.d1 * o.d2;
    o.blk0 = 0;
    // One output element per thread, as the kernels this replaces: a lone launch is latency-bound, and on a table's blocks
    // (ceil(total / 1024)) it measured 0.4 - 1.8 us slower per call; blocks of an LDS-walk launch past its units return at once
    o.nblk = n_blocks_for(o.total, 256, 2048);
    const dim3 grid((unsigned)o.nblk), block(256);
    switch (o.kind) {
    case RHO_PREP_FWD: hipLaunchKernelGGL(k_prep_one<RHO_PREP_FWD>, grid, block, 0, as_stream(stream), o); break;
    case RHO_PREP_DGRAD: hipLaunchKernelGGL(k_prep_one<RHO_PREP_DGRAD>, grid, block, 0, as_stream(stream), o); break;
    case RHO_PREP_PHASE: hipLaunchKernelGGL(k_prep_one<RHO_PREP_PHASE>, grid, block, 0, as_stream(stream), o); break;
    default: hipLaunchKernelGGL(k_prep_one<RHO_PREP_SEL>, grid, block, 0, as_stream(stream), o);
    }
    RHO_LAUNCH_CHECK();
    return 0;
}

static rho_prep_op prep_op(int kind, const float* w, void* out, int dtype, int64_t cout, int64_t cin, int kd, int kh, int kw, int64_t d1,
                           int64_t d2) {
    rho_prep_op o = {};
    o.w = w; o.out = out; o.kind = kind; o.dtype = dtype;
    o.cout = cout; o.cin = cin; o.kd = kd; o.kh = kh; o.kw = kw; o.d1 = d1; o.d2 = d2;
    return o;
}

extern "C" int rho_prep_conv_weight(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int64_t taps,
                                    int64_t coutp, int64_t cinp, const int32_t* row_src, void* stream) {
    rho_prep_op o = prep_op(RHO_PREP_FWD, w, out, dtype, cout, cin, 1, 1, taps32(taps), coutp, cinp);
    o.perm = row_src;
    return prep_one(o, stream);
}

extern "C" int rho_prep_conv_weight_dgrad(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int64_t taps,
                                          int64_t rowsp, int64_t colsp, const int32_t* col_src, void* stream) {
    rho_prep_op o = prep_op(RHO_PREP_DGRAD, w, out, dtype, cout, cin, 1, 1, taps32(taps), rowsp, colsp);
    o.perm = col_src;
    return prep_one(o, stream);
}

extern "C" int rho_prep_conv_weight_phase(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int kd, int kh, int kw, int ph_h,
                                          int ph_w, int64_t coutp, int64_t cinp, int dgrad, void* stream) {
    rho_prep_op o = prep_op(RHO_PREP_PHASE, w, out, dtype, cout, cin, kd, kh, kw, dgrad ? cinp : coutp, dgrad ? coutp : cinp);
    o.ph_h = ph_h; o.ph_w = ph_w; o.dgrad = dgrad != 0;
    return prep_one(o, stream);
}

extern "C" int rho_prep_conv_weight_sel(const float* w, void* out, int dtype, int64_t cout, int64_t cin, int kd, int kh, int kw, int kh2,
                                        int kw2, int sel_h, int sel_w, int flip_d, int64_t coutp, int64_t cinp, int dgrad, void* stream) {
    rho_prep_op o = prep_op(RHO_PREP_SEL, w, out, dtype, cout, cin, kd, kh, kw, dgrad ? cinp : coutp, dgrad ? coutp : cinp);
    o.kh2 = kh2; o.kw2 = kw2; o.sel_h = sel_h; o.sel_w = sel_w; o.flip_d = flip_d != 0; o.dgrad = dgrad != 0;
    return prep_one(o, stream);
}

// ================================================================================================ weight-gradient finalize
template <bool ACC>
__device__ __forceinline__ void wfin_store(float* g, float v) { *g = ACC ? *g + v : v; }

// Element i of the parameter gradient walked in buffer-row order; kinds: rho_wfin_op, include/rho_hip.h
template <bool ACC>
__device__ __forceinline__ void wfin_elem(const rho_wfin_op& o, int64_t i, int kind) {
    const int64_t taps = (int64_t)o.kd * o.kh * o.kw;
    const int tap = (int)(i % taps);
    const int64_t ci = (i / taps) % o.cin;
    const int64_t r = i / (taps * o.cin);
    if (kind == 2) {          // i walks [ci][tap]: grad[ci][tap] += dw[taps - 1 - tap][ci]
        const int64_t cc = i / taps;
        if (cc < o.cin) wfin_store<ACC>(o.grad + i, o.dw[(int64_t)(taps - 1 - tap) * o.cinb + cc]);
        return;
    }
    if (kind == 0) {          // fp32 [taps][coutp][cinb] -> [cout][cin][taps], undoing the qkv row permutation if any
        const int64_t dst_row = o.row_src ? (int64_t)o.row_src[r] : r;
        if (dst_row < 0 || dst_row >= o.cout) return;
        wfin_store<ACC>(o.grad + (dst_row * o.cin + ci) * taps + tap, o.dw[((int64_t)tap * o.coutp + r) * o.cinb + ci]);
        return;
    }
    // kind 1: every source tap takes the phase tap its row / column was summed into, over ALL phases of the conv, added once
    const int kx = tap % o.kw, ky = (tap / o.kw) % o.kh, kz = tap / (o.kw * o.kh);
    const int kh2 = o.up_h ? 2 : o.kh, kw2 = o.up_w ? 2 : o.kw;
    const int nb = o.up_w ? 2 : 1;
    float v = 0.0f;
    for (int a = (o.up_h ? 1 : 0); a <= (o.up_h ? 2 : 0); ++a)
        for (int b = (o.up_w ? 1 : 0); b <= (o.up_w ? 2 : 0); ++b) {
            const int r2 = phase_tap_of(a, ky), c2 = phase_tap_of(b, kx);
            const int pidx = (o.up_h ? a - 1 : 0) * nb + (o.up_w ? b - 1 : 0);
            v += o.dw[(int64_t)pidx * o.phase_stride + ((int64_t)((kz * kh2 + r2) * kw2 + c2) * o.coutp + r) * o.cinb + ci];
        }
    wfin_store<ACC>(o.grad + i, v);
}

constexpr int WFIN_TILE = 32 * 65;             // [tap][64 channels] (+1: conflict-free column reads)
template <bool ACC, int KIND>                  // KIND as in prep_block
__device__ __forceinline__ void wfin_block(const rho_wfin_op& o, int block, int nblk, float* tile) {
    const int kind = KIND < 0 ? o.kind : KIND;
    const int taps = o.kd * o.kh * o.kw;
    if (kind == 0 && taps > 1 && taps <= 32) {
        // [tap][row][channel] -> [row][channel][tap] through LDS: the buffer is read in 256-byte channel runs (one per tap), the
        // gradient written as one contiguous run of 64 * taps floats - both sides coalesced (the elementwise walk reads the buffer
        // with a stride of coutp * cin_buf floats between consecutive threads)
        const int64_t cg = (o.cin + 63) / 64;                      // 64-channel groups per row
        const int64_t units = o.cout * cg;
        for (int64_t u = block; u < units; u += nblk) {
            const int64_t r = u / cg;
            const int ci0 = (int)(u % cg) * 64;
            const int nc = (int)min((int64_t)64, o.cin - ci0);
            for (int e = threadIdx.x; e < taps * 64; e += 256) {
                const int t = e >> 6, c = e & 63;
                tile[t * 65 + c] = c < nc ? o.dw[((int64_t)t * o.coutp + r) * o.cinb + ci0 + c] : 0.0f;
            }
            __syncthreads();
            const int64_t dst_row = o.row_src ? (int64_t)o.row_src[r] : r;
            if (dst_row >= 0 && dst_row < o.cout) {
                float* g = o.grad + (dst_row * o.cin + ci0) * taps;
                for (int e = threadIdx.x; e < nc * taps; e += 256) {
                    const float v = tile[(e % taps) * 65 + e / taps];
                    if (ACC) g[e] += v; else g[e] = v;
                }
            }
            __syncthreads();
        }
        return;
    }
    const int64_t stride = (int64_t)nblk * 256;
    for (int64_t i = (int64_t)block * 256 + threadIdx.x; i < o.total; i += stride) wfin_elem<ACC>(o, i, kind);
}

// rho_wgrad_finalize_batch: the accumulation buffers of MANY convolutions (and their channel-sum vectors = bias gradients) into
// the parameter-gradient layout in one launch (one launch per buffer: ~170 launches per training step at BASELINE configs[2]).
// Always accumulates; kind 1 is ONE op for all phases of a conv, so no two ops of a launch touch the same gradient element.
__global__ __launch_bounds__(256) void k_wgrad_finalize_batch(const rho_wfin_op* __restrict__ ops, int nops) {
    __shared__ float tile[WFIN_TILE];
    int lo = 0, hi = nops - 1;
    const int b = (int)blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ops[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const rho_wfin_op o = ops[lo];
    wfin_block<true, -1>(o, b - o.blk0, o.nblk, tile);
}

extern "C" int rho_wgrad_finalize_batch(const rho_wfin_op* ops_dev, int64_t n_ops, int64_t n_blocks, void* stream) {
    if (!ops_dev || n_ops <= 0 || n_blocks <= 0 || n_blocks > 0x7FFFFFFF || n_ops > 0x7FFFFFFF) return RHO_E_ARG;
    hipLaunchKernelGGL(k_wgrad_finalize_batch, dim3((unsigned)n_blocks), dim3(256), 0, as_stream(stream), ops_dev, (int)n_ops);
    RHO_LAUNCH_CHECK();
    return 0;
}

template <bool ACC>
__global__ __launch_bounds__(256) void k_wfin_one(rho_wfin_op o) {
    __shared__ float tile[WFIN_TILE];
    wfin_block<ACC, 0>(o, (int)blockIdx.x, (int)gridDim.x, tile);
}

// One buffer: a kind-0 op by value; accumulate = 1 adds to the existing .grad
extern "C" int rho_wgrad_finalize(const float* dw, float* grad, int64_t cout, int64_t cin, int64_t taps, int64_t coutp,
                                  int64_t cin_buf, const int32_t* row_src, int accumulate, void* stream) {
    rho_wfin_op o = {};
    o.dw = dw; o.grad = grad; o.row_src = row_src;
    o.cout = cout; o.cin = cin; o.coutp = coutp; o.cinb = cin_buf;
    o.kd = o.kh = 1; o.kw = taps32(taps);
    if (!dw || !grad || cout <= 0 || cin <= 0 || o.kw <= 0 || coutp < cout || cin_buf < cin) return RHO_E_ARG;
    o.total = cout * cin * taps;
    o.nblk = n_blocks_for(o.total, 256, 2048);
    const dim3 grid((unsigned)o.nblk), block(256);
    if (accumulate) hipLaunchKernelGGL(k_wfin_one<true>, grid, block, 0, as_stream(stream), o);
    else hipLaunchKernelGGL(k_wfin_one<false>, grid, block, 0, as_stream(stream), o);
    RHO_LAUNCH_CHECK();
    return 0;
}

// ONE sub-pixel phase (buffer [kd * kh' * kw' taps][coutp][cin_buf], kh' / kw' = 2 on the phased axes) added to the gradient
// [cout][cin][kd * kh * kw] per call; kind 1 sums the phases first - another floating-point order, so this stays its own kernel.
__global__ __launch_bounds__(256) void k_wgrad_finalize_phase(const float* __restrict__ dw, float* __restrict__ grad, int64_t cout,
                                                              int64_t cin, int kd, int kh, int kw, int ph_h, int ph_w, int64_t coutp,
                                                              int64_t cinb, int accumulate) {
    const int64_t taps = (int64_t)kd * kh * kw;
    const int kh2 = ph_h ? 2 : kh, kw2 = ph_w ? 2 : kw;
    const int64_t total = cout * cin * taps;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(i % taps);
        const int64_t ci = (i / taps) % cin;
        const int64_t r = i / (taps * cin);
        const int kx = tap % kw, ky = (tap / kw) % kh, kz = tap / (kw * kh);
        const float v = dw[((int64_t)((kz * kh2 + phase_tap_of(ph_h, ky)) * kw2 + phase_tap_of(ph_w, kx)) * coutp + r) * cinb + ci];
        grad[i] = accumulate ? grad[i] + v : v;
    }
}

extern "C" int rho_wgrad_finalize_phase(const float* dw, float* grad, int64_t cout, int64_t cin, int kd, int kh, int kw, int ph_h, int ph_w,
                                        int64_t coutp, int64_t cin_buf, int accumulate, void* stream) {
    if (!dw || !grad || cout <= 0 || cin <= 0 || kd <= 0 || kh <= 0 || kw <= 0 || coutp < cout || cin_buf < cin) return RHO_E_ARG;
    if (bad_phase(ph_h, ph_w, kh, kw)) return RHO_E_ARG;
    const int g = n_blocks_for(cout * cin * kd * kh * kw, 256, 2048);
    hipLaunchKernelGGL(k_wgrad_finalize_phase, dim3((unsigned)g), dim3(256), 0, as_stream(stream), dw, grad, cout, cin, kd, kh, kw, ph_h, ph_w,
                       coutp, cin_buf, accumulate);
    RHO_LAUNCH_CHECK();
    return 0;
}
