// Shared pieces of the bf16 attention kernels (attention.hip: k_attn_bf16; attention_bwd.hip: k_attn_dq, k_attn_dkv,
// k_attn_dkv_fused): the MFMA operand helpers of the accumulator-as-operand scheme, the LDS row tile, and the Q / dO tile stager
// of the key-stationary kernels.  The stager owns the registers a tile travels in and the addresses of a thread's share; it does
// not decide WHEN it is called: load(t0) only issues the global loads, store(t0) only writes LDS, and the kernel places the two
// around its barriers (under the previous tile's MFMAs where it has the registers, between the barriers where it has not).
// k_attn_bf16 and k_attn_dq stage their K / V^T tiles with code of their own (DESIGN.md section 3 says why).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) short s16x4_t;

__device__ __forceinline__ uint4 tr_frag2(const char* lds, int r0, int r1) {
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds + r0));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(lds + r1));
    uint4 f;
    f.x = (uint32_t)(uint16_t)lo[0] | ((uint32_t)(uint16_t)lo[1] << 16);
    f.y = (uint32_t)(uint16_t)lo[2] | ((uint32_t)(uint16_t)lo[3] << 16);
    f.z = (uint32_t)(uint16_t)hi[0] | ((uint32_t)(uint16_t)hi[1] << 16);
    f.w = (uint32_t)(uint16_t)hi[2] | ((uint32_t)(uint16_t)hi[3] << 16);
    return f;
}

__device__ __forceinline__ f32x16_t mma_bf16(const uint4& a, const uint4& b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// pi: bits 2 and 3 of a tile row swapped.  A-operand rows fetched in this order make the accumulator of one MFMA, converted
// pairwise to bf16, the B operand of the next.
__device__ __forceinline__ int pi_row(int r) { return (r & 0x13) | ((r & 4) << 1) | ((r & 8) >> 1); }

// accumulator registers 8s..8s+7 -> bf16 B-operand fragment of k-step s
__device__ __forceinline__ uint4 acc_to_frag(const f32x16_t& v, int st) {
    uint4 f;
    f.x = pack_bf16x2(v[8 * st + 0], v[8 * st + 1]);
    f.y = pack_bf16x2(v[8 * st + 2], v[8 * st + 3]);
    f.z = pack_bf16x2(v[8 * st + 4], v[8 * st + 5]);
    f.w = pack_bf16x2(v[8 * st + 6], v[8 * st + 7]);
    return f;
}

// ------------------------------------------------------------------------------------------------ LDS tile layout
// A [row][CH] bf16 tile is read two ways: whole 16-byte row pieces (ds_read_b128, 16 different rows per lane group)
// and transposed 4-row x 64-byte windows (ds_read_b64_tr_b16, one half-wave = rows r..r+3 of one window).  A padded
// pitch serves only one of them (odd 16-byte-slot pitch: b128 conflict-free, the 4 windows overlap 4-fold - PMC:
// SQ_LDS_BANK_CONFLICT = 50 % of SQ_LDS_IDX_ACTIVE in these kernels).  For CH = 128 the rows are therefore unpadded
// (256 B = all 64 banks) and the 16-byte slot is XORed with a bit-permutation of the row index: bits 0-1 of the row
// pick the 64-byte window (4 consecutive rows -> 4 windows: tr reads conflict-free), bits 2-3 the slot inside it
// (any 16 rows distinct mod 16 -> 16 distinct slots: b128 reads conflict-free).
template <int CH>
struct RowTile {
    static constexpr bool SWZ = (CH == 128);
    static constexpr int P = SWZ ? 256 : CH * 2 + 16;
    static __device__ __forceinline__ int swz(int row) { return SWZ ? ((((row & 3) << 2) | ((row >> 2) & 3)) << 4) : 0; }
    // byte offset of 16-byte-aligned `byte` (may carry an 8-byte sub-offset) in `row`
    static __device__ __forceinline__ int at(int row, int byte) { return row * P + (byte ^ swz(row)); }
};

// ------------------------------------------------------------------------------------------------ Q + dO tile
// One QT-query tile of one (batch, head) for the key-stationary kernels: Q and dO rows as two RowTile<CH> tiles, -lse per query
// (-inf for rows beyond T: exp2(-inf) = 0 masks them) and, where the kernel computes dS (DK), -delta * scale.  Whole tiles use a
// scalar tile origin + per-thread 32-bit offsets computed once instead of clamps, selects and 64-bit multiplies per tile.
template <int CH, int QT, bool DK>
struct QdStage {
    using QL = RowTile<CH>;
    static constexpr int QPC = CH / 8;
    static constexpr int QIT = (QT * QPC + 255) / 256;
    static constexpr bool QEXACT = (QIT * 256 == QT * QPC);

    uint4 vq[QIT], vd[QIT];
    float nl_r = 0.0f, nd_r = 0.0f;
    unsigned qoff[QIT], doff[QIT], qlds[QIT];
    const bf16_raw *qbase, *dbase;
    const float *lbase, *ebase;
    char *q_lds, *d_lds;
    float *nlse_s, *ndel_s;
    size_t row2c;
    float scale;
    int T, C, tid;

    // qbase / dbase: row 0 of the head in qk (row stride row2c) / dout (row stride C); lbase / ebase: lse / delta of the head
    __device__ __forceinline__ void init(const bf16_raw* qbase_, size_t row2c_, const bf16_raw* dbase_, int C_, const float* lbase_,
                                         const float* ebase_, float scale_, int T_, char* q_lds_, char* d_lds_, float* nlse_s_,
                                         float* ndel_s_) {
        qbase = qbase_, dbase = dbase_, lbase = lbase_, ebase = ebase_, q_lds = q_lds_, d_lds = d_lds_, nlse_s = nlse_s_, ndel_s = ndel_s_;
        row2c = row2c_, scale = scale_, T = T_, C = C_, tid = threadIdx.x;
#pragma unroll
        for (int i = 0; i < QIT; ++i) {
            const int pc = tid + 256 * i, q = pc / QPC, piece = pc % QPC;
            qoff[i] = (unsigned)(((size_t)q * row2c + piece * 8) * 2);
            doff[i] = (unsigned)(((size_t)q * C + piece * 8) * 2);
            qlds[i] = (unsigned)QL::at(q, piece * 16);
        }
    }
    __device__ __forceinline__ bool whole(int qt0) const { return QEXACT && qt0 + QT <= T; }   // (uniform)

    __device__ __forceinline__ void load(int qt0) {
        if (whole(qt0)) {
            const char* const qb = reinterpret_cast<const char*>(qbase) + (size_t)qt0 * row2c * 2;
            const char* const db = reinterpret_cast<const char*>(dbase) + (size_t)qt0 * C * 2;
#pragma unroll
            for (int i = 0; i < QIT; ++i) {
                vq[i] = *reinterpret_cast<const uint4*>(qb + qoff[i]);
                vd[i] = *reinterpret_cast<const uint4*>(db + doff[i]);
            }
            if (tid < QT) {
                nl_r = -lbase[qt0 + tid];
                if constexpr (DK) nd_r = -ebase[qt0 + tid] * scale;
            }
        } else {
#pragma unroll
            for (int i = 0; i < QIT; ++i) {
                const int pc = tid + 256 * i;
                const int q = QEXACT ? pc / QPC : min(pc / QPC, QT - 1), piece = pc % QPC;
                const size_t qr = (size_t)min(qt0 + q, T - 1);
                vq[i] = *reinterpret_cast<const uint4*>(qbase + qr * row2c + piece * 8);
                vd[i] = *reinterpret_cast<const uint4*>(dbase + qr * C + piece * 8);
            }
            if (tid < QT) {
                const bool ok = qt0 + tid < T;
                nl_r = ok ? -lbase[qt0 + tid] : -INFINITY;          // exp2(-inf) = 0 masks the row
                if constexpr (DK) nd_r = ok ? -ebase[qt0 + tid] * scale : 0.0f;
            }
        }
    }
    __device__ __forceinline__ void store(int qt0) {
        if (tid < QT) {
            nlse_s[tid] = nl_r;
            if constexpr (DK) ndel_s[tid] = nd_r;
        }
        if (whole(qt0)) {
#pragma unroll
            for (int i = 0; i < QIT; ++i) {
                *reinterpret_cast<uint4*>(q_lds + qlds[i]) = vq[i];
                *reinterpret_cast<uint4*>(d_lds + qlds[i]) = vd[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < QIT; ++i) {
                const int pc = tid + 256 * i;
                const int q = pc / QPC, piece = pc % QPC;
                if (QEXACT || pc < QT * QPC) {
                    const bool ok = qt0 + q < T;
                    *reinterpret_cast<uint4*>(q_lds + QL::at(q, piece * 16)) = ok ? vq[i] : make_uint4(0u, 0u, 0u, 0u);
                    *reinterpret_cast<uint4*>(d_lds + QL::at(q, piece * 16)) = ok ? vd[i] : make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
    }
};
