// Host-side selection of the attention kernels: ONE plan per (dtype, ch, direction), computed once per call, behind
// rho_attention_fwd, rho_attention_bwd and rho_attention_variant.  The launches switch on the plan's (kind, ch, tile) and only
// map it to a template instantiation; which kernel a head width gets, with which tile length, is decided here and nowhere else.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "common.h"

enum AttnKind {
    ATTN_FWD_BF16,     // k_attn_bf16<CH, KT>
    ATTN_FWD_F32M,     // k_attn_f32m<CH, KT>                         exact f32 on the matrix cores
    ATTN_FWD_F32,      // k_attn_f32<CH, KT>                          exact f32, VALU (RHO_ATTN_F32_VALU=1)
    ATTN_BWD_PAIR,     // k_attn_dq<CH, KT> + k_attn_dkv<CH, KT, 0 / 1>
    ATTN_BWD_FUSED,    // k_attn_dq<CH, KT> + k_attn_dkv_fused<CH, KT>  (ch = 64 unless RHO_ATTN_DKV_SPLIT=1)
    ATTN_BWD_F32M,     // k_attn_dq_f32m<CH, KT> + k_attn_dkv_f32m<CH, KT>
    ATTN_BWD_F32,      // k_attn_dq_f32<CH, KT> + k_attn_dkv_f32<CH, KT>  (ch = 256, or RHO_ATTN_F32_VALU=1)
};

struct AttnPlan {
    int rc;            // 0, RHO_E_ARG or RHO_E_SHAPE: what the launch returns for this (dtype, ch)
    AttnKind kind;
    int ch;
    int kt;            // keys (forward, dQ) / queries (dK, dV) per LDS tile
    int rows;          // queries (keys) per workgroup: the grid's x extent is ceil(T / rows)
};

// Both switches are read once per process (the first launch or query latches them).
inline bool attn_env_f32_valu() {
    static const bool v = getenv("RHO_ATTN_F32_VALU") && atoi(getenv("RHO_ATTN_F32_VALU")) != 0;
    return v;
}
inline bool attn_env_dkv_split() {
    static const bool v = getenv("RHO_ATTN_DKV_SPLIT") && atoi(getenv("RHO_ATTN_DKV_SPLIT")) != 0;
    return v;
}

// key of a (ch, tile) pair for the launch switches
#define RHO_ATTN_KEY(ch, kt) ((ch) * 1024 + (kt))

inline AttnPlan attn_plan(int dtype, int64_t ch, bool backward) {
    AttnPlan p = {0, ATTN_FWD_BF16, (int)ch, 0, 128};
    if (dtype != RHO_BF16 && dtype != RHO_F32) {
        p.rc = RHO_E_ARG;
        return p;
    }
    if (ch != 16 && ch != 32 && ch != 64 && ch != 128 && ch != 256) {
        p.rc = RHO_E_SHAPE;
        return p;
    }
    if (dtype == RHO_BF16) {
        // KT = 32 at ch = 256 keeps the K and V^T (Q and dO) tiles inside static LDS
        p.kt = ch >= 256 ? 32 : 64;
        if (!backward) p.kind = ATTN_FWD_BF16;
        // ch = 64: dQ + the fused dK / dV kernel; RHO_ATTN_DKV_SPLIT=1 keeps the pair (A/B).  ch = 128 stays on the pair: fused it
        // needs 128 accumulator + 32 K-fragment + 32 score registers + operands > 256 per wave at two waves per SIMD.
        else p.kind = (ch == 64 && !attn_env_dkv_split()) ? ATTN_BWD_FUSED : ATTN_BWD_PAIR;
        return p;
    }
    // exact f32: MFMA kernels; RHO_ATTN_F32_VALU=1 selects the VALU kernels (A/B and cross-check).  The backward at ch = 256
    // keeps the VALU pair: two 128-register accumulators + fragments do not fit a wave.
    const bool valu = attn_env_f32_valu() || (backward && ch > 128);
    if (valu) {
        p.kind = backward ? ATTN_BWD_F32 : ATTN_FWD_F32;
        p.kt = ch <= 64 ? 64 : (ch == 128 ? 32 : 16);
        p.rows = 64;
    } else {
        p.kind = backward ? ATTN_BWD_F32M : ATTN_FWD_F32M;
        p.kt = backward ? (ch <= 32 ? 64 : 32) : (ch <= 64 ? 64 : 32);
    }
    return p;
}

// "k_attn_bf16<64,64>"; backward: "k_attn_delta<bf16>+k_attn_dq<64,64>+k_attn_dkv_fused<64,64>"
inline void attn_plan_name(const AttnPlan& p, char* buf, int cap) {
    const int c = p.ch, k = p.kt;
    switch (p.kind) {
        case ATTN_FWD_BF16: snprintf(buf, cap, "k_attn_bf16<%d,%d>", c, k); break;
        case ATTN_FWD_F32M: snprintf(buf, cap, "k_attn_f32m<%d,%d>", c, k); break;
        case ATTN_FWD_F32: snprintf(buf, cap, "k_attn_f32<%d,%d>", c, k); break;
        case ATTN_BWD_PAIR:
            snprintf(buf, cap, "k_attn_delta<bf16>+k_attn_dq<%d,%d>+k_attn_dkv<%d,%d,0>+k_attn_dkv<%d,%d,1>", c, k, c, k, c, k);
            break;
        case ATTN_BWD_FUSED: snprintf(buf, cap, "k_attn_delta<bf16>+k_attn_dq<%d,%d>+k_attn_dkv_fused<%d,%d>", c, k, c, k); break;
        case ATTN_BWD_F32M: snprintf(buf, cap, "k_attn_delta<f32>+k_attn_dq_f32m<%d,%d>+k_attn_dkv_f32m<%d,%d>", c, k, c, k); break;
        case ATTN_BWD_F32: snprintf(buf, cap, "k_attn_delta<f32>+k_attn_dq_f32<%d,%d>+k_attn_dkv_f32<%d,%d>", c, k, c, k); break;
    }
}
