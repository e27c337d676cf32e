// n-D convolution (kernel 1 or 3 per axis, zero padding k/2) for channels-last activations as an
// implicit GEMM on the CDNA4 matrix cores, designed around the 160 KiB LDS of a gfx950 CU:
//
//   * A workgroup (4 waves) owns an output tile of 256 positions (TD x TH x TW, chosen per layer)
//     and BM output channels.  For each 64-byte input-channel chunk (32 bf16 / 16 f32 channels) it
//     stages the tile's input region INCLUDING THE HALO into LDS once -- applying the folded
//     GroupNorm+FiLM affine and SiLU on the way (unet_v2.py:212-216,285-289), zero-filling the
//     padding AFTER the activation -- and then runs all kd*kh*kw taps out of that resident tile
//     at shifted LDS addresses.  Global->LDS traffic is ~2.3x the input instead of 27x, the
//     GN/SiLU work is paid 2.3x instead of 27x, and torch.cat / nearest-upsample / stride never
//     exist as tensors: they are address arithmetic in the loader (unet_v2.py:729,122-131,153).
//   * Orientation is D[cout][position] = W[cout][k] * X[k][position] with 32x32 MFMA tiles
//     (v_mfma_f32_32x32x16_bf16, or the exact-f32 v_mfma_f32_32x32x2_f32): each lane ends up
//     holding 4 consecutive output channels of ONE position, so the epilogue (bias, residual,
//     additive embedding) writes 8/16-byte channels-last pieces with no shuffles.
//   * LDS rows are 64 B of payload on an 80 B pitch: for ds_read_b128 the 16-byte slot index is
//     5*row mod 16, a bijection, so 32 consecutive rows are conflict-free for every lane group.
//   * Weights ([tap][cout][cin], prepared once) stream through a 2-deep LDS ring, one tap ahead.
//
// Replaces conv_nd at every call site of rho_diffusion/models/unet_v2.py (see include/rho_hip.h).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "conv_common.h"

// Taps per workgroup barrier of the 8-wave M16 variant (with the tap order pinned, see RHO_FENCE: 3 is 3 % faster than 1; the
// LDS weight ring is 9 slots deep then).  The host sizes the ring with the same constant.
#define RHO_GB_WIDE 3
// ... and on the 32-cout variant (4 MFMAs per tap and wave = 128 MFMA cycles between barriers; round 3, c5's mc = 32 levels: conv3
// 17.5 -> 17.1 ms per sampling step in a same-box A/B, gpurun_out/ab2_*; 0 = a barrier per tap)
#ifndef RHO_GB_BM32
#define RHO_GB_BM32 1
#endif

struct ConvK {
    const char* x1;
    const char* x2;
    const float* pre_a;
    const float* pre_b;
    const char* w;
    const float* bias;
    const char* res;
    const float* res_add;
    char* y;
    char* y2;
    int c1, c2, cin;
    int cout, coutp, split;
    int D, H, W;     // input extents (depth carries the batch when merged)
    int Do, Ho, Wo;  // output extents
    long long S_in, S_out;  // positions per sample
    int sh, sw, up_h, up_w, pre_silu, y2_f32;
    int TD, TH, TW, ID, IH, IW, NP;
    int tiles_h, tiles_w;
    int res_add_stride;
    int y2_cl;            // y2 is channels-last [.., cout - split] (dgrad of a concatenated input) instead of channel-major
    const char* res2;     // residual for the y2 region (channels-last only): in-place gradient accumulation
    int pair_lg;          // -1: none; else log2 of the row-index bit that pairs two 8-wide halo rows 8 (mod 16) positions apart
    int zs_h, zs_w;       // zero-stuffed input (dgrad of a stride-2 conv): virtual extent H/W, source extent Hs/Ws
    int Hs, Ws;
    float* stats;         // fused GroupNorm statistics of the output: [N][tps][2][split] (see rho_conv_desc.stats)
    int tps;              // tiles per sample
    int lgTW, lgTH;       // tile extents are powers of two
    float inv_ihw, inv_iw;  // 1 / (IH*IW), 1 / IW: exact small-integer division through one float multiply
    int cofast;           // cout tiles of one position tile on consecutive launch slots of one XCD
    int coef_off;         // > 0: byte offset in LDS of the staged prologue coefficients [2][cin] (3-D tiles: one sample per tile)
    // Sub-pixel phase of a conv behind a nearest x2 upsample (rho_conv_desc.ph_h / ph_w): taps start pad_h / pad_w rows before the
    // output position; the launch writes output row oh * oy_mul + oy_add of a tensor with Ho_out x Wo_out rows per depth slice
    int pad_h, pad_w, oy_mul, oy_add, ox_mul, ox_add, Ho_out, Wo_out;
    int stats_off;        // first statistics tile of this launch within the tps tiles of a sample
    int iy_mul, iy_add, ix_mul, ix_add;   // input row / column of virtual position g: g * mul + add (phd_*: one parity of a 2x tensor)
    // GroupNorm backward reduction fused into a dgrad launch (rho_conv_desc.gnb_*): stats <- per-tile sums of dz and dz * x
    const char* gnb_x1;
    const char* gnb_x2;
    const float* gnb_a;
    const float* gnb_b;
    int gnb_c1, gnb_silu;
    // Split-K (small grids, rho_conv_desc.ws): blockIdx.z = k-split s of ksplit; the split contracts the input-channel chunks
    // [nck * s / ksplit, nck * (s + 1) / ksplit) and stores its fp32 partial tile to slab[s] ([positions][coutp]); k_splitk_reduce
    // adds the slabs, the bias, the residuals and rounds once
    int ksplit;
    float* slab;
    long long slab_stride;      // floats per split
    // Folded 1x1x1 skip convolution (rho_conv_desc.sk_*; FSK instantiations): contracted into the accumulators before the tap loop
    const char* sk_x1;
    const char* sk_x2;
    const char* sk_w;
    const float* sk_bias;
    int sk_c1, sk_c2;
    // GroupNorm backward APPLY fused into the epilogue (rho_conv_desc.gna_*): out += cA * (g * act'(a x0 + b)) + cQ * x0 + cP
    const char* gna_g;
    const float* gna_cA;
    const float* gna_cP;
    const float* gna_cQ;
    // GEO instantiations (compile-time 4 x 8 x 8 tile): floor(a / d) of a workgroup-uniform a as one scalar multiply-high, for
    // d = tiles_w, tiles_w * tiles_h and the number of cout tiles (see geo_div)
    unsigned mg_tw, mg_thw, mg_ct;
};

// The geometry the GEO instantiations of k_conv bake in: a 4 x 8 x 8 output tile of a stride-1 3x3x3 layer (10 x 10 halo rows per
// depth slice, 600 halo positions), whole tiles only, one sample per tile, row bit 2 pairing the 8-wide halo rows (the host loop in
// conv_plan_stages finds pair_lg = 2 for IW = 10: 4 rows = 40 positions = 8 mod 16)
struct Geo488 {
    static constexpr int TD = 4, TH = 8, TW = 8, ID = 6, IH = 10, IW = 10, NP = 600, LGTW = 3, LGTH = 3, PAIR_LG = 2;
};
// floor(a / d) = umulhi(a + 1, floor((2^32 - 1) / d)) for d >= 1 and d * (a + 1) <= 2^32 (the plan keeps a and d below 2^16)
__device__ __forceinline__ int geo_div(int a, unsigned magic) { return (int)__umulhi((unsigned)a + 1u, magic); }

// floor(a / d) for 0 <= a < 2^20 with inv = 1.0f / d: (a + 0.5) * inv is at least 0.5 / d away from an integer, the
// float error is ~1e-7 * a / d.  (The integer division sequence costs ~20 VALU instructions; the per-tile setup of the
// narrow layers ran 1100 VALU instructions of this kind against 430 MFMAs.)
__device__ __forceinline__ int fdiv_small(int a, float inv) { return (int)(((float)a + 0.5f) * inv); }


// Column c (0..31) of MFMA tile m (0..7 = wave*2 + j) -> index of the output position inside the 256-position tile.
// ds_read_b128 serves a wave in 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32): with an odd slot pitch a
// group is conflict-free iff its 16 halo positions are distinct mod 16.  So the columns are ordered group-major and
// each group gets either 16 consecutive positions of one row (TW >= 16) or, for 8-wide tiles, two rows whose halo
// offset is 8 (mod 16) -- the row bit `pair_lg` chosen on the host.  (PMC before this map: SQ_LDS_BANK_CONFLICT was
// 40-50 % of SQ_LDS_IDX_ACTIVE in this kernel.)
// position of rank k (0..15) of 16-position unit u (0..15): 16 positions whose halo rows are distinct mod 16
__host__ __device__ constexpr __forceinline__ int unit_position(int u, int k, int TW, int pair_lg) {
    if (TW == 8 && pair_lg >= 0) {
        const int lo = u & ((1 << pair_lg) - 1);
        const int row = ((u >> pair_lg) << (pair_lg + 1)) | lo | ((k >> 3) << pair_lg);
        return row * 8 + (k & 7);
    }
    return u * 16 + k;
}
__device__ __forceinline__ int tile_position(int m, int c, int TW, int pair_lg) {
    const int q = c >> 2;
    const int g = (0x96 >> q) & 1;                 // lane group of this column
    const int k = ((q >> 1) << 2) | (c & 3);       // rank inside the group, 0..15
    return unit_position(2 * m + g, k, TW, pair_lg);
}

// The 16x16x32 MFMA layout (M16 variants): a lane holds row / column i = lane & 15 and the 16-byte K piece lane >> 4, so
// a ds_read_b128 lane group {0-3, 12-15 | 20-27} mixes 8 rows at piece p with 8 rows at piece p + 1.  With the odd slot
// pitch that is conflict-free iff both 8-row halves have distinct halo rows (mod 16) of ONE parity: column tile m16 takes
// the ranks of parity (m16 & 1) of the two units of pair m16 >> 1 - half A (i in 0-3, 12-15) from the even unit, half B
// (i in 4-11) from the odd one.  The same 32 positions as the 32-wide tile m16 >> 1 of the other layout.
__host__ __device__ constexpr __forceinline__ int m16_hb(int i) { return (0x0FF0 >> i) & 1; }
__host__ __device__ constexpr __forceinline__ int m16_k8(int i) { return m16_hb(i) ? i - 4 : (i < 4 ? i : i - 8); }
__host__ __device__ constexpr __forceinline__ int tile_position16(int m16, int i, int TW, int pair_lg) {
    return unit_position(2 * (m16 >> 1) + m16_hb(i), 2 * m16_k8(i) + (m16 & 1), TW, pair_lg);
}

// GEO epilogue: a thread's item k is staged row lr0 + 32 * k (lr0 = its item-0 row, 0..31).  With TW = 8 and pair_lg = 2 the bits
// of the tile position that k sets (row bit 1, depth) are disjoint from those lr0 sets (row bits 0 and 2, the column), so
// position(lr0 + 32 k) = position(lr0) + geo_item_delta(k) with no carry between the (depth, row, column) fields.
__host__ __device__ constexpr int geo_row_position(int lr) { return tile_position16((lr >> 6) * 4 + ((lr >> 4) & 3), lr & 15, 8, 2); }
__host__ __device__ constexpr int geo_item_delta(int k) { return geo_row_position(32 * k); }
__host__ __device__ constexpr bool geo_items_additive(int nit) {
    for (int k = 0; k < nit; ++k)
        for (int lr0 = 0; lr0 < 32; ++lr0)
            if (geo_row_position(lr0 + 32 * k) != (geo_row_position(lr0) | geo_item_delta(k)) || (geo_row_position(lr0) & geo_item_delta(k)) != 0) return false;
    return true;
}

// GNA: the 1x1x1 instantiations whose epilogue carries the GroupNorm backward apply (rho_conv_desc.gna_*; no residual operand there:
// its 32 registers are what the extra operand takes)
// GEO: the tile geometry of Geo488 is a compile-time constant (the bf16 3x3x3 16x16x32 instantiations; conv_plan_stages selects it
// for whole 4 x 8 x 8 tiles of a stride-1 layer).  Halo decode, tap offsets and output offsets become constants or instruction
// immediates, the bounds tests of ragged tiles go, and a chunk's halo is staged in straight-line code.  The order of the MFMAs, of the
// statistics sums and of the prologue expressions is that of the generic form: outputs and statistics are bit-identical.
template <typename T, int KD, int KH, int KW, int BM, int MAXP, int NW, bool M16 = false, bool FSK = false, bool GNA = false, bool GEO = false>
// (second launch bound = waves per SIMD the register allocation must allow: 2 for the 8-wave variants and for the 4-wave 1x1x1
//  variant, which without it took 241 VGPRs + 64 AGPRs = one workgroup per CU and left its HBM-bound layers at 3.3 TB/s)
__global__ __launch_bounds__(NW * 64, (NW == 8 || (KD * KH * KW == 1 && MAXP <= 10)) ? 2 : 1) void k_conv(const ConvK p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int CK = ET<T>::CK;
    constexpr int PE = ET<T>::PE;
    constexpr int NT = KD * KH * KW;
    constexpr int NTHR = NW * 64;
    constexpr int RPP = NTHR / 4;          // rows (halo positions / weight rows) covered per staging pass
    constexpr int WCO = NW / 4;            // waves along cout
    constexpr int MT = BM / 32 / WCO;      // 32-row cout tiles per wave
    constexpr int WROWS = (BM + RPP - 1) / RPP;  // weight-tile rows per thread
    static_assert(!GEO || (M16 && sizeof(T) == 2 && KD == 3 && KH == 3 && KW == 3 && !GNA), "GEO: the bf16 3x3x3 16x16x32 variants");
    static_assert(!GEO || ((MAXP - 1) * RPP < Geo488::NP && MAXP * RPP >= Geo488::NP), "GEO: only the last halo slot is partial");
    // tile geometry: constants under GEO, launch parameters otherwise
    const int gTD = GEO ? Geo488::TD : p.TD, gTH = GEO ? Geo488::TH : p.TH, gTW = GEO ? Geo488::TW : p.TW;
    const int gIH = GEO ? Geo488::IH : p.IH, gIW = GEO ? Geo488::IW : p.IW, gNP = GEO ? Geo488::NP : p.NP;
    const int gLGTW = GEO ? Geo488::LGTW : p.lgTW, gLGTH = GEO ? Geo488::LGTH : p.lgTH, gPAIR = GEO ? Geo488::PAIR_LG : p.pair_lg;

    char* const halo = smem;
    char* const wbuf = smem + (size_t)gNP * PITCH;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wpos = wave & 3;             // position quarter of this wave
    const int wco = wave >> 2;             // cout half (NW == 8)
    const int half = lane >> 5;
    const int piece = tid & 3;

    // ---- tile coordinates
    // Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Give every XCD a contiguous range of
    // tiles instead of every 8th one, so that the halo faces shared by neighbouring tiles are re-read from the same L2.
    int bt = blockIdx.x;
    int ct = blockIdx.y;
    if (p.cofast) {
        // several cout tiles and gridDim.x a multiple of 8: the cout tiles of one position tile take consecutive launch
        // slots of the same XCD, so the input tile they all read comes from HBM once and from that L2 afterwards
        const int L = blockIdx.x + gridDim.x * blockIdx.y;
        const int slot = L >> 3;
        const int sq = GEO ? geo_div(slot, p.mg_ct) : slot / (int)gridDim.y;
        ct = slot - sq * (int)gridDim.y;
        bt = (L & 7) * ((int)gridDim.x >> 3) + sq;
    } else {
        const int nt = gridDim.x, per = nt >> 3;
        if (per > 0) {
            const int full = per << 3;                      // tiles covered by the 8 equal ranges; the tail keeps its index
            if (bt < full) bt = (bt & 7) * per + (bt >> 3);
        }
    }
    int tw_i, th_i, td_i;
    if constexpr (GEO) {
        const int row = geo_div(bt, p.mg_tw);          // td_i * tiles_h + th_i
        td_i = geo_div(bt, p.mg_thw);
        tw_i = bt - row * p.tiles_w;
        th_i = row - td_i * p.tiles_h;
    } else {
        tw_i = bt % p.tiles_w;
        th_i = (bt / p.tiles_w) % p.tiles_h;
        td_i = bt / (p.tiles_w * p.tiles_h);
    }
    const int co0 = ct * BM;
    const bool splitk = (KD != 3) && p.ksplit > 1;            // (2-D / 1-D launches have gridDim.z = 1 otherwise: z carries the k-split)
    const int n = splitk ? 0 : (int)blockIdx.z;
    const int od0 = td_i * gTD, oh0 = th_i * gTH, ow0 = tw_i * gTW;
    const int gd_base = od0 - (KD / 2);
    const int gh_base = GEO ? oh0 - 1 : p.up_h ? (oh0 / 2 - 1) : (oh0 * p.sh - p.pad_h);
    const int gw_base = GEO ? ow0 - 1 : p.up_w ? (ow0 / 2 - 1) : (ow0 * p.sw - p.pad_w);

    // ---- halo slots owned by this thread: global linear input position (or -1 = zero padding,
    //      -2 = beyond the tile) and sample index for the prologue coefficients
    constexpr int NSMP = (KD == 3) ? 1 : MAXP;  // 3-D tiles never straddle samples: the sample is blockIdx.z
    int spos[MAXP];
    int ssmp[NSMP];
    // GEO: whether this thread's last slot lies inside the 600 halo positions (every earlier slot does)
    const bool last_in = !GEO || (tid >> 2) + RPP * (MAXP - 1) < Geo488::NP;
    if constexpr (GEO) {
        // slot -> (id, ih, iw) by constant division; the position is the tile's first halo position (one scalar) plus id * H * W +
        // ih * W + iw; -1 = zero padding (and the slots past the tile, which are never written)
        const int hw = p.H * p.W;
        const int pos0 = ((n * p.D + gd_base) * p.H + gh_base) * p.W + gw_base;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const unsigned hp = (unsigned)(tid >> 2) + RPP * i;
            const unsigned id = hp / (Geo488::IH * Geo488::IW), r = hp - id * (Geo488::IH * Geo488::IW);
            const unsigned ih = r / Geo488::IW, iw = r - ih * Geo488::IW;
            bool ok = ((unsigned)(gd_base + (int)id) < (unsigned)p.D) & ((unsigned)(gh_base + (int)ih) < (unsigned)p.H) &
                      ((unsigned)(gw_base + (int)iw) < (unsigned)p.W);
            if (i == MAXP - 1) ok = ok && last_in;
            spos[i] = ok ? pos0 + (int)id * hw + (int)ih * p.W + (int)iw : -1;
        }
    } else {
        const int ihw = p.IH * p.IW;
#pragma unroll
        for (int i = 0; i < MAXP; ++i) {
            const int hp = (tid >> 2) + RPP * i;
            int pos = -2, smp = 0;
            if (hp < p.NP) {
                const int id = fdiv_small(hp, p.inv_ihw);
                const int r = hp - id * ihw;
                const int ih = fdiv_small(r, p.inv_iw);
                const int iw = r - ih * p.IW;
                const int gd = gd_base + id;
                int gh = gh_base + ih, gw = gw_base + iw;
                bool ok = ((unsigned)gd < (unsigned)p.D) & ((unsigned)gh < (unsigned)p.H) & ((unsigned)gw < (unsigned)p.W);
                if (p.zs_h) { ok = ok && ((gh & 1) == 0) && ((gh >> 1) < p.Hs); gh >>= 1; }
                if (p.zs_w) { ok = ok && ((gw & 1) == 0) && ((gw >> 1) < p.Ws); gw >>= 1; }
                if (ok) {
                    pos = ((n * p.D + gd) * p.Hs + (gh * p.iy_mul + p.iy_add)) * p.Ws + (gw * p.ix_mul + p.ix_add);
                    if constexpr (KD != 3) smp = (int)((long long)pos / p.S_in);
                } else {
                    pos = -1;
                }
            }
            spos[i] = pos;
            if constexpr (KD != 3) ssmp[i] = smp;
        }
    }

    // ---- per-lane LDS byte offsets of the B (activation) fragments, per column tile and tap axis
    // (M16: j = pair of 16-wide column tiles; the odd tile of a pair is one halo row = +PITCH further, stride 1 only)
    int offd[2], offh[2][KH], offw[2][KW];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pp = M16 ? tile_position16(2 * (wpos * 2 + j), lane & 15, gTW, gPAIR)
                           : tile_position(wpos * 2 + j, lane & 31, gTW, gPAIR);
        const int pw = pp & (gTW - 1);
        const int ph = (pp >> gLGTW) & (gTH - 1);
        const int pd = pp >> (gLGTW + gLGTH);
        offd[j] = pd * gIH * gIW * PITCH + 16 * (M16 ? (lane >> 4) : half);
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) {
            const int ih = GEO ? ph + kh : p.up_h ? (((ph + kh - 1) >> 1) + 1) : (ph * p.sh + kh);
            offh[j][kh] = ih * gIW * PITCH;
        }
#pragma unroll
        for (int kw = 0; kw < KW; ++kw) {
            const int iw = GEO ? pw + kw : p.up_w ? (((pw + kw - 1) >> 1) + 1) : (pw * p.sw + kw);
            offw[j][kw] = iw * PITCH;
        }
    }
    // M16: MFMA row i of cout tile t (16 couts) lives in LDS row 32 * (t >> 1) + 16 * hb(i) + 2 * k8(i) + (t & 1)
    const int a_off = M16 ? (wco * (BM / WCO) + 16 * m16_hb(lane & 15) + 2 * m16_k8(lane & 15)) * PITCH + 16 * (lane >> 4)
                          : (wco * (BM / WCO) + (lane & 31)) * PITCH + 16 * half;

    f32x16_t acc[MT][2];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][j][r] = 0.0f;

    int ck_lo = 0, nck = p.cin / CK;
    if (splitk) {
        const int nall = nck, kz = (int)blockIdx.z;
        ck_lo = (int)((long long)nall * kz / p.ksplit);
        nck = (int)((long long)nall * (kz + 1) / p.ksplit) - ck_lo;       // >= 1: the host keeps ksplit <= chunks
    }
    const size_t wrow_bytes = (size_t)p.cin * sizeof(T);

    // weight tile: BM rows x 4 pieces of 16 B; thread -> row (tid>>2) + 64*k, piece tid&3.
    // (plain scalars, no arrays by reference: those end up in scratch)
    const bool w_active = (BM >= RPP) || (tid < BM * 4);
    // address = uniform 64-bit base (tap, chunk, cout tile: scalar ALU) + one 32-bit per-thread offset, the `saddr` form of
    // global_load: per-tap 64-bit pointers in VGPRs (27 taps x 2 registers, hoisted out of the chunk loop) spilled to scratch
    const char* const w_src0 = p.w + (size_t)co0 * wrow_bytes + (size_t)ck_lo * 64;      // (a chunk is 64 bytes of every weight row)
    // (re-declared opaque at every chunk: otherwise base + tap * stride + offset is hoisted as 27 per-lane 64-bit pointers anyway)
    unsigned w_voff = (unsigned)(tid >> 2) * (unsigned)wrow_bytes + (unsigned)piece * 16u;         // < 128 rows x 16 KiB
    const size_t w_tap_stride = (size_t)p.coutp * wrow_bytes;
    int w_row = tid >> 2;                  // LDS row of this thread's weight row(s); rows RPP apart keep the permutation
    if constexpr (M16) w_row = (w_row & ~31) + 16 * m16_hb(w_row & 15) + 2 * m16_k8(w_row & 15) + ((w_row >> 4) & 1);
    const int w_dst0 = w_row * PITCH + piece * 16;
    // Weights: G taps form one barrier step (G = 3 for the narrow-cout variants, where 8 MFMAs per barrier would be
    // barrier-bound), fetched PD steps ahead of their use (L2 latency ~1.5k cycles vs 0.25-0.5k cycles of MFMA per
    // tap) into a register ring of PD sets; set (step % PD) holds that step's G tiles; the LDS ring stays 2 deep.
    constexpr int G = 1;   // measured: G = 3 on the narrow-cout variants changes nothing (barriers are not their limiter)
    constexpr int NS = NT / G;
    constexpr int PD = (NS % 3 == 0) ? 3 : 1;
    constexpr int SLOT = G * BM * PITCH;
    uint4 wq0[PD][G], wq1[PD][G];
#pragma unroll
    for (int i = 0; i < PD; ++i)
#pragma unroll
        for (int g = 0; g < G; ++g) wq0[i][g] = wq1[i][g] = make_uint4(0u, 0u, 0u, 0u);
#define RHO_LOAD_W(set_, ck_, st_)                                                                       \
    do {                                                                                                \
        _Pragma("unroll") for (int g_ = 0; g_ < G; ++g_) {                                              \
            const char* ws_ = w_src0 + (size_t)((st_) * G + g_) * w_tap_stride + (size_t)(ck_) * 64;    \
            if (w_active) wq0[set_][g_] = *reinterpret_cast<const uint4*>(ws_ + w_voff);                \
            if constexpr (WROWS == 2) wq1[set_][g_] = *reinterpret_cast<const uint4*>(ws_ + RPP * wrow_bytes + w_voff); \
        }                                                                                               \
    } while (0)
// PIPE paths inside the chunk loop: the fetch pointer `wl` walks tap by tap (a loop-carried scalar: nothing to hoist, two scalar
// adds per tap; 27 hoisted 64-bit bases overflowed the SGPR file and came back as v_readlane per use).
#define RHO_LOAD_WP(set_, st_)                                                                          \
    do {                                                                                                \
        if (w_active) wq0[set_][0] = *reinterpret_cast<const uint4*>(wl + w_voff);                      \
        if constexpr (WROWS == 2) wq1[set_][0] = *reinterpret_cast<const uint4*>(wl + RPP * wrow_bytes + w_voff); \
        if (((st_) + LD) % NS == NS - 1) wl = w_src0 + (size_t)min(ck + ((st_) + LD) / NS + 1, nck - 1) * 64; \
        else wl += w_tap_stride;                                                                        \
    } while (0)
#define RHO_STORE_W(buf_, set_)                                                                         \
    do {                                                                                                \
        _Pragma("unroll") for (int g_ = 0; g_ < G; ++g_) {                                              \
            char* wd_ = wbuf + (size_t)(buf_) * SLOT + g_ * BM * PITCH + w_dst0;                        \
            if (w_active) *reinterpret_cast<uint4*>(wd_) = wq0[set_][g_];                               \
            if constexpr (WROWS == 2) *reinterpret_cast<uint4*>(wd_ + RPP * PITCH) = wq1[set_][g_];     \
        }                                                                                               \
    } while (0)

    // Pipelined variant (3 | NS, i.e. every kernel with more than one tap): an R-slot LDS weight ring, slot = step % R.
    // Step q's tile is fetched at step q-LD into register set q % 3, handed to LDS at the end of step q-D (two steps in
    // flight) and read from step q-1 on, at least one barrier AFTER it was written - so the fragment reads of step q+1
    // are issued while step q's MFMAs run, instead of right after a barrier with every wave of the workgroup waiting.
    // GB = steps per barrier: a write at step q needs a barrier in (q, q+D-1] before its first read and one in
    // (q+D-R, q] after the slot's last read, i.e. D = GB+1 and R >= 2*GB+1 (R = 9 for GB = 3 keeps the slot static).
    constexpr bool PIPE = (NS % 3 == 0) && (G == 1);
    // measured on the 8-wave 128-cout variant: GB = 3, R = 9 is 3 % SLOWER than a barrier per tap (131 vs 127 ms per
    // c3 step) - the per-tap barrier is not what limits this kernel - so GB stays 1.
    // (the slot of a step is st % RS: the ring depth must divide the taps of a chunk - 9 | 27 and 9 | 9, not the 3 taps of 1-D)
    constexpr int GB = (NS % 9 == 0 && ((BM == 128 && NW == 8 && M16) || (RHO_GB_BM32 && BM == 32 && !M16))) ? RHO_GB_WIDE : 1;
    constexpr int RS = (GB == 3) ? 9 : 3;          // LDS ring slots
    constexpr int DS = GB + 1;                     // store distance
    constexpr int LD = DS + 2;                     // load distance
    // Folded GroupNorm affine of the prologue: read from global memory at every chunk's landing it is one exposed L2 round
    // trip per chunk; a 3-D tile lies in one sample, so that sample's coefficients are staged in LDS once per tile.
    const float* coef = nullptr;
    if constexpr (NT != 1 && KD == 3) {
        if ((GEO || p.coef_off > 0) && p.pre_a != nullptr) {      // (GEO: the plan refuses the path without staged coefficients)
            float* cw_ = reinterpret_cast<float*>(smem + p.coef_off);
            for (int i = tid; i < p.cin; i += NTHR) {
                cw_[i] = p.pre_a[(size_t)n * p.cin + i];
                cw_[p.cin + i] = p.pre_b[(size_t)n * p.cin + i];
            }
            coef = cw_;
            __syncthreads();
        }
    }
    if constexpr (FSK) {
        // ---- folded 1x1x1 skip convolution: acc += sk_w[co][:] . cat(sk_x1, sk_x2)[position][:] over the tile's 256 output positions,
        // one "tap" of the M16 schedule per 32-channel chunk, BEFORE the tap loop touches LDS.  The activations are staged in the
        // tile's own order (row r = position r of the tile: the odd 16-column tile of a pair is one row further, as in the halo)
        // into two buffers over the bytes the halo tile and the weight ring use afterwards; chunk c + 1 is fetched while chunk c
        // runs, one barrier per chunk.
        static_assert(M16 && MT == 2 && KD == 3, "folded skip: the 64-couts-per-wave 16x16x32 layout of the 3-D kernels");
        typedef float f32x4_t __attribute__((ext_vector_type(4)));
        typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
        constexpr int XR = 256 / RPP;                       // activation rows per thread
        const int skc = p.sk_c1 + p.sk_c2, nsk = skc / CK;
        char* const sa = smem;                               // [2][256 rows]
        char* const sw = smem + 2 * 256 * PITCH;             // [2][BM rows]
        int gp[XR];
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int r = (tid >> 2) + RPP * i;
            const int od = od0 + (r >> (gLGTW + gLGTH)), oh = oh0 + ((r >> gLGTW) & (gTH - 1)), ow = ow0 + (r & (gTW - 1));
            const bool ok = GEO || (od < p.Do && oh < p.Ho && ow < p.Wo);
            gp[i] = ok ? ((n * p.Do + od) * p.Ho + oh) * p.Wo + ow : -1;
        }
        int cb[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
            cb[j] = tile_position16(2 * (wpos * 2 + j), lane & 15, gTW, gPAIR) * PITCH + 16 * (lane >> 4);
        const unsigned skw_voff = (unsigned)(tid >> 2) * (unsigned)skc * (unsigned)sizeof(T) + (unsigned)piece * 16u;
        const char* const skw0 = p.sk_w + (size_t)co0 * skc * sizeof(T);
        uint4 xr[XR], wr0 = make_uint4(0u, 0u, 0u, 0u), wr1 = make_uint4(0u, 0u, 0u, 0u);
        auto sk_load = [&](int c) {
            const int ch = c * CK;
            const char* src;
            int cs, csrc;
            if (ch < p.sk_c1) { src = p.sk_x1; cs = p.sk_c1; csrc = ch; } else { src = p.sk_x2; cs = p.sk_c2; csrc = ch - p.sk_c1; }
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int ps = (GEO || gp[i] > 0) ? gp[i] : 0;
                xr[i] = *reinterpret_cast<const uint4*>(src + ((size_t)ps * cs + csrc) * sizeof(T) + piece * 16);
            }
            const char* ws_ = skw0 + (size_t)c * 64;
            if (w_active) wr0 = *reinterpret_cast<const uint4*>(ws_ + skw_voff);
            if constexpr (WROWS == 2) wr1 = *reinterpret_cast<const uint4*>(ws_ + (size_t)RPP * skc * sizeof(T) + skw_voff);
        };
        auto sk_store = [&](int slot) {
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                const int r = (tid >> 2) + RPP * i;
                *reinterpret_cast<uint4*>(sa + (slot * 256 + r) * PITCH + piece * 16) = (GEO || gp[i] >= 0) ? xr[i] : make_uint4(0u, 0u, 0u, 0u);
            }
            char* const wd = sw + slot * BM * PITCH + w_dst0;
            if (w_active) *reinterpret_cast<uint4*>(wd) = wr0;
            if constexpr (WROWS == 2) *reinterpret_cast<uint4*>(wd + RPP * PITCH) = wr1;
        };
        auto sk_mm = [&](const u32x4_t (&fa)[2], const u32x4_t (&fb)[2], int tp, int jp) {
            f32x16_t& c = acc[tp][jp];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int q = 4 * (2 * tt + jj);
                    f32x4_t v = {c[q], c[q + 1], c[q + 2], c[q + 3]};
                    v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[tt]), __builtin_bit_cast(bf16x8_t, fb[jj]), v, 0, 0, 0);
                    c[q] = v[0]; c[q + 1] = v[1]; c[q + 2] = v[2]; c[q + 3] = v[3];
                }
        };
        sk_load(0);
        for (int c = 0; c < nsk; ++c) {
            const int slot = c & 1;
            sk_store(slot);                                  // (slot last read in iteration c - 2: every wave has passed the barrier of c - 1)
            if (c + 1 < nsk) sk_load(c + 1);
            __syncthreads();
            u32x4_t fa01[2], fa23[2], fb0[2], fb1[2];
            const char* const wA = sw + slot * BM * PITCH + a_off;
            const char* const xB = sa + slot * 256 * PITCH;
            fa01[0] = *reinterpret_cast<const u32x4_t*>(wA);
            fa01[1] = *reinterpret_cast<const u32x4_t*>(wA + PITCH);
            fb0[0] = *reinterpret_cast<const u32x4_t*>(xB + cb[0]);
            fb0[1] = *reinterpret_cast<const u32x4_t*>(xB + cb[0] + PITCH);
            fb1[0] = *reinterpret_cast<const u32x4_t*>(xB + cb[1]);
            fb1[1] = *reinterpret_cast<const u32x4_t*>(xB + cb[1] + PITCH);
            fa23[0] = *reinterpret_cast<const u32x4_t*>(wA + 32 * PITCH);
            fa23[1] = *reinterpret_cast<const u32x4_t*>(wA + 33 * PITCH);
            sk_mm(fa01, fb0, 0, 0);
            sk_mm(fa01, fb1, 0, 1);
            sk_mm(fa23, fb0, 1, 0);
            sk_mm(fa23, fb1, 1, 1);
        }
        __syncthreads();                                     // the tap loop's prologue overwrites these LDS bytes
    }
    const char* wl = w_src0;
    if constexpr (NT != 1) {
    if constexpr (PIPE) {
        RHO_LOAD_W(0, 0, 0);
        RHO_LOAD_W(1, 0, 1);
        RHO_LOAD_W(2, 0, 2);
        RHO_STORE_W(0, 0);
        RHO_STORE_W(1, 1);
        if constexpr (DS > 2) RHO_STORE_W(2, 2);
#pragma unroll
        for (int q = 3; q < LD; ++q) RHO_LOAD_W(q % 3, min(q / NS, nck - 1), q % NS);
#pragma unroll
        for (int q = 3; q < DS; ++q) RHO_STORE_W(q % RS, q % 3);
        wl = w_src0 + (size_t)(LD % NS) * w_tap_stride + (size_t)min(LD / NS, nck - 1) * 64;   // step LD: fetched at tap 0 of chunk 0
    } else {
        // steps 0 .. PD-1 of chunk 0 in flight (PD <= NS), step 0 landed in LDS slot 0
#pragma unroll
        for (int i = 0; i < PD; ++i) RHO_LOAD_W(i, 0, i);
        RHO_STORE_W(0, 0);
    }
    int cur = 0;

    // Halo staging.  HPF (one workgroup per CU, nothing else to hide behind): the NEXT chunk's global loads are
    // issued into registers while the last taps of the current chunk run on the matrix cores, and only the
    // prologue + LDS write happens between chunks (issue-early / write-late).  Otherwise (>= 2 workgroups per CU
    // overlap each other) load and write in small batches to keep the register footprint down.
    constexpr bool HPF = (BM >= 128) && (MAXP * RPP <= 640);
    constexpr int TPF = (NT > 6) ? NT - 6 : 0;        // tap at which the next chunk's loads are issued
    uint4 hv[HPF ? MAXP : 1];
    auto halo_src = [&](int ck_, const char*& src, int& cs, int& csrc) {
        const int c = (ck_lo + ck_) * CK;
        if (c < p.c1) { src = p.x1; cs = p.c1; csrc = c; } else { src = p.x2; cs = p.c2; csrc = c - p.c1; }
    };
#define RHO_HALO_LOAD(ck_)                                                                                         \
    do {                                                                                                          \
        const char* src_; int cs_, csrc_;                                                                         \
        halo_src(ck_, src_, cs_, csrc_);                                                                          \
        /* branch-free (padding lanes read position 0 and are zeroed at write time): loads under an exec mask */  \
        /* are invisible to the compiler's counted vmcnt waits, which would then drain them immediately        */  \
        _Pragma("unroll") for (int i = 0; i < MAXP; ++i) {                                                        \
            const int ps_ = spos[i] > 0 ? spos[i] : 0;                                                            \
            hv[i] = *reinterpret_cast<const uint4*>(src_ + ((size_t)ps_ * cs_ + csrc_) * sizeof(T) + piece * 16); \
        }                                                                                                         \
    } while (0)
    if constexpr (HPF) RHO_HALO_LOAD(0);

    for (int ck = 0; ck < nck; ++ck) {
        if constexpr (M16) asm volatile("" : "+v"(w_voff));
        // ---- stage the halo tile of this channel chunk (previous chunk's reads are fenced by the
        //      barrier that closed its last tap)
        {
            const int c = (ck_lo + ck) * CK;
            if constexpr (GEO) {
                // Straight-line staging: the thread's prologue coefficients (its channel piece of this chunk) are read from LDS
                // once per chunk, every slot is loaded (padding slots read position 0), activated and then zeroed by a select - no
                // branch per slot, so the slots' SiLU chains interleave (conv32.h, "one exec-masked block per row").  The load
                // shape is the generic one: the whole halo early (HPF) or two batches of five.
                const bool has_pre = p.pre_a != nullptr;
                f32x2_t av[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}}, bv[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
                if (has_pre) {
                    const float* const ca = coef + c + piece * PE;
                    const float* const cb = ca + p.cin;
                    const float4 a0 = *reinterpret_cast<const float4*>(ca), a1 = *reinterpret_cast<const float4*>(ca + 4);
                    const float4 b0 = *reinterpret_cast<const float4*>(cb), b1 = *reinterpret_cast<const float4*>(cb + 4);
                    av[0] = f32x2_t{a0.x, a0.y}; av[1] = f32x2_t{a0.z, a0.w}; av[2] = f32x2_t{a1.x, a1.y}; av[3] = f32x2_t{a1.z, a1.w};
                    bv[0] = f32x2_t{b0.x, b0.y}; bv[1] = f32x2_t{b0.z, b0.w}; bv[2] = f32x2_t{b1.x, b1.y}; bv[3] = f32x2_t{b1.z, b1.w};
                }
                const char* src = nullptr;
                int cs = 0, csrc = 0;
                if constexpr (!HPF) halo_src(ck, src, cs, csrc);
                constexpr int NB = HPF ? MAXP : 5;           // slots per batch (divides MAXP)
                static_assert(MAXP % NB == 0, "whole batches");
#pragma unroll
                for (int i0 = 0; i0 < MAXP; i0 += NB) {
                    uint4 v[NB];
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        if constexpr (HPF) {
                            v[q] = hv[i0 + q];
                        } else {
                            const int ps = spos[i0 + q] > 0 ? spos[i0 + q] : 0;
                            v[q] = *reinterpret_cast<const uint4*>(src + ((size_t)ps * cs + csrc) * sizeof(T) + piece * 16);
                        }
                    }
                    if (has_pre) {                           // (wave-uniform, as is pre_silu: one branch per batch)
                        if (p.pre_silu) {
#pragma unroll
                            for (int q = 0; q < NB; ++q) v[q] = apply_pre_regs<true>(v[q], av, bv);
                        } else {
#pragma unroll
                            for (int q = 0; q < NB; ++q) v[q] = apply_pre_regs<false>(v[q], av, bv);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        const int i = i0 + q;
                        const bool in = spos[i] >= 0;
                        const uint4 u = make_uint4(in ? v[q].x : 0u, in ? v[q].y : 0u, in ? v[q].z : 0u, in ? v[q].w : 0u);
                        const int hp = (tid >> 2) + RPP * i;
                        if (i < MAXP - 1 || last_in) *reinterpret_cast<uint4*>(halo + hp * PITCH + piece * 16) = u;
                    }
                }
            } else if constexpr (HPF) {
#pragma unroll
                for (int i = 0; i < MAXP; ++i) {
                    if (spos[i] != -2) {
                        uint4 u = spos[i] >= 0 ? hv[i] : make_uint4(0u, 0u, 0u, 0u);
                        if (p.pre_a != nullptr && spos[i] >= 0) {
                            if (KD == 3 && coef != nullptr) {
                                u = apply_pre<T>(u, coef + c + piece * PE, coef + p.cin + c + piece * PE, p.pre_silu);
                            } else {
                                const int smp = (KD == 3) ? n : ssmp[(KD == 3) ? 0 : i];
                                const size_t co = (size_t)smp * p.cin + c + piece * PE;
                                u = apply_pre<T>(u, p.pre_a + co, p.pre_b + co, p.pre_silu);
                            }
                        }
                        const int hp = (tid >> 2) + RPP * i;
                        *reinterpret_cast<uint4*>(halo + hp * PITCH + piece * 16) = u;
                    }
                }
            } else {
                const char* src;
                int cs, csrc;
                halo_src(ck, src, cs, csrc);
#ifdef RHO_PROBE_GB10   /* probe build: the whole small halo (10 pieces) in one batch - one exposed load latency per chunk instead of two */
                constexpr int GB = (MAXP == 10) ? 10 : ((MAXP % 7 == 0) ? 7 : 5);
#else
                constexpr int GB = (MAXP % 7 == 0) ? 7 : 5;  // loads in flight per batch (divides MAXP)
#endif
#pragma unroll
                for (int i0 = 0; i0 < MAXP; i0 += GB) {
                    uint4 v[GB];
#pragma unroll
                    for (int q = 0; q < GB; ++q) {
                        const int i = i0 + q;
                        if (i < MAXP) {
                            v[q] = make_uint4(0u, 0u, 0u, 0u);
                            if (spos[i] >= 0)
                                v[q] = *reinterpret_cast<const uint4*>(src + ((size_t)spos[i] * cs + csrc) * sizeof(T) + piece * 16);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < GB; ++q) {
                        const int i = i0 + q;
                        if (i < MAXP) {
                            if (spos[i] != -2) {
                                uint4 u = v[q];
                                if (p.pre_a != nullptr && spos[i] >= 0) {
                                    if (KD == 3 && coef != nullptr) {
                                        u = apply_pre<T>(u, coef + c + piece * PE, coef + p.cin + c + piece * PE, p.pre_silu);
                                    } else {
                                        const int smp = (KD == 3) ? n : ssmp[(KD == 3) ? 0 : i];
                                        const size_t co = (size_t)smp * p.cin + c + piece * PE;
                                        u = apply_pre<T>(u, p.pre_a + co, p.pre_b + co, p.pre_silu);
                                    }
                                }
                                const int hp = (tid >> 2) + RPP * i;
                                *reinterpret_cast<uint4*>(halo + hp * PITCH + piece * 16) = u;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();

        if constexpr (PIPE && M16) {
            // 16 MFMAs (16x16x32) per tap in four phases of 2 x 2 tiles: (a01,F) (a01,S) (a23,S) (a23,F), where F / S are the
            // two column-tile pairs in an order that alternates with the tap.  Five 2-fragment register sets (a01, a23, bS and
            // bF[2]); every set is read from LDS two phases (>= 128 MFMA cycles) before its first use:
            //   phase 0 reads a23 (phase 2) | 1 reads the next tap's F | 2 reads the next tap's a01 | 3 reads the next tap's S.
            static_assert(MT == 2, "M16 tap schedule: 64 couts per wave");
            typedef float f32x4_t __attribute__((ext_vector_type(4)));
            typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
            u32x4_t a01[2], a23[2], bS[2][2], bF[2][2];
            auto rdA = [&](int slot, int tp, u32x4_t (&fa)[2]) {
                const char* w = wbuf + (size_t)slot * SLOT + a_off + tp * 32 * PITCH;
                fa[0] = *reinterpret_cast<const u32x4_t*>(w);
                fa[1] = *reinterpret_cast<const u32x4_t*>(w + PITCH);
            };
            // stride 1, no upsampling (M16): a tap shifts every lane by the same (kd * IH * IW + kh * IW + kw) rows - a scalar
            // added to one per-lane base per column pair, instead of 27 x 2 per-lane offsets kept in VGPRs across the chunk loop
            const int bbase[2] = {offd[0] + offh[0][0] + offw[0][0], offd[1] + offh[1][0] + offw[1][0]};
            // (opaque per chunk: computed by the scalar ALU at each use - hoisted out of the chunk loop the 27 offsets and the 27
            //  weight bases overflow the SGPR file and come back as v_readlane per use)
            // (GEO: the 27 offsets are constants below 2^16 and ride in the offset field of the ds_read instructions)
            int ihs = gIH, iws = gIW;
            if constexpr (!GEO) asm volatile("" : "+s"(ihs), "+s"(iws));
            auto rdB = [&](int tap, int jp, u32x4_t (&fb)[2]) {
                const int kd = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
                const char* b = halo + (bbase[jp] + ((kd * ihs + kh) * iws + kw) * PITCH);
                fb[0] = *reinterpret_cast<const u32x4_t*>(b);
                fb[1] = *reinterpret_cast<const u32x4_t*>(b + PITCH);
            };
            auto mm = [&](const u32x4_t (&fa)[2], const u32x4_t (&fb)[2], int tp, int jp) {   // tp, jp: compile-time after unrolling
                f32x16_t& c = acc[tp][jp];
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int q = 4 * (2 * tt + jj);
                        f32x4_t v = {c[q], c[q + 1], c[q + 2], c[q + 3]};
                        v = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[tt]), __builtin_bit_cast(bf16x8_t, fb[jj]),
                                                                    v, 0, 0, 0);
                        c[q] = v[0]; c[q + 1] = v[1]; c[q + 2] = v[2]; c[q + 3] = v[3];
                    }
            };
            rdA(0, 0, a01);
            rdB(0, 0, bF[0]);
            rdB(0, 1, bS[0]);
            // MFMA intrinsics carry no chain: instruction selection gathers a tap's 16 MFMAs and the scheduler then bursts the
            // fragment reads right before the barrier's lgkmcnt(0).  An empty volatile asm that passes the fragments a group is
            // about to use pins the order: the group's MFMAs come after it (data), the reads issued before it stay before it
            // (memory clobber) - so every read is issued two groups (>= 128 MFMA cycles) ahead of its first use.
#define RHO_PHASE() __builtin_amdgcn_sched_barrier(0)
#define RHO_FENCE(A_, B_)                                                                                             \
    do {                                                                                                              \
        asm volatile("" : "+v"(A_[0]), "+v"(A_[1]), "+v"(B_[0]), "+v"(B_[1]) : : "memory");                           \
        __builtin_amdgcn_sched_barrier(0);                                                                            \
    } while (0)
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                RHO_LOAD_WP((st + LD) % 3, st);
                if constexpr (HPF) {
                    if (st == TPF) {
                        __builtin_amdgcn_sched_barrier(0);     // keep the halo loads younger than the weight fetch above
                        RHO_HALO_LOAD(min(ck + 1, nck - 1));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                const int slot = st % RS, nslot = (st + 1) % RS;
                const bool more = st + 1 < NS;                 // next chunk's first tap: after its halo is staged
                const int jf = st & 1, js = jf ^ 1;            // column-tile pair of F / S in this tap (swapped in the next)
                const int fc = st & 1, fn = fc ^ 1;            // fragment buffers of this / the next tap
                // group 0: this tap's second cout pair
                rdA(slot, 1, a23);
                RHO_FENCE(a01, bF[fc]);
                mm(a01, bF[fc], 0, jf);
                // group 1
                if (more) rdB(st + 1, js, bF[fn]);
                RHO_FENCE(a01, bS[fc]);
                mm(a01, bS[fc], 0, js);
                // group 2: the last fragment reads of the tap, two groups (>= 128 MFMA cycles) before a barrier's lgkmcnt(0)
                if (more) rdA(nslot, 0, a01);
                if (more) rdB(st + 1, jf, bS[fn]);
                RHO_FENCE(a23, bS[fc]);
                mm(a23, bS[fc], 1, js);
                // group 3: the LDS weight store (fetched two taps ago; late in the tap its vmcnt wait is free)
                RHO_STORE_W((st + DS) % RS, (st + DS) % 3);
                RHO_FENCE(a23, bF[fc]);
                mm(a23, bF[fc], 1, jf);
                if (st % GB == GB - 1) __syncthreads();
                RHO_PHASE();
            }
        } else if constexpr (PIPE) {
            // fragments: X = k-half 0 of the current step (already in flight), Y = k-half 1
            uint4 xa[MT], xb[2], ya[MT], yb[2];
            auto frag_reads = [&](int tap, int slot, int s_, uint4 (&fa)[MT], uint4 (&fb)[2]) {
                const int kd = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
                const char* wcur = wbuf + (size_t)slot * SLOT + a_off + 32 * s_;
                const int dtap = kd * p.IH * p.IW * PITCH + 32 * s_;
                fb[0] = *reinterpret_cast<const uint4*>(halo + (dtap + offd[0] + offh[0][kh] + offw[0][kw]));
                fb[1] = *reinterpret_cast<const uint4*>(halo + (dtap + offd[1] + offh[1][kh] + offw[1][kw]));
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) fa[mi] = *reinterpret_cast<const uint4*>(wcur + mi * 32 * PITCH);
            };
            frag_reads(0, 0, 0, xa, xb);
#pragma unroll
            for (int st = 0; st < NS; ++st) {
                {   // step st + LD -> register set (st + LD) % 3 (its previous tile went to LDS at the end of step st - 1);
                    // unconditional and clamped, so the loads in flight are a static count (counted vmcnt, no drain)
                    const int nst = (st + LD) % NS;
                    const int nckk = min(ck + (st + LD) / NS, nck - 1);
                    RHO_LOAD_W((st + LD) % 3, nckk, nst);
                }
                if constexpr (HPF) {
                    if (st == TPF) {
                        __builtin_amdgcn_sched_barrier(0);     // keep the halo loads younger than the weight fetch above
                        RHO_HALO_LOAD(min(ck + 1, nck - 1));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                frag_reads(st, st % RS, 1, ya, yb);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    mma_step<T>(xa[mi], xb[0], acc[mi][0]);
                    mma_step<T>(xa[mi], xb[1], acc[mi][1]);
                }
                if (st + 1 < NS) frag_reads(st + 1, (st + 1) % RS, 0, xa, xb);  // next chunk's first step: after its halo is staged
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    mma_step<T>(ya[mi], yb[0], acc[mi][0]);
                    mma_step<T>(ya[mi], yb[1], acc[mi][1]);
                }
                RHO_STORE_W((st + DS) % RS, (st + DS) % 3);    // step st + DS (slot last read in step st + DS - RS)
                if (st % GB == GB - 1) __syncthreads();
            }
        } else {
            // ---- all taps out of the resident tile, G taps per barrier step
    #pragma unroll
            for (int st = 0; st < NS; ++st) {
                const bool has_next = !(ck == nck - 1 && st == NS - 1);
                // step q = ck*NS + st: its register set (st % PD) went to LDS one step ago -> refill it with step q + PD
                // now, so the fetch has PD steps of MFMA work to hide under; at the end of this step, step q + 1 (fetched
                // PD - 1 steps ago) is handed to the other LDS slot.  Unconditional (past the end it re-reads the last
                // chunk's tiles) so that the number of loads in flight is static and the compiler waits with a counted
                // vmcnt instead of draining to 0.
                {
                    const int nst = (st + PD < NS) ? st + PD : st + PD - NS;
                    const int nckk = (st + PD < NS) ? ck : min(ck + 1, nck - 1);
                    RHO_LOAD_W(st % PD, nckk, nst);
                }
                // next chunk's halo: issued AFTER this step's weight fetch (vmcnt retires in order, so the counted waits
                // for the next PD-1 steps' weights do not drain these loads) and unconditionally (static count)
                if constexpr (HPF) {
                    if (st * G == TPF) {
                        __builtin_amdgcn_sched_barrier(0);     // keep the halo loads younger than the weight fetch above
                        RHO_HALO_LOAD(min(ck + 1, nck - 1));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
    #pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int tap = st * G + g;
                    const int kd = tap / (KH * KW), kh = (tap / KW) % KH, kw = tap % KW;
                    const char* wcur = wbuf + (size_t)cur * SLOT + g * BM * PITCH + a_off;
                    const int dtap = kd * p.IH * p.IW * PITCH;
                    const char* b0p = halo + (dtap + offd[0] + offh[0][kh] + offw[0][kw]);
                    const char* b1p = halo + (dtap + offd[1] + offh[1][kh] + offw[1][kw]);
    #pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const uint4 b0 = *reinterpret_cast<const uint4*>(b0p + 32 * s);
                        const uint4 b1 = *reinterpret_cast<const uint4*>(b1p + 32 * s);
    #pragma unroll
                        for (int mi = 0; mi < MT; ++mi) {
                            const uint4 a = *reinterpret_cast<const uint4*>(wcur + mi * 32 * PITCH + 32 * s);
                            mma_step<T>(a, b0, acc[mi][0]);
                            mma_step<T>(a, b1, acc[mi][1]);
                        }
                    }
                }
                if (has_next) RHO_STORE_W(cur ^ 1, (st + 1) % PD);
                __syncthreads();
                cur ^= 1;
            }
            }
    }

    } else {
        // ---- 1x1x1: a GEMM over channel chunks.  There is no halo and one tap per chunk, so the generic path (stage a
        // chunk, barrier, 8 MFMAs, barrier) exposed one global-load latency per chunk (0.88 ms for the 512 -> 1536 qkv
        // projection, 0.2 TFLOP).  Here chunk c + DX is fetched into a register ring while chunk c runs, activations and
        // weights are double-buffered in LDS, and one barrier per chunk orders both the hand-over and the slot reuse.
        constexpr int XS = (256 + RPP - 1) / RPP;          // activation rows per thread (the tile is 256 linear positions)
        constexpr int DX = (NW == 8) ? 4 : 2;              // chunks in flight (4-wave variants: two workgroups per CU share the registers)
        constexpr int HSLOT = 256 * PITCH;
        char* const wb2 = smem + 2 * HSLOT;                // [2][BM rows]
        uint4 xq[DX][XS], wx0[DX], wx1[DX];
#pragma unroll
        for (int i = 0; i < DX; ++i) wx0[i] = wx1[i] = make_uint4(0u, 0u, 0u, 0u);
        auto issue = [&](auto SET, int ckk) {
            constexpr int S_ = decltype(SET)::value;
            const int cc = min(ckk, nck - 1);              // clamped: static number of loads in flight (counted vmcnt)
            const int c = (ck_lo + cc) * CK;
            const char* src;
            int cs, csrc;
            if (c < p.c1) { src = p.x1; cs = p.c1; csrc = c; } else { src = p.x2; cs = p.c2; csrc = c - p.c1; }
#pragma unroll
            for (int i = 0; i < XS; ++i) {
                const int ps = spos[i] > 0 ? spos[i] : 0;
                xq[S_][i] = *reinterpret_cast<const uint4*>(src + ((size_t)ps * cs + csrc) * sizeof(T) + piece * 16);
            }
            const char* ws = w_src0 + (size_t)cc * 64;
            if (w_active) wx0[S_] = *reinterpret_cast<const uint4*>(ws + w_voff);
            if constexpr (WROWS == 2) wx1[S_] = *reinterpret_cast<const uint4*>(ws + RPP * wrow_bytes + w_voff);
        };
        // The folded GroupNorm affine of the prologue: fetched from global memory inside the chunk loop it would be the
        // youngest load in flight at every hand-over, and waiting for it (vmcnt is in-order) drains the whole register
        // ring: one exposed memory latency per chunk (qkv projection: 0.8 ms at 260 TFLOP/s).  A tile that lies in one
        // sample (block-uniform test) stages that sample's coefficients in LDS once; tiles straddling samples keep the
        // global fetch.
        float* const coef = reinterpret_cast<float*>(smem + 2 * HSLOT + 2 * BM * PITCH);   // [2][nck * CK]
        const bool has_pre = p.pre_a != nullptr;
        bool coef_lds = false;
        if (has_pre) {
            const int pos0 = ((n * p.D + gd_base) * p.Hs + gh_base) * p.Ws + gw_base;     // the tile's first position
            const int smp_ref = (int)((long long)pos0 / p.S_in);
            bool mine = !(p.up_h | p.up_w | p.zs_h | p.zs_w) && p.sh == 1 && p.sw == 1;
#pragma unroll
            for (int i = 0; i < XS; ++i)
                if (spos[i] >= 0 && ssmp[i] != smp_ref) mine = false;
            coef_lds = __syncthreads_and(mine ? 1 : 0) != 0;
            if (coef_lds) {
                const int cpad = nck * CK, cbase = ck_lo * CK;          // (this launch's chunks: all of them unless k-split)
                for (int i = tid; i < cpad; i += NTHR) {
                    const bool in = cbase + i < p.cin;
                    coef[i] = in ? p.pre_a[(size_t)smp_ref * p.cin + cbase + i] : 0.0f;
                    coef[cpad + i] = in ? p.pre_b[(size_t)smp_ref * p.cin + cbase + i] : 0.0f;
                }
                __syncthreads();
            }
        }
        auto land = [&](auto SET, int ck, auto LDSCOEF) {   // registers -> LDS slot ck & 1 (prologue applied)
            constexpr int S_ = decltype(SET)::value;
            const int c = ck * CK;
            char* const hs = smem + (ck & 1) * HSLOT;
#pragma unroll
            for (int i = 0; i < XS; ++i) {
                if (spos[i] != -2) {
                    uint4 u = spos[i] >= 0 ? xq[S_][i] : make_uint4(0u, 0u, 0u, 0u);
                    if (has_pre && spos[i] >= 0) {
                        if constexpr (decltype(LDSCOEF)::value) {
                            const float* const ca = coef + c + piece * PE;
                            u = apply_pre<T>(u, ca, ca + nck * CK, p.pre_silu);
                        } else {
                            const size_t co = (size_t)ssmp[i] * p.cin + ck_lo * CK + c + piece * PE;
                            u = apply_pre<T>(u, p.pre_a + co, p.pre_b + co, p.pre_silu);
                        }
                    }
                    const int hp = (tid >> 2) + RPP * i;
                    *reinterpret_cast<uint4*>(hs + hp * PITCH + piece * 16) = u;
                }
            }
            char* const wd = wb2 + (ck & 1) * BM * PITCH + w_dst0;
            if (w_active) *reinterpret_cast<uint4*>(wd) = wx0[S_];
            if constexpr (WROWS == 2) *reinterpret_cast<uint4*>(wd + RPP * PITCH) = wx1[S_];
        };
        auto compute = [&](int ck) {
            const char* const hs = smem + (ck & 1) * HSLOT;
            const char* const wcur = wb2 + (ck & 1) * BM * PITCH + a_off;
            const char* b0p = hs + (offd[0] + offh[0][0] + offw[0][0]);
            const char* b1p = hs + (offd[1] + offh[1][0] + offw[1][0]);
#pragma unroll
            for (int s_ = 0; s_ < 2; ++s_) {
                const uint4 b0 = *reinterpret_cast<const uint4*>(b0p + 32 * s_);
                const uint4 b1 = *reinterpret_cast<const uint4*>(b1p + 32 * s_);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const uint4 a = *reinterpret_cast<const uint4*>(wcur + mi * 32 * PITCH + 32 * s_);
                    mma_step<T>(a, b0, acc[mi][0]);
                    mma_step<T>(a, b1, acc[mi][1]);
                }
            }
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 = std::integral_constant<int, 3>;
        issue(I0{}, 0); issue(I1{}, 1);
        if constexpr (DX == 4) { issue(I2{}, 2); issue(I3{}, 3); }
        // Groups of DX chunks run without a branch (same number of loads in flight on every path: the hand-over waits are
        // counted, `vmcnt(9)`-style, instead of draining); the last nck % DX chunks have nothing left to fetch.
#define RHO_ONE_STEP(K_, ISET, LC)                                                                  \
        land(ISET{}, ck0 + K_, LC{});                                                               \
        __syncthreads();                                                                            \
        issue(ISET{}, ck0 + K_ + DX);                                                               \
        compute(ck0 + K_);
#define RHO_ONE_TAIL(K_, ISET, LC)                                                                  \
        if (ck0 + K_ < nck) {                                                                       \
            land(ISET{}, ck0 + K_, LC{});                                                           \
            __syncthreads();                                                                        \
            compute(ck0 + K_);                                                                      \
        }
        if (!has_pre || coef_lds) {
            int ck0 = 0;
            for (; ck0 + DX <= nck; ck0 += DX) {
                RHO_ONE_STEP(0, I0, std::true_type)
                RHO_ONE_STEP(1, I1, std::true_type)
                if constexpr (DX == 4) {
                    RHO_ONE_STEP(2, I2, std::true_type)
                    RHO_ONE_STEP(3, I3, std::true_type)
                }
            }
            RHO_ONE_TAIL(0, I0, std::true_type)
            if constexpr (DX == 4) {
                RHO_ONE_TAIL(1, I1, std::true_type)
                RHO_ONE_TAIL(2, I2, std::true_type)
            }
        } else {
            int ck0 = 0;
            for (; ck0 + DX <= nck; ck0 += DX) {
                RHO_ONE_STEP(0, I0, std::false_type)
                RHO_ONE_STEP(1, I1, std::false_type)
                if constexpr (DX == 4) {
                    RHO_ONE_STEP(2, I2, std::false_type)
                    RHO_ONE_STEP(3, I3, std::false_type)
                }
            }
            RHO_ONE_TAIL(0, I0, std::false_type)
            if constexpr (DX == 4) {
                RHO_ONE_TAIL(1, I1, std::false_type)
                RHO_ONE_TAIL(2, I2, std::false_type)
            }
        }
#undef RHO_ONE_STEP
#undef RHO_ONE_TAIL
    }
#undef RHO_PHASE
#undef RHO_FENCE
#undef RHO_LOAD_W
#undef RHO_LOAD_WP
#undef RHO_STORE_W
#undef RHO_HALO_LOAD
    // The epilogue reads its parameters (output / residual / bias / statistics pointers, output geometry) from the kernel-argument
    // segment again instead of from `p`: held in SGPRs across the tap loop they pushed the kernel past the scalar register file
    // (120 spills to VGPR lanes: ~300 v_readlane per tile in the set-up and 4 per epilogue item, all VALU issue slots).  The asm
    // keeps the reloads below the loop.
    const __attribute__((address_space(4))) ConvK* qp = (const __attribute__((address_space(4))) ConvK*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(qp));
    const __attribute__((address_space(4))) ConvK& q = *qp;
    // ---- epilogue: lane holds, for position column (lane&31) of tile j, channels
    //      co0 + 32*mi + 8*rg + 4*half + {0,1,2,3}  in acc[mi][j][4*rg + {0..3}]
    if (splitk) {
        // k-split launch: the raw fp32 partial sums of this split go to its slab ([launch positions][coutp]; the host only splits
        // launches whose outputs are all channels-last); bias, residuals and the rounding happen once, in k_splitk_reduce
        float* const slab = q.slab + (size_t)blockIdx.z * q.slab_stride;
#pragma unroll
        for (int jx = 0; jx < (M16 ? 4 : 2); ++jx) {
            const int pp = M16 ? tile_position16(wpos * 4 + jx, lane & 15, q.TW, q.pair_lg) : tile_position(wpos * 2 + jx, lane & 31, q.TW, q.pair_lg);
            const int pw = pp & (q.TW - 1);
            const int ph = (pp >> q.lgTW) & (q.TH - 1);
            const int pd = pp >> (q.lgTW + q.lgTH);
            const int od = od0 + pd, oh = oh0 + ph, ow = ow0 + pw;
            if (od >= q.Do || oh >= q.Ho || ow >= q.Wo) continue;
            const size_t L = ((size_t)od * q.Ho + oh) * q.Wo + ow;
            const int j = M16 ? (jx >> 1) : jx;
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
                for (int rx = 0; rx < (M16 ? 2 : 4); ++rx) {
                    const int rg = M16 ? 2 * rx + (jx & 1) : rx;
                    const int co = M16 ? co0 + wco * (BM / WCO) + 16 * (2 * mi + rx) + 4 * (lane >> 4)
                                       : co0 + wco * (BM / WCO) + mi * 32 + rg * 8 + half * 4;
                    *reinterpret_cast<float4*>(slab + L * q.coutp + co) =
                        make_float4(acc[mi][j][rg * 4 + 0], acc[mi][j][rg * 4 + 1], acc[mi][j][rg * 4 + 2], acc[mi][j][rg * 4 + 3]);
                }
            }
        }
        return;
    }
    // (round 4: the second channels-last region of a launch - the gradient of the second source of a concatenated input - takes the
    //  same transposed path when its width is whole 16-byte pieces: the fused GroupNorm-backward apply needs both regions here)
    const bool reg2 = q.y2_cl && co0 >= q.split && ((q.cout - q.split) % PE == 0);
    const bool cl_region = (co0 < q.split) || reg2;
    if (cl_region) {
        const int rw = reg2 ? q.cout - q.split : q.split;          // row width of this region's tensor
        const int rc0 = reg2 ? co0 - q.split : co0;                // first channel of this tile inside it
        char* const ry = reg2 ? q.y2 : q.y;
        const char* const rrp = reg2 ? q.res2 : q.res;
        const float* const radd = reg2 ? nullptr : q.res_add;
        // Channels-last output (every block of this launch region: BM divides split).  The accumulator layout gives a
        // lane 4 channels of one position, i.e. 8-byte stores (and residual loads) scattered over 32 rows per
        // instruction.  Transpose through LDS instead (the halo / weight space is free now): fp32 rows of BM channels,
        // 128 positions per pass, then every lane moves one 16-byte piece and the 16-byte pieces of a row are
        // consecutive lanes.  (Probe: without any epilogue the 64-cout layers run 23 % faster; the scattered form
        // also wrote 1.36x the algorithmic bytes.)
        constexpr int ROWB = BM * 4 + 16;                 // odd number of 16-byte slots: conflict-free column writes
        constexpr int PPR = BM / PE;                      // 16-byte output pieces per row
        static_assert(NTHR % PPR == 0, "a thread keeps one channel piece across its rows (statistics accumulators)");
        char* const stg = smem;
        float ssum[PE], ssq[PE];                          // GroupNorm partial sums of this thread's channel piece
#pragma unroll
        for (int e = 0; e < PE; ++e) ssum[e] = ssq[e] = 0.0f;
        {
            __syncthreads();                              // tap loop done with the LDS bytes reused here
            {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
                        for (int rg = 0; rg < 4; ++rg) {
                            // M16: group rg of acc[mi][j] = cout tile 2 * mi + (rg >> 1), column tile 2 * j + (rg & 1)
                            const int lr = M16 ? wpos * 64 + (2 * j + (rg & 1)) * 16 + (lane & 15) : wpos * 64 + j * 32 + (lane & 31);
                            const int cl = M16 ? wco * (BM / WCO) + 16 * (2 * mi + (rg >> 1)) + 4 * (lane >> 4)
                                               : wco * (BM / WCO) + mi * 32 + rg * 8 + half * 4;
                            *reinterpret_cast<float4*>(stg + lr * ROWB + cl * 4) =
                                make_float4(acc[mi][j][rg * 4 + 0], acc[mi][j][rg * 4 + 1], acc[mi][j][rg * 4 + 2], acc[mi][j][rg * 4 + 3]);
                        }
                }
            }
            // Item k of this thread: row tid / PPR + k * (NTHR / PPR), 16-byte channel piece tid % PPR.  Output offsets and
            // the residual loads are issued BEFORE the barrier that publishes the staged rows: their latency runs under the
            // barrier and the LDS reads instead of after them (one exposed global latency per tile otherwise).
            constexpr int NIT = 256 * PPR / NTHR;
            static_assert(256 * PPR % NTHR == 0, "whole items per thread");
            int eoff[NIT];                                   // output position (the host guarantees < 2^31 positions), -1 = outside
            uint4 rres[GNA ? 1 : NIT];
            uint4 gx[NIT];                                  // gnb: this thread's piece of the forward input at its output positions
            float bia[PE];                                  // bias (+ the per-sample additive term, 3-D: one sample per tile)
            float gna[PE], gnb[PE];                         // gnb: folded affine of the forward prologue, this thread's channels
            const bool gnb_on = q.gnb_x1 != nullptr;
            // gna: the GroupNorm backward apply of this thread's channels rides in the store loop (rho_conv_desc.gna_*)
            const bool gna_on = GNA && q.gna_g != nullptr;
            uint4 gg[GNA ? NIT : 1];
            float gca[GNA ? PE : 1], gcp[GNA ? PE : 1], gcq[GNA ? PE : 1];
            {
                const int piece = tid % PPR;
                const int gco = co0 + piece * PE;           // the piece lies in one concat source (widths are multiples of 32)
                const bool g_first = gco < q.gnb_c1;
                const char* const gsrc = g_first ? q.gnb_x1 : q.gnb_x2;
                // (statistics: one tensor of `split` channels; apply: the concat of both regions, cout channels)
                const int gC = gna_on ? q.cout : q.split;
                const int gcs = g_first ? q.gnb_c1 : gC - q.gnb_c1, gch = g_first ? gco : gco - q.gnb_c1;
                if (gnb_on) {
                    const int nsg = GEO ? n : n + bt / q.tps;   // the tile's sample (statistics are only fused for one-sample tiles)
#pragma unroll
                    for (int e = 0; e < PE; ++e) {
                        gna[e] = q.gnb_a[(size_t)nsg * gC + gco + e];
                        gnb[e] = q.gnb_b[(size_t)nsg * gC + gco + e];
                    }
                    if constexpr (GNA) {
                        const int cpg = gC / 32;
#pragma unroll
                        for (int e = 0; e < PE; ++e) {
                            const int ce = (gco + e < gC) ? gco + e : gC - 1;        // (padding pieces of the last tile: never stored)
                            gca[e] = q.gna_cA[(size_t)nsg * gC + ce];
                            gcp[e] = q.gna_cP[(size_t)nsg * 32 + ce / cpg];
                            gcq[e] = q.gna_cQ[(size_t)nsg * 32 + ce / cpg];
                        }
                    }
                }
#pragma unroll
                for (int q4 = 0; q4 < PE / 4; ++q4) {
                    const float4 b4 = *reinterpret_cast<const float4*>(q.bias + co0 + piece * PE + q4 * 4);
                    bia[q4 * 4 + 0] = b4.x; bia[q4 * 4 + 1] = b4.y; bia[q4 * 4 + 2] = b4.z; bia[q4 * 4 + 3] = b4.w;
                    if constexpr (FSK) {
                        if (q.sk_bias != nullptr) {          // the folded skip convolution's own bias
                            const float4 s4 = *reinterpret_cast<const float4*>(q.sk_bias + co0 + piece * PE + q4 * 4);
                            bia[q4 * 4 + 0] += s4.x; bia[q4 * 4 + 1] += s4.y; bia[q4 * 4 + 2] += s4.z; bia[q4 * 4 + 3] += s4.w;
                        }
                    }
                    if constexpr (KD == 3) {
                        if (radd != nullptr) {
                            const float4 e = *reinterpret_cast<const float4*>(radd + (long long)n * q.res_add_stride + co0 + piece * PE + q4 * 4);
                            bia[q4 * 4 + 0] += e.x; bia[q4 * 4 + 1] += e.y; bia[q4 * 4 + 2] += e.z; bia[q4 * 4 + 3] += e.w;
                        }
                    }
                }
                // GEO: item k of a thread lies a compile-time offset from its item 0 (geo_item_delta), so an output row is the tile's
                // first row (scalar) + the thread's row inside the tile + a scalar per item; whole tiles: no bounds tests but the
                // channel-piece test of the second region, which does not depend on the item
                const bool pc_ok = rc0 + piece * PE + PE <= rw;     // (the last tile of the second region may reach past its tensor)
                int L0 = 0;
                if constexpr (GEO) {
                    static_assert(!GEO || (NTHR / PPR == 32 && geo_items_additive(NIT)), "GEO: item k = item 0 + a constant");
                    const int lr0 = tid / PPR;
                    const int pp0 = geo_row_position(lr0);
                    L0 = ((n * q.Do + od0 + (pp0 >> 6)) * q.Ho + oh0 + ((pp0 >> 3) & 7)) * q.Wo + ow0 + (pp0 & 7);
                }
#pragma unroll
                for (int k = 0; k < NIT; ++k) {
                    int L;
                    bool ok;
                    if constexpr (GEO) {
                        const int dk = geo_item_delta(k);
                        L = L0 + ((dk >> 6) * q.Ho + ((dk >> 3) & 7)) * q.Wo + (dk & 7);
                        ok = pc_ok;
                    } else {
                    const int lr = tid / PPR + k * (NTHR / PPR);
                    const int pp = M16 ? tile_position16((lr >> 6) * 4 + ((lr >> 4) & 3), lr & 15, q.TW, q.pair_lg)
                                       : tile_position((lr >> 6) * 2 + ((lr >> 5) & 1), lr & 31, q.TW, q.pair_lg);
                    const int pw = pp & (q.TW - 1);
                    const int ph = (pp >> q.lgTW) & (q.TH - 1);
                    const int pd = pp >> (q.lgTW + q.lgTH);
                    const int od = od0 + pd, oh = oh0 + ph, ow = ow0 + pw;
                    ok = od < q.Do && oh < q.Ho && ow < q.Wo && pc_ok;
                    L = ((n * q.Do + od) * q.Ho_out + (oh * q.oy_mul + q.oy_add)) * q.Wo_out + (ow * q.ox_mul + q.ox_add);
                    }
                    eoff[k] = (GEO || ok) ? L : -1;
                    if constexpr (!GNA) {
                        rres[k] = make_uint4(0u, 0u, 0u, 0u);
                        if (ok && rrp != nullptr)   // (32 x 32 -> 64-bit multiply: one v_mad_u64_u32 instead of a 64 x 64 sequence)
                            rres[k] = *reinterpret_cast<const uint4*>(rrp + ((size_t)(unsigned)L * (unsigned)rw + (unsigned)(rc0 + piece * PE)) * sizeof(T));
                    }
                    gx[k] = make_uint4(0u, 0u, 0u, 0u);
                    if (ok && gnb_on) gx[k] = *reinterpret_cast<const uint4*>(gsrc + ((size_t)(unsigned)L * (unsigned)gcs + (unsigned)gch) * sizeof(T));
                    if constexpr (GNA) {
                        gg[k] = make_uint4(0u, 0u, 0u, 0u);
                        if (ok) gg[k] = *reinterpret_cast<const uint4*>(q.gna_g + ((size_t)(unsigned)L * (unsigned)gC + (unsigned)gco) * sizeof(T));
                    }
                }
            }
            __syncthreads();
            if (!GEO || rc0 + (tid % PPR) * PE + PE <= rw) {
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                if (!GEO && eoff[k] < 0) continue;
                const int lr = tid / PPR + k * (NTHR / PPR), piece = tid % PPR;
                const int L = eoff[k];
                const int co = co0 + piece * PE;
                float v[PE];
#pragma unroll
                for (int q4 = 0; q4 < PE / 4; ++q4) {
                    const float4 a4 = *reinterpret_cast<const float4*>(stg + lr * ROWB + (piece * PE + q4 * 4) * 4);
                    v[q4 * 4 + 0] = a4.x + bia[q4 * 4 + 0]; v[q4 * 4 + 1] = a4.y + bia[q4 * 4 + 1];
                    v[q4 * 4 + 2] = a4.z + bia[q4 * 4 + 2]; v[q4 * 4 + 3] = a4.w + bia[q4 * 4 + 3];
                }
                if (KD != 3 && radd != nullptr) {
                    const long long ns = (long long)L / q.S_out;
#pragma unroll
                    for (int q4 = 0; q4 < PE / 4; ++q4) {
                        const float4 e = *reinterpret_cast<const float4*>(radd + ns * q.res_add_stride + co + q4 * 4);
                        v[q4 * 4 + 0] += e.x; v[q4 * 4 + 1] += e.y; v[q4 * 4 + 2] += e.z; v[q4 * 4 + 3] += e.w;
                    }
                }
                const size_t eo = (size_t)(unsigned)L * (unsigned)rw + (unsigned)(rc0 + piece * PE);
                if constexpr (GNA) {
                    // + cA * (g * act'(a x0 + b)) + cQ * x0 + cP: rho_gn_bwd_apply's term, from the operands that pass read
                    float xv[PE], gv[PE];
                    if constexpr (sizeof(T) == 2) {
                        const uint4 a_ = gx[k], b_ = gg[k];
                        xv[0] = __uint_as_float(a_.x << 16); xv[1] = __uint_as_float(a_.x & 0xFFFF0000u);
                        xv[2] = __uint_as_float(a_.y << 16); xv[3] = __uint_as_float(a_.y & 0xFFFF0000u);
                        xv[4] = __uint_as_float(a_.z << 16); xv[5] = __uint_as_float(a_.z & 0xFFFF0000u);
                        xv[6] = __uint_as_float(a_.w << 16); xv[7] = __uint_as_float(a_.w & 0xFFFF0000u);
                        gv[0] = __uint_as_float(b_.x << 16); gv[1] = __uint_as_float(b_.x & 0xFFFF0000u);
                        gv[2] = __uint_as_float(b_.y << 16); gv[3] = __uint_as_float(b_.y & 0xFFFF0000u);
                        gv[4] = __uint_as_float(b_.z << 16); gv[5] = __uint_as_float(b_.z & 0xFFFF0000u);
                        gv[6] = __uint_as_float(b_.w << 16); gv[7] = __uint_as_float(b_.w & 0xFFFF0000u);
                    } else {
                        const uint4 a_ = gx[k], b_ = gg[k];
                        xv[0] = __uint_as_float(a_.x); xv[1] = __uint_as_float(a_.y); xv[2] = __uint_as_float(a_.z); xv[3] = __uint_as_float(a_.w);
                        gv[0] = __uint_as_float(b_.x); gv[1] = __uint_as_float(b_.y); gv[2] = __uint_as_float(b_.z); gv[3] = __uint_as_float(b_.w);
                    }
#pragma unroll
                    for (int e = 0; e < PE; ++e) {
                        float gq = gv[e];
                        if (q.gnb_silu) gq *= dsilu_f(fmaf(gna[e], xv[e], gnb[e]));
                        v[e] += fmaf(gca[e], gq, fmaf(gcq[e], xv[e], gcp[e]));
                    }
                }
                if constexpr (sizeof(T) == 2) {
                    if (!GNA && rrp != nullptr) {
                        const uint4 r = rres[GNA ? 0 : k];
                        v[0] += __uint_as_float(r.x << 16); v[1] += __uint_as_float(r.x & 0xFFFF0000u);
                        v[2] += __uint_as_float(r.y << 16); v[3] += __uint_as_float(r.y & 0xFFFF0000u);
                        v[4] += __uint_as_float(r.z << 16); v[5] += __uint_as_float(r.z & 0xFFFF0000u);
                        v[6] += __uint_as_float(r.w << 16); v[7] += __uint_as_float(r.w & 0xFFFF0000u);
                    }
                    const uint4 o = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
                    {   // streaming store: the 1 GB outputs do not fit the caches, keep L2 for the halo re-reads (whole step -0.5 %)
                        typedef unsigned int u32x4_nt __attribute__((ext_vector_type(4)));
                        const u32x4_nt ov = {o.x, o.y, o.z, o.w};
                        __builtin_nontemporal_store(ov, reinterpret_cast<u32x4_nt*>(ry + eo * 2));
                    }
                    if (q.stats != nullptr) {             // statistics of the values as stored (what a reader would see)
                        v[0] = __uint_as_float(o.x << 16); v[1] = __uint_as_float(o.x & 0xFFFF0000u);
                        v[2] = __uint_as_float(o.y << 16); v[3] = __uint_as_float(o.y & 0xFFFF0000u);
                        v[4] = __uint_as_float(o.z << 16); v[5] = __uint_as_float(o.z & 0xFFFF0000u);
                        v[6] = __uint_as_float(o.w << 16); v[7] = __uint_as_float(o.w & 0xFFFF0000u);
                    }
                } else {
                    if (!GNA && rrp != nullptr) {
                        const uint4 r = rres[GNA ? 0 : k];
                        v[0] += __uint_as_float(r.x); v[1] += __uint_as_float(r.y); v[2] += __uint_as_float(r.z); v[3] += __uint_as_float(r.w);
                    }
                    *reinterpret_cast<float4*>(ry + eo * 4) = make_float4(v[0], v[1], v[2], v[3]);
                }
                if (q.stats != nullptr) {
                    if (gnb_on && !gna_on) {
                        // dgrad of a conv behind GroupNorm (+SiLU): v = d act(a x + b) as stored; the norm's backward needs the
                        // per-channel sums of dz = v * act'(a x + b) and of dz * x (rho_gn_bwd_finalize, fmt 1)
                        float xv[PE];
                        if constexpr (sizeof(T) == 2) {
                            const uint4 q = gx[k];
                            xv[0] = __uint_as_float(q.x << 16); xv[1] = __uint_as_float(q.x & 0xFFFF0000u);
                            xv[2] = __uint_as_float(q.y << 16); xv[3] = __uint_as_float(q.y & 0xFFFF0000u);
                            xv[4] = __uint_as_float(q.z << 16); xv[5] = __uint_as_float(q.z & 0xFFFF0000u);
                            xv[6] = __uint_as_float(q.w << 16); xv[7] = __uint_as_float(q.w & 0xFFFF0000u);
                        } else {
                            const uint4 q = gx[k];
                            xv[0] = __uint_as_float(q.x); xv[1] = __uint_as_float(q.y); xv[2] = __uint_as_float(q.z); xv[3] = __uint_as_float(q.w);
                        }
#pragma unroll
                        for (int e = 0; e < PE; ++e) {
                            float dz = v[e];
                            if (q.gnb_silu) dz *= dsilu_f(fmaf(gna[e], xv[e], gnb[e]));
                            ssum[e] += dz;
                            ssq[e] = fmaf(dz, xv[e], ssq[e]);
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < PE; ++e) {
                            ssum[e] += v[e];
                            ssq[e] = fmaf(v[e], v[e], ssq[e]);
                        }
                    }
                }
            }
            }
        }
        if (q.stats != nullptr) {
            // threads tid = piece (mod PPR) hold partials of the same channels: combine through LDS in thread order
            // (fixed order => reproducible), one (channel, statistic) per finishing thread
            __syncthreads();
            float* red = reinterpret_cast<float*>(stg);                     // [NTHR][2 * PE]
#pragma unroll
            for (int e = 0; e < PE; ++e) {
                red[tid * (2 * PE) + e] = ssum[e];
                red[tid * (2 * PE) + PE + e] = ssq[e];
            }
            __syncthreads();
            // (GEO: no phases, so a sample's tps tiles are this launch's own tiles)
            const int ns = GEO ? n : n + bt / q.tps, ts = GEO ? bt : bt % q.tps + q.stats_off;
            for (int item = tid; item < PPR * 2 * PE; item += NTHR) {
                const int piece = item / (2 * PE), e2 = item % (2 * PE);
                float accv = 0.0f;
                for (int q = 0; q < NTHR / PPR; ++q) accv += red[(q * PPR + piece) * (2 * PE) + e2];
                const int stat = e2 / PE, ch = co0 + piece * PE + (e2 % PE);
                q.stats[(((size_t)ns * q.tps + ts) * 2 + stat) * q.split + ch] = accv;
            }
        }
        return;
    }
    if constexpr (GEO) return;       // (the plan gives GEO launches channels-last regions only)
#pragma unroll
    for (int jx = 0; jx < (M16 ? 4 : 2); ++jx) {
        const int pp = M16 ? tile_position16(wpos * 4 + jx, lane & 15, q.TW, q.pair_lg) : tile_position(wpos * 2 + jx, lane & 31, q.TW, q.pair_lg);
        const int pw = pp & (q.TW - 1);
        const int ph = (pp >> q.lgTW) & (q.TH - 1);
        const int pd = pp >> (q.lgTW + q.lgTH);
        const int od = od0 + pd, oh = oh0 + ph, ow = ow0 + pw;
        if (od >= q.Do || oh >= q.Ho || ow >= q.Wo) continue;
        const long long L = (((long long)n * q.Do + od) * q.Ho + oh) * q.Wo + ow;
        const long long ns = L / q.S_out;
        const long long ps = L - ns * q.S_out;
        const int j = M16 ? (jx >> 1) : jx;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
            for (int rx = 0; rx < (M16 ? 2 : 4); ++rx) {
                const int rg = M16 ? 2 * rx + (jx & 1) : rx;
                const int co = M16 ? co0 + wco * (BM / WCO) + 16 * (2 * mi + rx) + 4 * (lane >> 4)
                                   : co0 + wco * (BM / WCO) + mi * 32 + rg * 8 + half * 4;
                const float4 bv = *reinterpret_cast<const float4*>(q.bias + co);
                float v0 = acc[mi][j][rg * 4 + 0] + bv.x;
                float v1 = acc[mi][j][rg * 4 + 1] + bv.y;
                float v2 = acc[mi][j][rg * 4 + 2] + bv.z;
                float v3 = acc[mi][j][rg * 4 + 3] + bv.w;
                if (cl_region) {
                    if (q.res_add != nullptr) {
                        const float4 e = *reinterpret_cast<const float4*>(q.res_add + ns * q.res_add_stride + co);
                        v0 += e.x; v1 += e.y; v2 += e.z; v3 += e.w;
                    }
                    const size_t eo = (size_t)L * q.split + co;
                    if constexpr (sizeof(T) == 2) {
                        if (q.res != nullptr) {
                            const uint2 r = *reinterpret_cast<const uint2*>(q.res + eo * 2);
                            v0 += __uint_as_float(r.x << 16); v1 += __uint_as_float(r.x & 0xFFFF0000u);
                            v2 += __uint_as_float(r.y << 16); v3 += __uint_as_float(r.y & 0xFFFF0000u);
                        }
                        *reinterpret_cast<uint2*>(q.y + eo * 2) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                    } else {
                        if (q.res != nullptr) {
                            const float4 r = *reinterpret_cast<const float4*>(q.res + eo * 4);
                            v0 += r.x; v1 += r.y; v2 += r.z; v3 += r.w;
                        }
                        *reinterpret_cast<float4*>(q.y + eo * 4) = make_float4(v0, v1, v2, v3);
                    }
                } else if (q.y2_cl) {
                    const int w2 = q.cout - q.split;
                    const size_t eo = (size_t)L * w2 + (co - q.split);
                    if (co < q.cout) {                 // widths are multiples of 4: a 4-channel piece is all in or all out
                        if constexpr (sizeof(T) == 2) {
                            if (q.res2 != nullptr) {
                                const uint2 r = *reinterpret_cast<const uint2*>(q.res2 + eo * 2);
                                v0 += __uint_as_float(r.x << 16); v1 += __uint_as_float(r.x & 0xFFFF0000u);
                                v2 += __uint_as_float(r.y << 16); v3 += __uint_as_float(r.y & 0xFFFF0000u);
                            }
                            *reinterpret_cast<uint2*>(q.y2 + eo * 2) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                        } else {
                            if (q.res2 != nullptr) {
                                const float4 r = *reinterpret_cast<const float4*>(q.res2 + eo * 4);
                                v0 += r.x; v1 += r.y; v2 += r.z; v3 += r.w;
                            }
                            *reinterpret_cast<float4*>(q.y2 + eo * 4) = make_float4(v0, v1, v2, v3);
                        }
                    }
                } else {
                    const float vv[4] = {v0, v1, v2, v3};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (co + e < q.cout) {
                            const size_t eo = ((size_t)ns * (q.cout - q.split) + (co + e - q.split)) * q.S_out + ps;
                            if (q.y2_f32 || sizeof(T) == 4)
                                reinterpret_cast<float*>(q.y2)[eo] = vv[e];
                            else
                                reinterpret_cast<bf16_raw*>(q.y2)[eo] = f32_to_bf16(vv[e]);
                        }
                    }
                }
            }
        }
    }
}

struct SplitMap {          // launch grid position (od, oh, ow) -> output row ((od * Ho_out) + oh * oy_mul + oy_add) * Wo_out + ow * ox_mul + ox_add
    int Ho, Wo, Ho_out, Wo_out, oy_mul, oy_add, ox_mul, ox_add;      // (identity unless the launch is one sub-pixel phase of its output)
};
struct SplitOut {          // the two channels-last output regions of a launch: co < split -> y (+ res, res_add), else y2 (+ res2)
    int cout, coutp, split;
    const float* bias;
    const float* res_add;
    long long res_add_stride, S_out;
    const char* res;
    char* y;
    const char* res2;
    char* y2;
};
// Second half of a k-split conv: out[L][co] = round( sum_s slab[s][L][co] + bias[co] + res_add[sample(L)][co] + res[L][co] ), the
// slabs added in split order (fixed => reproducible), the same operand order as the fused epilogue after the contraction.
template <typename T>
__global__ __launch_bounds__(256) void k_splitk_reduce(const float* __restrict__ slab, long long slab_stride, int ksplit, long long positions,
                                                       SplitOut o, SplitMap m) {
    const int c4 = o.coutp / 4;
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= positions * c4) return;
    const long long Ls = item / c4;                      // position in the launch's own grid = slab row
    int co = (int)(item - Ls * c4) * 4;
    if (co >= o.cout) return;                            // padding columns of the last cout tile (widths are multiples of 4)
    const size_t so = (size_t)Ls * o.coutp + co;
    float4 a = *reinterpret_cast<const float4*>(slab + so);
    for (int s = 1; s < ksplit; ++s) {
        const float4 b = *reinterpret_cast<const float4*>(slab + (size_t)s * slab_stride + so);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    long long L = Ls;
    if (m.oy_mul != 1 || m.ox_mul != 1) {
        const int ow = (int)(Ls % m.Wo);
        const long long r = Ls / m.Wo;
        const int oh = (int)(r % m.Ho);
        L = ((r / m.Ho) * m.Ho_out + (oh * m.oy_mul + m.oy_add)) * m.Wo_out + (ow * m.ox_mul + m.ox_add);
    }
    const float4 bv = *reinterpret_cast<const float4*>(o.bias + co);
    float v0 = a.x + bv.x, v1 = a.y + bv.y, v2 = a.z + bv.z, v3 = a.w + bv.w;
    const bool first = co < o.split;
    if (first && o.res_add != nullptr) {
        const float4 e = *reinterpret_cast<const float4*>(o.res_add + (L / o.S_out) * o.res_add_stride + co);
        v0 += e.x; v1 += e.y; v2 += e.z; v3 += e.w;
    }
    const int width = first ? o.split : o.cout - o.split;
    const char* const res = first ? o.res : o.res2;
    char* const y = first ? o.y : o.y2;
    if (!first) co -= o.split;
    const size_t eo = (size_t)L * width + co;
    if constexpr (sizeof(T) == 2) {
        if (res != nullptr) {
            const uint2 r = *reinterpret_cast<const uint2*>(res + eo * 2);
            v0 += __uint_as_float(r.x << 16); v1 += __uint_as_float(r.x & 0xFFFF0000u);
            v2 += __uint_as_float(r.y << 16); v3 += __uint_as_float(r.y & 0xFFFF0000u);
        }
        *reinterpret_cast<uint2*>(y + eo * 2) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
    } else {
        if (res != nullptr) {
            const float4 r = *reinterpret_cast<const float4*>(res + eo * 4);
            v0 += r.x; v1 += r.y; v2 += r.z; v3 += r.w;
        }
        *reinterpret_cast<float4*>(y + eo * 4) = make_float4(v0, v1, v2, v3);
    }
}

#include "conv32.h"
#include "gemm1x1.h"

// ------------------------------------------------------------------------------------------ host
namespace {

using namespace rho_conv;

// One launch, planned on the host: which kernel runs, with which arguments, and what the caller has to provide for it.  conv_plan()
// fills it from the descriptor alone - no HIP call, no pointer of the descriptor followed - and rho_conv_nd_fwd and its three
// queries all read it, so a query cannot disagree with the launch.  The stages run in this order and the first failure ends the
// plan.  A query reads the status of the stage it depends on and no later one: callers ask for the statistics tiles and the
// workspace first and attach stats / gnb_* / ws afterwards, so those queries succeed for descriptors a launch would still refuse.
enum Stage {
    ST_DESC,     // 1  descriptor validation
    ST_ROUTE,    // 2  k_conv32 / k_gemm1x1 (which plan their own launch, conv32.h / gemm1x1.h) or k_conv
    ST_GEOM,     // 3  geometry, cout tile, position tile, grid, statistics tiles      -> rho_conv_stats_tiles
    ST_KSPLIT,   // 4  k-split and its workspace                                        -> rho_conv_workspace_bytes
    ST_ATTACH,   // 5  stats / gnb_* / gna_* / sk_* attachments, LDS bytes
    ST_KEY,      // 6  variant key and its instantiation                                -> rho_conv_variant, rho_conv_nd_fwd
    ST_DONE
};
enum Kernel { K_CONV, K_CONV32, K_GEMM1X1 };
struct VariantKey { bool bf16; int kd, kh, kw, BM, MAXP, NW; bool M16, FSK, GNA, GEO; };      // one instantiation of k_conv
using ConvFn = void (*)(const ConvK);
struct ConvPlan : PlanStatus<Stage> {
    Kernel kernel;
    VariantKey key;          // k_conv only, as are fn, k, grid and lds
    ConvFn fn;
    ConvK k;
    dim3 grid;
    size_t lds;
    int64_t stats_tiles;     // statistics tiles per sample (0: this launch has none)
    int64_t ws_want;         // workspace bytes the k-split asks for (0: not split)
    int ksplit;              // the split the attached workspace allows (1: none)
    long long positions;     // output positions of the launch's own grid = rows of a k-split slab
};

// key -> instantiation; nullptr for a key that has none.  The cout tiles of one flavour: 128 couts on 8 waves with S / 2 halo slots
// per thread, 64 (and 32, where the flavour has it) couts on 4 waves with S
template <typename T, int KD, int KH, int KW, int S, bool M16, bool FSK, bool GNA, bool BM32, bool GEO = false>
ConvFn conv_tiles(const VariantKey& v) {
    if (v.MAXP != (v.BM == 128 ? S / 2 : S) || v.NW != (v.BM == 128 ? 8 : 4)) return nullptr;
    if (v.BM == 128) return k_conv<T, KD, KH, KW, 128, S / 2, 8, M16, FSK, GNA, GEO>;
    if (v.BM == 64) return k_conv<T, KD, KH, KW, 64, S, 4, M16, FSK, GNA, GEO>;
    if constexpr (BM32) { if (v.BM == 32) return k_conv<T, KD, KH, KW, 32, S, 4, M16, FSK, GNA, GEO>; }
    return nullptr;
}
// ... and the flavours of one tap shape.  Every shape has the small-halo tiles (np <= 640: S = 10); the sub-pixel phase shapes (2-tap
// axes; 3x1x1: the even-even parity of a stride-2 split) are stride 1 and have no others.
template <typename T, int KD, int KH, int KW>
ConvFn conv_kernel_taps(const VariantKey& v) {
    constexpr int NT = KD * KH * KW;
    constexpr bool PHASE = (KH == 2 || KW == 2 || (KD == 3 && KH == 1 && KW == 1));
    constexpr bool HAS_M16 = sizeof(T) == 2 && NT > 1 && NT % 3 == 0;      // the 16x16x32 MFMA layout (holds a higher clock under load)
    if (v.GEO) {              // compile-time 4 x 8 x 8 tile: the 16x16x32 3x3x3 variants, with and without the folded skip
        if constexpr (HAS_M16 && NT == 27) {
            if (v.M16 && !v.GNA) return v.FSK ? conv_tiles<T, KD, KH, KW, 10, true, true, false, false, true>(v) : conv_tiles<T, KD, KH, KW, 10, true, false, false, false, true>(v);
        }
        return nullptr;
    }
    if (v.FSK) {              // folded skip: the 16x16x32 3x3x3 variants
        if constexpr (HAS_M16 && NT == 27) { if (v.M16 && !v.GNA) return conv_tiles<T, KD, KH, KW, 10, true, true, false, false>(v); }
        return nullptr;
    }
    if (v.GNA) {              // GroupNorm backward apply in the epilogue: 1x1x1
        if constexpr (NT == 1) { if (!v.M16) return conv_tiles<T, 1, 1, 1, 10, false, false, true, true>(v); }
        return nullptr;
    }
    if (v.M16) {
        if constexpr (HAS_M16) return conv_tiles<T, KD, KH, KW, 10, true, false, false, false>(v);
        return nullptr;
    }
    if (ConvFn f = conv_tiles<T, KD, KH, KW, 10, false, false, false, true>(v)) return f;
    if constexpr (!PHASE) return conv_tiles<T, KD, KH, KW, 28, false, false, false, true>(v);
    return nullptr;
}
template <typename T>
ConvFn conv_kernel(const VariantKey& v) {
    if (v.kd < 1 || v.kd > 3 || v.kh < 1 || v.kh > 3 || v.kw < 1 || v.kw > 3) return nullptr;
    switch (v.kd * 100 + v.kh * 10 + v.kw) {
        case 333: return conv_kernel_taps<T, 3, 3, 3>(v);
        case 133: return conv_kernel_taps<T, 1, 3, 3>(v);
        case 113: return conv_kernel_taps<T, 1, 1, 3>(v);
        case 111: return conv_kernel_taps<T, 1, 1, 1>(v);
        // sub-pixel phases of a conv behind a nearest x2 upsample (3-D / 2-D: both inner axes; 1-D: the last)
        case 322: return conv_kernel_taps<T, 3, 2, 2>(v);
        case 122: return conv_kernel_taps<T, 1, 2, 2>(v);
        case 112: return conv_kernel_taps<T, 1, 1, 2>(v);
        // parity split of a 3-D stride-2 conv (1- and 2-tap inner axes)
        case 311: return conv_kernel_taps<T, 3, 1, 1>(v);
        case 312: return conv_kernel_taps<T, 3, 1, 2>(v);
        case 321: return conv_kernel_taps<T, 3, 2, 1>(v);
    }
    return nullptr;
}
ConvFn conv_kernel(const VariantKey& v) { return v.bf16 ? conv_kernel<bf16_raw>(v) : conv_kernel<float>(v); }

bool m16_env_on() { static const bool on = env_on("RHO_CONV_M16"); return on; }
// A/B knob: short contractions (<= N input-channel chunks) on the 4-wave 64-cout tile, two workgroups per CU, instead of the
// 8-wave 128-cout tile whose waves all sit in set-up / epilogue at the same time (0 = off)
int bm64_max_chunks() { static const int n = getenv("RHO_BM64_MAX_CHUNKS") ? atoi(getenv("RHO_BM64_MAX_CHUNKS")) : 0; return n; }
bool splitk_env_on() { static const bool on = env_on("RHO_CONV_SPLITK"); return on; }
// A/B knob: the compile-time-geometry instantiations (GEO) for whole 4 x 8 x 8 tiles of stride-1 bf16 3x3x3 layers (0 = generic form)
bool geo_env_on() { static const bool on = env_on("RHO_CONV_GEO"); return on; }
unsigned geo_magic(long long d) { return (unsigned)(0xFFFFFFFFull / (unsigned long long)d); }      // see geo_div

// The stages of a plan: returns the error of the stage that p.stage names, or 0 with p.stage = ST_DONE
int conv_plan_stages(const rho_conv_desc& d, ConvPlan& p) {
    if (!d.x1 || !d.w || !d.bias) return RHO_E_ARG;
    if (d.dtype != RHO_F32 && d.dtype != RHO_BF16) return RHO_E_ARG;
    const int CK = d.dtype == RHO_BF16 ? 32 : 16;
    const int c2 = d.x2 ? d.c2 : 0;
    const int cin = d.c1 + c2;
    if (d.c1 <= 0 || d.c1 % CK || c2 % CK) return RHO_E_ALIGN;
    if (d.cout <= 0 || d.coutp < d.cout || d.coutp % 32 || d.split < 0 || d.split > d.cout || d.split % 32) return RHO_E_ARG;
    if (d.split > 0 && !d.y) return RHO_E_ARG;
    if (d.split < d.cout && !d.y2) return RHO_E_ARG;
    if (d.split < d.cout && d.split > 0 && d.coutp != d.cout && !d.y2_cl) return RHO_E_ARG;  // mixed layouts need exact tiling
    if (d.y2_cl && ((d.cout - d.split) % 4 != 0)) return RHO_E_ALIGN;
    if ((d.zs_h || d.zs_w) && (d.up_h || d.up_w || d.sh != 1 || d.sw != 1 || d.out_h <= 0 || d.out_w <= 0)) return RHO_E_ARG;
    if (d.split == d.cout && d.coutp != d.cout) return RHO_E_ARG;               // channels-last rows are not padded
    if ((d.sh != 1 && d.sh != 2) || (d.sw != 1 && d.sw != 2)) return RHO_E_ARG;
    if ((d.up_h && d.sh != 1) || (d.up_w && d.sw != 1)) return RHO_E_ARG;
    if ((d.up_h && d.kh != 3) || (d.up_w && d.kw != 3)) return RHO_E_ARG;
    if (d.n <= 0 || d.d <= 0 || d.h <= 0 || d.w_ <= 0) return RHO_E_ARG;
    // sub-pixel phases: a 2-tap axis at the source resolution, stride 1, the output rows of one parity
    if (d.ph_h < 0 || d.ph_h > 2 || d.ph_w < 0 || d.ph_w > 2) return RHO_E_ARG;
    if ((d.ph_h && ((d.kh != 2 && d.kh != 1) || d.sh != 1 || d.up_h || d.zs_h)) || (d.ph_w && ((d.kw != 2 && d.kw != 1) || d.sw != 1 || d.up_w || d.zs_w)))
        return RHO_E_ARG;
    if ((!d.ph_h && !d.phd_h && d.kh == 2) || (!d.ph_w && !d.phd_w && d.kw == 2)) return RHO_E_ARG;
    if ((d.ph_h || d.ph_w) && (d.split != d.cout || d.kd == 2)) return RHO_E_ARG;      // channels-last outputs only
    if (d.phd_h < 0 || d.phd_h > 2 || d.phd_w < 0 || d.phd_w > 2) return RHO_E_ARG;
    if ((d.phd_h && ((d.kh != 2 && d.kh != 1) || d.sh != 1 || d.up_h || d.zs_h || d.ph_h)) ||
        (d.phd_w && ((d.kw != 2 && d.kw != 1) || d.sw != 1 || d.up_w || d.zs_w || d.ph_w)))
        return RHO_E_ARG;
    if ((d.ph_h || d.phd_h || d.ph_w || d.phd_w) && d.kd * d.kh * d.kw == 1) return RHO_E_ARG;   // (the 1x1x1 path merges the axes)
    if ((d.phd_h || d.phd_w) && (d.kd == 2 || d.pre_a)) return RHO_E_ARG;

    p.stage = ST_ROUTE;
    p.ksplit = 1;
    // the 32 -> 32 channel 3x3x3 layers: the persistent register-resident-weights kernel (conv32.h); the wide bf16 1x1x1
    // convolutions without prologue (attention qkv / proj_out, un-folded skips): a plain GEMM (gemm1x1.h)
    const bool c32 = conv32_applies(d);
    if (c32 || gemm1x1_applies(d)) {
        p.kernel = c32 ? K_CONV32 : K_GEMM1X1;
        p.stats_tiles = c32 ? conv32_wps(d) : gemm1x1_stats_tiles(d);
        p.stage = ST_DONE;
        return 0;
    }

    p.stage = ST_GEOM;
    const int taps = d.kd * d.kh * d.kw;
    const bool k111 = d.kd == 1 && d.kh == 1 && d.kw == 1;
    // output extents per sample (padding k/2).  Zero-stuffed input (dgrad of a stride-2 conv): the
    // virtual input and the output both have the forward conv's input extent out_h / out_w.
    const int hv = d.zs_h ? d.out_h : d.h, wv = d.zs_w ? d.out_w : d.w_;   // virtual input extents
    // (phases: the launch's own output grid is the source grid; it lands on every second row / column of the real output)
    const int ho = (d.ph_h || d.phd_h) ? d.h : d.up_h ? d.h * 2 : (hv + 2 * (d.kh / 2) - d.kh) / d.sh + 1;
    const int wo = (d.ph_w || d.phd_w) ? d.w_ : d.up_w ? d.w_ * 2 : (wv + 2 * (d.kw / 2) - d.kw) / d.sw + 1;
    const int ho_out = d.ph_h ? 2 * ho : ho, wo_out = d.ph_w ? 2 * wo : wo;
    const int n_phase = (d.ph_h ? 2 : 1) * (d.ph_w ? 2 : 1);
    const int phase_idx = (d.ph_h ? d.ph_h - 1 : 0) * (d.ph_w ? 2 : 1) + (d.ph_w ? d.ph_w - 1 : 0);
    ConvK& k = p.k;
    // (a 1-tap phased axis sits on the output row: the even parity of a stride-2 conv's forward / data gradient)
    k.pad_h = d.kh == 1 ? 0 : d.ph_h ? 2 - d.ph_h : d.phd_h ? d.phd_h - 1 : d.kh / 2;
    k.pad_w = d.kw == 1 ? 0 : d.ph_w ? 2 - d.ph_w : d.phd_w ? d.phd_w - 1 : d.kw / 2;
    k.iy_mul = d.phd_h ? 2 : 1; k.iy_add = d.phd_h ? d.phd_h - 1 : 0;
    k.ix_mul = d.phd_w ? 2 : 1; k.ix_add = d.phd_w ? d.phd_w - 1 : 0;
    k.oy_mul = d.ph_h ? 2 : 1; k.oy_add = d.ph_h ? d.ph_h - 1 : 0;
    k.ox_mul = d.ph_w ? 2 : 1; k.ox_add = d.ph_w ? d.ph_w - 1 : 0;
    if (k111 && (d.sh != 1 || d.sw != 1 || d.up_h || d.up_w)) return RHO_E_ARG;
    const int gridz = merge_batch(d, hv, wv, ho, wo, k);
    k.Hs = d.zs_h ? d.h : d.phd_h ? 2 * d.h : k.H;
    k.Ws = d.zs_w ? d.w_ : d.phd_w ? 2 * d.w_ : k.W;
    k.zs_h = d.zs_h; k.zs_w = d.zs_w;
    k.y2_cl = d.y2_cl; k.res2 = (const char*)d.res2;
    k.S_in = (long long)d.d * d.h * d.w_ * (d.phd_h ? 2 : 1) * (d.phd_w ? 2 : 1);
    k.S_out = (long long)d.d * ho_out * wo_out;
    if (d.n * k.S_in >= (1LL << 31) || d.n * k.S_out >= (1LL << 31)) return RHO_E_SHAPE;
    k.Ho_out = k111 ? 1 : ho_out;
    k.Wo_out = k111 ? k.Wo : wo_out;

    // cout tile
    int BM = 32;
    if (d.coutp % 128 == 0 && (d.split % 128 == 0)) BM = 128;
    else if (d.coutp % 64 == 0 && (d.split % 64 == 0)) BM = 64;
    if (BM == 128 && bm64_max_chunks() > 0 && d.kd == 3 && taps > 1 && cin / CK <= bm64_max_chunks()) BM = 64;
    VariantKey& v = p.key;
    v = VariantKey{d.dtype == RHO_BF16, d.kd, d.kh, d.kw, BM, 0, BM == 128 ? 8 : 4, false, false, false, false};

    // position tile.  The weight ring is sized before the tile is known, for every launch the 16x16x32 layout could take
    // (bf16, taps a multiple of 3, stride 1, no upsampling); the layout itself also needs the small halo, see below.
    const size_t lds_cap = 160 * 1024;
    const bool m16_geo = v.bf16 && taps > 1 && taps % 3 == 0 && d.sh == 1 && d.sw == 1 && !d.up_h && !d.up_w;
    const int WSLOTS = (taps % 3 == 0) ? ((((BM == 128 && m16_geo) || (RHO_GB_BM32 && BM == 32)) && RHO_GB_WIDE == 3 && taps % 9 == 0) ? 9 : 3) : 2;   // LDS weight-ring depth (matches the kernel's PIPE / RS)
    int np_cap = (int)((lds_cap - (size_t)WSLOTS * BM * PITCH) / PITCH);
    if (np_cap > 28 * 64) np_cap = 28 * 64;
    const TileChoice t = choose_tile_small_first(d, k.Do, k.Ho, k.Wo, np_cap);
    if (!t.ok) return RHO_E_SHAPE;
    // np = halo positions of the chosen tile -> halo slots per thread: 5 (8 waves) / 10 for np <= 640, else 14 / 28
    const bool small = t.NP <= 640;
    v.MAXP = (BM == 128 ? 1 : 2) * (small ? 5 : 14);
    v.M16 = m16_geo && m16_env_on() && small && BM >= 64;

    k.x1 = (const char*)d.x1; k.x2 = (const char*)d.x2; k.pre_a = d.pre_a; k.pre_b = d.pre_b;
    k.w = (const char*)d.w; k.bias = d.bias; k.res = (const char*)d.res; k.res_add = d.res_add;
    k.y = (char*)d.y; k.y2 = (char*)d.y2;
    k.c1 = d.c1; k.c2 = c2; k.cin = cin;
    k.cout = d.cout; k.coutp = d.coutp; k.split = d.split;
    k.res_add_stride = d.res_add_stride > 0 ? d.res_add_stride : d.split;
    k.sh = d.sh; k.sw = d.sw; k.up_h = d.up_h; k.up_w = d.up_w; k.pre_silu = d.pre_silu; k.y2_f32 = d.y2_f32;
    k.TD = t.TD; k.TH = t.TH; k.TW = t.TW; k.ID = t.ID; k.IH = t.IH; k.IW = t.IW; k.NP = t.NP;
    k.tiles_h = cdiv(k.Ho, t.TH); k.tiles_w = cdiv(k.Wo, t.TW);
    k.lgTW = ilog2(t.TW); k.lgTH = ilog2(t.TH);
    if ((1 << k.lgTW) != t.TW || (1 << k.lgTH) != t.TH) return RHO_E_SHAPE;      // choose_tile only returns powers of two
    k.inv_ihw = 1.0f / (float)(t.IH * t.IW); k.inv_iw = 1.0f / (float)t.IW;
    // 8-wide tiles: pair rows (pd*TH + ph) differing in one bit whose halo offset is 8 (mod 16) positions
    k.pair_lg = -1;
    if (t.TW == 8 && d.sw == 1 && d.sh == 1 && !d.up_h && !d.up_w) {
        for (int b = 0; b < 5 && k.pair_lg < 0; ++b) {
            const long long delta = (b < k.lgTH) ? (long long)(1 << b) * t.IW : (long long)(1 << (b - k.lgTH)) * t.IH * t.IW;
            if ((1 << b) < t.TD * t.TH && delta % 16 == 8) k.pair_lg = b;
        }
    }
    if (d.pre_a && !d.pre_b) return RHO_E_ARG;
    // the compile-time form of this tile (Geo488): stride 1 and no upsampling (the 16x16x32 layout already asks for that), no
    // zero-stuffing, no phases, whole tiles, every output region channels-last in whole 16-byte pieces
    v.GEO = geo_env_on() && v.M16 && d.kd == 3 && d.kh == 3 && d.kw == 3 && t.TD == 4 && t.TH == 8 && t.TW == 8 && k.pair_lg == 2 &&
            !d.zs_h && !d.zs_w && !d.ph_h && !d.ph_w && !d.phd_h && !d.phd_w && k.Do % 4 == 0 && k.Ho % 8 == 0 && k.Wo % 8 == 0 &&
            (d.split == d.cout || (d.y2_cl && (d.cout - d.split) % 8 == 0));

    const long long tiles = (long long)cdiv(k.Do, t.TD) * k.tiles_h * k.tiles_w;
    if (tiles > 0x7FFFFFFFLL || d.coutp / BM > 65535 || gridz > 65535) return RHO_E_SHAPE;
    k.cofast = (d.coutp / BM > 1 && tiles % 8 == 0) ? 1 : 0;
    if (tiles * (d.coutp / BM) >= 65536) v.GEO = false;      // (geo_div's range: tile index, cofast slot and every divisor below 2^16)
    k.mg_tw = geo_magic(k.tiles_w); k.mg_thw = geo_magic((long long)k.tiles_w * k.tiles_h); k.mg_ct = geo_magic(d.coutp / BM);
    p.grid = dim3((unsigned)tiles, (unsigned)(d.coutp / BM), (unsigned)gridz);
    // fused output statistics: only where a tile belongs to one sample and the whole output is channels-last
    int64_t tps_geo = 0;                                 // tiles per sample where every tile lies in one sample, else 0
    if (d.kd == 3) tps_geo = tiles * n_phase;            // phases: the launches of one output share the buffer, each its own tile range
    else if (taps == 1 && k.S_out % 256 == 0 && t.TW == 256) tps_geo = k.S_out / 256;
    p.stats_tiles = (d.split == d.cout && d.split > 0) ? tps_geo : 0;

    p.stage = ST_KSPLIT;
    // k-split (rho_conv_desc.ws): merged-batch launches (2-D / 1-D kernels with taps) whose grid leaves most CUs idle
    p.positions = (long long)k.Do * k.Ho * k.Wo;
    const long long wgs = tiles * (d.coutp / BM);
    const int chunks = cin / CK;
    if (splitk_env_on() && d.kd == 1 && (d.split == d.cout || d.y2_cl) && !d.stats && !d.gna_g && wgs <= 128 && chunks >= 4) {
        int want = (int)(512 / wgs);                               // about two workgroups per CU
        if (want > 16) want = 16;
        const int per = taps == 1 ? 4 : 2;                         // chunks per split at least: the set-up of a tile is paid per split
        if (want > chunks / per) want = chunks / per;
        const long long slab_bytes = p.positions * d.coutp * (long long)sizeof(float);
        if (want >= 2) p.ws_want = want * slab_bytes;
        if (d.ws != nullptr && want >= 2) {
            if (d.ws_bytes / slab_bytes < want) want = (int)(d.ws_bytes / slab_bytes);
            if (want >= 2) p.ksplit = want;
        }
    }
    k.ksplit = p.ksplit; k.slab = (float*)d.ws; k.slab_stride = p.positions * d.coutp;
    if (p.ksplit > 1) p.grid.z = (unsigned)p.ksplit;

    p.stage = ST_ATTACH;
    k.tps = 1;
    if (d.stats) {
        if (p.stats_tiles <= 0) return RHO_E_ARG;
        k.stats = d.stats; k.tps = (int)p.stats_tiles;
        k.stats_off = phase_idx * (int)tiles;
    }
    if (d.gna_g) {
        // GroupNorm backward apply in the epilogue: both output regions on the transposed path, one sample per tile
        const int pe = v.bf16 ? 8 : 4;
        if (taps != 1 || d.res || d.res2 || d.stats || !d.gnb_x1 || !d.gnb_a || !d.gnb_b || !d.gna_cA || !d.gna_cP || !d.gna_cQ || d.split <= 0 || d.cout % 32 ||
            d.gnb_c1 <= 0 || d.gnb_c1 > d.cout || d.gnb_c1 % 32 || ((d.gnb_c1 < d.cout) != (d.gnb_x2 != nullptr)) || tps_geo <= 0 ||
            (d.split < d.cout && (!d.y2_cl || (d.cout - d.split) % pe != 0)) || d.gnb_silu < 0 || d.gnb_silu > 1 || n_phase != 1)
            return RHO_E_ARG;
        k.gna_g = (const char*)d.gna_g; k.gna_cA = d.gna_cA; k.gna_cP = d.gna_cP; k.gna_cQ = d.gna_cQ;
        k.tps = (int)tps_geo;
    } else if (d.gnb_x1) {
        if (!d.stats || !d.gnb_a || !d.gnb_b || d.gnb_c1 <= 0 || d.gnb_c1 > d.split || d.gnb_c1 % 32 || (d.split - d.gnb_c1) % 32 ||
            ((d.gnb_c1 < d.split) != (d.gnb_x2 != nullptr)))
            return RHO_E_ARG;
    }
    if (d.gna_g || d.gnb_x1) {
        k.gnb_x1 = (const char*)d.gnb_x1; k.gnb_x2 = (const char*)d.gnb_x2; k.gnb_a = d.gnb_a; k.gnb_b = d.gnb_b;
        k.gnb_c1 = d.gnb_c1; k.gnb_silu = d.gnb_silu;
    }
    size_t lds = (size_t)t.NP * PITCH + (size_t)WSLOTS * BM * PITCH;
    size_t lds_sk = 0;
    if (d.sk_w) {
        // folded 1x1x1 skip: the 16x16x32 3x3x3 variants only (bf16, stride 1, whole output channels-last, same-size input)
        if (!d.sk_x1 || d.sk_c1 <= 0 || d.sk_c1 % CK || d.sk_c2 < 0 || d.sk_c2 % CK || ((d.sk_c2 > 0) != (d.sk_x2 != nullptr))) return RHO_E_ARG;
        if (!(v.M16 && d.kd == 3 && d.kh == 3 && d.kw == 3 && d.split == d.cout && !d.zs_h && !d.zs_w && !d.ph_h && !d.ph_w && !d.phd_h && !d.phd_w)) return RHO_E_ARG;
        k.sk_x1 = (const char*)d.sk_x1; k.sk_x2 = (const char*)d.sk_x2; k.sk_w = (const char*)d.sk_w; k.sk_bias = d.sk_bias;
        k.sk_c1 = d.sk_c1; k.sk_c2 = d.sk_c2;
        lds_sk = (size_t)2 * 256 * PITCH + (size_t)2 * BM * PITCH;
    }
    if (taps > 1 && d.kd == 3 && d.pre_a && lds + (size_t)2 * cin * sizeof(float) <= (BM == 128 ? lds_cap : lds_cap / 2)) {
        k.coef_off = (int)lds;                                    // after the halo tile and the weight ring
        lds += (size_t)2 * cin * sizeof(float);
    }
    if (taps == 1)        // 1x1x1: double-buffered activations + weights + the prologue coefficients of one sample
        lds = (size_t)2 * 256 * PITCH + (size_t)2 * BM * PITCH + (d.pre_a ? (size_t)2 * k.cin * sizeof(float) : 0);
    if (k.coef_off > 0 && (size_t)k.coef_off < lds_sk) { lds -= (size_t)2 * cin * sizeof(float); k.coef_off = 0; }   // (the skip phase's buffers would overlap them)
    if (d.pre_a && k.coef_off == 0) v.GEO = false;             // (its staging reads the prologue coefficients from LDS only)
    if (lds < lds_sk) lds = lds_sk;
    if (d.stats) { const size_t lr = (size_t)(BM == 128 ? 512 : 256) * 16 * sizeof(float); if (lds < lr) lds = lr; }
    const size_t lds_epi = (size_t)256 * (BM * 4 + 16);       // epilogue transpose staging (fp32 rows, all 256 positions at once)
    if ((d.split > 0 || d.y2_cl) && lds < lds_epi) lds = lds_epi;
    p.lds = lds;

    p.stage = ST_KEY;
    v.FSK = k.sk_w != nullptr; v.GNA = k.gna_g != nullptr;
    p.fn = conv_kernel(v);
    if (p.fn == nullptr) {
        // a tap shape that has only the small-halo tiles (the phase kernels) is a shape error, any other key has no kernel at all
        VariantKey s = v;
        s.MAXP = BM == 128 ? 5 : 10;
        return conv_kernel(s) != nullptr ? RHO_E_SHAPE : RHO_E_ARG;
    }
    p.stage = ST_DONE;
    return 0;
}

ConvPlan conv_plan(const rho_conv_desc* dp) {
    ConvPlan p{};             // (stage = ST_DESC)
    p.rc = dp ? conv_plan_stages(*dp, p) : RHO_E_ARG;
    return p;
}

int launch_conv(const rho_conv_desc& d, const ConvPlan& p, hipStream_t st) {
    if (p.kernel == K_CONV32) return launch_conv32(d, st);
    if (p.kernel == K_GEMM1X1) return launch_gemm1x1(d, st);
    const ConvK& k = p.k;
    const int rc = launch_lds(p.fn, p.grid, dim3(p.key.NW * 64), p.lds, st, k);
    if (rc != 0 || p.ksplit == 1) return rc;
    const long long items = p.positions * (d.coutp / 4);
    const dim3 rgrid((unsigned)((items + 255) / 256));
    const SplitMap sm{k.Ho, k.Wo, k.Ho_out, k.Wo_out, k.oy_mul, k.oy_add, k.ox_mul, k.ox_add};
    const SplitOut so{d.cout, d.coutp, d.split, d.bias, d.res_add, (long long)k.res_add_stride, k.S_out, (const char*)d.res, (char*)d.y,
                      (const char*)d.res2, (char*)d.y2};
    if (d.dtype == RHO_BF16) hipLaunchKernelGGL(k_splitk_reduce<bf16_raw>, rgrid, dim3(256), 0, st, k.slab, k.slab_stride, p.ksplit, p.positions, so, sm);
    else hipLaunchKernelGGL(k_splitk_reduce<float>, rgrid, dim3(256), 0, st, k.slab, k.slab_stride, p.ksplit, p.positions, so, sm);
    return hip_status();
}

}  // namespace

extern "C" int rho_conv_nd_fwd(const rho_conv_desc* dp, void* stream) {
    const ConvPlan p = conv_plan(dp);
    return p.rc != 0 ? p.rc : launch_conv(*dp, p, as_stream(stream));
}

// The name of what rho_conv_nd_fwd launches, formatted from the plan's key
extern "C" int rho_conv_variant(const rho_conv_desc* dp, char* buf, int cap) {
    if (!buf || cap < 64) return RHO_E_ARG;
    buf[0] = 0;
    const ConvPlan p = conv_plan(dp);
    const VariantKey& v = p.key;
    if (p.rc != 0) return p.rc;
    if (p.kernel == K_CONV32) snprintf(buf, (size_t)cap, "k_conv32<bf16>");
    else if (p.kernel == K_GEMM1X1) snprintf(buf, (size_t)cap, "k_gemm1x1<bf16,256x%d>", G1_BN);
    else snprintf(buf, (size_t)cap, "k_conv<%s,%d,%d,%d,BM=%d,MAXP=%d,NW=%d,M16=%d>%s%s", v.bf16 ? "bf16" : "f32", v.kd, v.kh, v.kw, v.BM,
                  v.MAXP, v.NW, (int)v.M16, v.FSK ? "+skip" : "", v.GNA ? "+gn_apply" : "");
    // the name is the contract; behind its terminating NUL a second string tells which form of the instantiation runs
    // ("geo=1": compile-time 4 x 8 x 8 tile geometry), for tests and the --dump-ops table
    const size_t len = strlen(buf);
    if (len + 8 <= (size_t)cap) snprintf(buf + len + 1, (size_t)cap - len - 1, "geo=%d", (p.kernel == K_CONV && v.GEO) ? 1 : 0);
    return 0;
}

extern "C" int64_t rho_conv_stats_tiles(const rho_conv_desc* dp) {
    const ConvPlan p = conv_plan(dp);
    return p.status(ST_GEOM) == 0 ? p.stats_tiles : 0;
}

extern "C" int64_t rho_conv_workspace_bytes(const rho_conv_desc* dp) {
    const ConvPlan p = conv_plan(dp);
    return p.status(ST_KSPLIT) == 0 ? p.ws_want : 0;
}
