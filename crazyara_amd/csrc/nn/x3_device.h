// Device helpers of the float16x3 tower kernels, shared by the translation units that hold them (x3.hip: the symmetric, split-board,
// two-role and float16p8 towers; x3_tail.cpp: the two-role tower with a 64-channel tail chunk): the split of f32 values into f16 pairs,
// the LDS tile geometry, the depthwise on the expand accumulators, the weight descriptors, the residual stream in the project
// registers and its SE gate.  Everything has internal linkage (anonymous namespace): each translation unit inlines its own copy.
#pragma once
#include "kernels.h"
#include "device_utils.h"

#include <type_traits>

// CRA_X3_ABL: development switches that TIME parts of the tower's chunk loop (scripts/ubench/x3_tower_ablate.hip); every bit computes wrong
// results on purpose, so they only compile in a development build.  1: no depthwise arithmetic, 2: no expand MFMAs, 4: no project MFMAs,
// 8: no LDS operand reads (expand and project), 16: no weight loads, 32: no chunk barriers, 64: no t2 stores, 128: the expand GEMM issues
// the mixed split's instruction mix (per 64 k two f16 MFMAs and one 8-bit 16x16x128 on whatever the registers hold); tower_p8_kernel
// honours 1, 2, 4, 16, 64 and (round 6, the weight-port question) 512: the 8-bit weight images are fetched at HALF size -- one 16-byte
// piece per lane and 64-k step, the other half a register copy -- i.e. the L2 -> CU stream of a 3-bytes-per-weight layout with its byte
// permutes stood in for by the copies; 1024: no 8-bit weight fetches at all (2 bytes per weight)
#ifndef CRA_X3_ABL
#define CRA_X3_ABL 0
#endif
#if CRA_X3_ABL != 0 && !defined(CRA_DEVELOPMENT)
#error "CRA_X3_ABL is a development switch (wrong results): build with -DCRA_DEVELOPMENT"
#endif
// CRA_X3_TRACE=<block>: development, the two-role tower stamps the shader clock at its phase boundaries while it runs block <block>
// (workgroups 0 and 131, every wave; scripts/ubench/x3_tower_ablate.hip prints the timeline)
#if defined(CRA_X3_TRACE) && !defined(CRA_DEVELOPMENT)
#error "CRA_X3_TRACE is a development switch: build with -DCRA_DEVELOPMENT"
#endif

namespace cra {

#ifdef CRA_X3_TRACE
namespace {
__device__ unsigned long long x3_trace[2][8][128][2];      // [workgroup 0 | 131][wave][stamp](clock, interval * 16 + phase id)
}  // namespace
#define X3_STAMP(id)                                                                                    \
    do {                                                                                                \
        if (tracing && trace_n < 128) {                                                                 \
            const unsigned long long t_ = __builtin_readcyclecounter();                                 \
            if (lane == 0) {                                                                            \
                x3_trace[b != 0][wave][trace_n][0] = t_;                                                \
                x3_trace[b != 0][wave][trace_n][1] = (unsigned long long)((kk + 1) * 16 + (id));        \
            }                                                                                           \
            ++trace_n;                                                                                  \
        }                                                                                               \
    } while (0)
#define X3_STAMP_SLAB(i_, sl_) do { const int kk = (i_) - 1; X3_STAMP(6); (void)(sl_); } while (0)      // (a k-slab of an EXPAND interval begins)
#else
#define X3_STAMP(id) do { } while (0)
#define X3_STAMP_SLAB(i_, sl_) do { } while (0)
#endif

namespace {
constexpr int X3_ABL = CRA_X3_ABL;
__device__ __forceinline__ void x3_mfma(const half8& a, const half8& b, f32x4& c, bool on) {
    if (on) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    else asm volatile("" : "+v"(c) : "v"(a), "v"(b));
}

// (a, b) -> packed f16 pairs hi = rne(a | b), lo = rne((a | b) - hi): 4 instructions (pack-convert, two mix-precision FMAs that read the
// f16 halves in place, pack-convert) where the compiler's form of the same arithmetic takes about ten.  The difference a - hi is exact.
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
    float ra, rb;
    asm("v_cvt_pk_f16_f32 %0, %3, %4\n\t"
        "v_fma_mix_f32 %1, %0, -1.0, %3 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %2, %0, -1.0, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(hi), "=&v"(ra), "=&v"(rb)
        : "v"(a), "v"(b));
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(lo) : "v"(ra), "v"(rb));
}
__device__ __forceinline__ void split8(const float (&v)[8], half8& hi, half8& lo) {
    uint32_t h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_pair(v[2 * j], v[2 * j + 1], h[j], l[j]);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    hi = __builtin_bit_cast(half8, u32x4{h[0], h[1], h[2], h[3]});
    lo = __builtin_bit_cast(half8, u32x4{l[0], l[1], l[2], l[3]});
}
__device__ __forceinline__ void split4(const float (&v)[4], half4& hi, half4& lo) {
    uint32_t h[2], l[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) split_pair(v[2 * j], v[2 * j + 1], h[j], l[j]);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    hi = __builtin_bit_cast(half4, u32x2{h[0], h[1]});
    lo = __builtin_bit_cast(half4, u32x2{l[0], l[1]});
}
}  // namespace

// ---- the fused bottleneck block's tiles, depthwise and weights (x3.hip: "Fused bottleneck block") ----
namespace {
struct X3Block {
    static constexpr int C = 256, NW = 8, NE = 1, CK = 16 * NW * NE, NTHR = 64 * NW, NJ = C / 16 / NW;
    static constexpr int XROW = C + 16;      // halves; 32-byte row pad (16 and 48 bytes measured the same: profiles/r03/s_*)
    static constexpr int TROW = CK + 16;
    static constexpr size_t dws_bytes = size_t(NW) * NE * 1024;
    // NE = 1: the depthwise output tile is double-buffered -- ONE barrier per chunk (the depthwise of chunk k + 1 writes the other
    // buffer while slower waves still read chunk k's in their project phase), and the waves of a SIMD drift apart: one is in a
    // matrix phase while its partner runs the depthwise
    static constexpr int T2BUF = NE == 1 ? 2 : 1;
    static constexpr size_t lds_bytes = (size_t(2) * 64 * XROW + size_t(2) * T2BUF * 64 * TROW) * sizeof(half_t) + dws_bytes;   // NE = 1: 151,552 B; NE = 2: 155,648 B
};
static_assert(X3Block::lds_bytes + 8192 <= 160 * 1024, "LDS budget (tower_p8_kernel<5> takes 8 KiB more for its records)");

struct X3Tiles {
    half_t *xh, *xl;        // [64][XROW] block input = residual stream, hi / lo
    half_t *t2h, *t2l;      // [T2BUF][64][TROW] depthwise output of a chunk, hi / lo (buffer = chunk parity)
    float* dws;             // [8 waves][NE][256 floats] the waves' depthwise records of the chunk (16 rows x 16 channels each)
};
__device__ __forceinline__ X3Tiles x3_tiles(char* smem) {
    X3Tiles t;
    t.xh = reinterpret_cast<half_t*>(smem);
    t.xl = t.xh + 64 * X3Block::XROW;
    t.t2h = t.xl + 64 * X3Block::XROW;
    t.t2l = t.t2h + X3Block::T2BUF * 64 * X3Block::TROW;
    t.dws = reinterpret_cast<float*>(t.t2l + X3Block::T2BUF * 64 * X3Block::TROW);
    return t;
}

// Row order of the board tiles in LDS.  A 16-square MFMA tile t (rows t * 16 ... + 15 of the x and t2 tiles) holds board ranks t (lanes
// l15 = 0-7, files a-h) and t + 4 (lanes 8-15): the rank above / below a lane's square is then the SAME lane of tile t - 1 / t + 1, so the
// depthwise finds its vertical neighbours in the neighbouring accumulator registers without a lane shuffle or a select; only rank 4's upper
// and rank 3's lower neighbour cross the two halves (one row_ror:8 each).  Everything between staging and the store to HBM works on tile
// rows and never needs to know which square a row is.
__device__ __forceinline__ int x3_row(int sq) { return ((sq >> 3) & 3) * 16 + (sq >> 5) * 8 + (sq & 7); }      // square -> tile row
__device__ __forceinline__ int x3_square(int row) { return ((row >> 4) + 4 * ((row >> 3) & 1)) * 8 + (row & 7); }   // tile row -> square

typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int CTRL> __device__ __forceinline__ f32x2 dpp_mov2(f32x2 v) { return f32x2{dpp_mov<CTRL>(v.x), dpp_mov<CTRL>(v.y)}; }
__device__ __forceinline__ f32x2 pair_of(const f32x4& v, int p) { return p == 0 ? f32x2{v[0], v[1]} : f32x2{v[2], v[3]}; }

// D of one 16-channel tile: BN1 bias + ReLU on the expand accumulators, depthwise 3x3, BN2 bias + ReLU, exact f32 in the tap order of
// block_kernel_dpp (kernels.hip).  A lane holds 4 channels (accumulator rows r) of one file on ranks t / t + 4 (x3_row); channels go two
// at a time (P = 0, 1).
// Horizontal neighbours: row_shr:1 / row_shl:1 copies, each feeding the three outputs it is up / mid / down neighbour of; lane 8 would
// read lane 7 (file h of the other rank) and lane 0 a zero: a lane on file a / h reads its dx = -1 / +1 weights from the record's ZERO rows
// (an address offset computed once per kernel, x3_edge_offsets; as six multiplies per channel the masks were 7 % of the depthwise).
// In pieces (load, gather<P>, taps<P>) so that a caller can spread them over a stretch of MFMAs.
//   rec: this tile's records in LDS, [16 rows: taps dx = -1 (dy = -1, 0, 1), dx = 0, dx = +1, BN1 bias, BN2 bias, 5 rows of zeros][16 channels]
struct X3EdgeOffsets { int left, right; };                       // in floats: 11 rows / 5 rows from the dx = -1 / +1 rows to the zero rows, or 0
__device__ __forceinline__ X3EdgeOffsets x3_edge_offsets(int l15) { return X3EdgeOffsets{(l15 & 7) == 0 ? 11 * 16 : 0, (l15 & 7) == 7 ? 5 * 16 : 0}; }
struct X3Depthwise {
    f32x2 w[11];                                                 // the current channel pair's records (rows 0 ... 10)
    f32x2 S[6], L[6], R[6];                                      // rank - 1 ... rank + 4 of this lane's half: S[1 + t] = tile t
    float outv[4][4];                                            // [tile][channel r]

    template <int P> __device__ __forceinline__ void load(const float* rec, int lg, const X3EdgeOffsets& e) {
#pragma unroll
        for (int q = 0; q < 11; ++q) w[q] = *reinterpret_cast<const f32x2*>(rec + (q < 3 ? e.left : q >= 6 && q < 9 ? e.right : 0) + q * 16 + lg * 4 + 2 * P);
    }
    // acc_scale: the accumulators carry the weights' power-of-two scale (Precision float16p8): S = relu(acc * acc_scale + bias), one FMA instead of the add
    template <int P, bool SCALED = false> __device__ __forceinline__ void gather(const f32x4 (&acc)[4], bool upper, int c0 = 0, int c1 = 2, float acc_scale = 1.f) {
        if constexpr (X3_ABL & 1) {
#pragma unroll
            for (int t = 0; t < 4; ++t) S[1 + t] = pair_of(acc[t], P) + w[0];
            return;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c < c0 || c >= c1) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) S[1 + t][c] = SCALED ? fmaxf(fmaf(acc[t][2 * P + c], acc_scale, w[9][c]), 0.f) : fmaxf(acc[t][2 * P + c] + w[9][c], 0.f);
            const float across_up = dpp_mov<DPP_ROW_ROR8>(S[4][c]), across_dn = dpp_mov<DPP_ROW_ROR8>(S[1][c]);
            S[0][c] = upper ? across_up : 0.f;                    // above rank 4 lies rank 3 (tile 3, other half); above rank 0 the edge
            S[5][c] = upper ? 0.f : across_dn;                    // below rank 3 lies rank 4 (tile 0, other half); below rank 7 the edge
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                L[j][c] = dpp_mov<DPP_ROW_SHR1>(S[j][c]);
                R[j][c] = dpp_mov<DPP_ROW_SHL1>(S[j][c]);
            }
        }
    }
    // plain v_fmac_f32, NOT v_pk_fma_f32: a packed f32 FMA does not run in the shadow of MFMAs (scripts/ubench/mix_kinds.hip: an MFMA
    // followed by two of them 38.5 cycles, by two v_fmac_f32 18.5; beside another wave's MFMAs 14.7 cycles each against 8.75)
    template <int P> __device__ __forceinline__ void taps(int t0, int t1) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < t0 || t >= t1) continue;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if constexpr (X3_ABL & 1) {
                    outv[t][2 * P + c] = S[1 + t][c];
                    continue;
                }
                float a = w[10][c];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    a = fmaf(w[dy][c], L[t + dy][c], a);
                    a = fmaf(w[3 + dy][c], S[t + dy][c], a);
                    a = fmaf(w[6 + dy][c], R[t + dy][c], a);
                }
                outv[t][2 * P + c] = fmaxf(a, 0.f);
            }
        }
    }
    // keeps the values computed so far where they were written (a piece set between MFMAs is otherwise sunk to its first use)
    __device__ __forceinline__ void pin_taps(int t0, int t1, int P) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (t >= t0 && t < t1) asm volatile("" : "+v"(outv[t][2 * P + c]));
    }
};
__device__ __forceinline__ void x3_depthwise(const f32x4 (&acc)[4], const float* rec, int lg, bool upper, const X3EdgeOffsets& e, float (&outv)[4][4]) {
    X3Depthwise dw;
    dw.template load<0>(rec, lg, e);
    dw.template gather<0>(acc, upper);
    dw.template taps<0>(0, 4);
    dw.template load<1>(rec, lg, e);
    dw.template gather<1>(acc, upper);
    dw.template taps<1>(0, 4);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) outv[t][r] = dw.outv[t][r];
}
// D of one 16-channel tile with a 5x5 depthwise (RISEv3.3's wide blocks; Precision float16p8's tower_p8_kernel<5>): X3Depthwise's scheme
// on ranks - 2 ... + 2 and files - 2 ... + 2, one channel at a time (25 weights in registers).  The rank above / below a lane's square is the
// same lane of the neighbouring tile; two rows on either side of the rank 3 / 4 seam come from the other half of the row (row_ror:8).
// Horizontal neighbours are row_shr / row_shl copies by 1 and 2; a lane whose file lacks a neighbour reads that column's weights from the
// record's zero rows (X3EdgeOffsets5).
//   rec: this tile's records in LDS, [32 rows: taps column dx = -2 (dy = -2 ... 2), dx = -1, 0, +1, +2, BN1 bias, BN2 bias, 5 rows of zeros][16 channels]
struct X3EdgeOffsets5 { int o[5]; };                             // in floats, per tap column: to the zero rows 27 ... 31, or 0
__device__ __forceinline__ X3EdgeOffsets5 x3_edge_offsets5(int l15) {
    const int f = l15 & 7;
    X3EdgeOffsets5 e;
    e.o[0] = f < 2 ? 27 * 16 : 0;
    e.o[1] = f < 1 ? 22 * 16 : 0;
    e.o[2] = 0;
    e.o[3] = f > 6 ? 12 * 16 : 0;
    e.o[4] = f > 5 ? 7 * 16 : 0;
    return e;
}
struct X3Depthwise5 {
    float w[27];                                                 // the current channel's records (rows 0 ... 26)
    float S[8];                                                  // rank - 2 ... rank + 5 of this lane's half: S[2 + t] = tile t
    float outv[4][4];                                            // [tile][channel r]

    template <int CH> __device__ __forceinline__ void load(const float* rec, int lg, const X3EdgeOffsets5& e) {
#pragma unroll
        for (int q = 0; q < 27; ++q) w[q] = rec[(q < 25 ? e.o[q / 5] : 0) + q * 16 + lg * 4 + CH];
    }
    template <int CH> __device__ __forceinline__ void gather(const f32x4 (&acc)[4], bool upper, float acc_scale) {
#pragma unroll
        for (int t = 0; t < 4; ++t) S[2 + t] = fmaxf(fmaf(acc[t][CH], acc_scale, w[25]), 0.f);
        const float u3 = dpp_mov<DPP_ROW_ROR8>(S[5]), u2 = dpp_mov<DPP_ROW_ROR8>(S[4]);
        const float d0 = dpp_mov<DPP_ROW_ROR8>(S[2]), d1 = dpp_mov<DPP_ROW_ROR8>(S[3]);
        S[1] = upper ? u3 : 0.f;                                  // above rank 4 lies rank 3 (tile 3, other half), above that rank 2; above rank 0 the edge
        S[0] = upper ? u2 : 0.f;
        S[6] = upper ? 0.f : d0;                                  // below rank 3 lie ranks 4, 5 (tiles 0, 1, other half); below rank 7 the edge
        S[7] = upper ? 0.f : d1;
    }
    template <int CH> __device__ __forceinline__ void taps() {
        float a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[t] = w[26];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v[5] = {dpp_mov<DPP_ROW_SHR2>(S[j]), dpp_mov<DPP_ROW_SHR1>(S[j]), S[j], dpp_mov<DPP_ROW_SHL1>(S[j]), dpp_mov<DPP_ROW_SHL2>(S[j])};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int dy = j - t;
                if (dy < 0 || dy > 4) continue;
#pragma unroll
                for (int g = 0; g < 5; ++g) a[t] = fmaf(w[g * 5 + dy], v[g], a[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) outv[t][CH] = fmaxf(a[t], 0.f);
    }
};
// float board tile [64][256] (optionally x := x * gate[c], _ChannelAttentionModule.forward, builder_util.py:114) -> split tiles
__device__ __forceinline__ void x3_stage_tile(const X3Tiles& T, const float* xb, const float* g, int tid) {
    constexpr int C = X3Block::C, XROW = X3Block::XROW;
#pragma unroll 1
    for (int i = tid; i < 64 * (C / 8); i += X3Block::NTHR) {
        const int sq = i / (C / 8), v = i - sq * (C / 8), r = x3_row(sq);
        float f[8];
        load8<float>(xb + size_t(sq) * C + v * 8, f);
        if (g) {
            float gv[8];
            load8<float>(g + v * 8, gv);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= gv[j];
        }
        half8 h, l;
        split8(f, h, l);
        *reinterpret_cast<half8*>(T.xh + r * XROW + v * 8) = h;
        *reinterpret_cast<half8*>(T.xl + r * XROW + v * 8) = l;
    }
}

// The chunk loop of one block: accP[j][t] += project(depthwise(expand(x))) for this wave's 32 couts x 64 squares.  The caller has put a
// barrier behind the last write of the x tiles.  On return every wave is done with the x tiles (the last expand phase lies before the
// last chunk barrier); other waves may still be reading t2 in their last project phase.
// Weights are read with raw buffer loads: resource descriptor + wave-uniform byte offset in SGPRs, the lane part one constant VGPR.
// (Through the pointers of a descriptor array in device memory the compiler can only emit FLAT loads, which count on the LDS
// counter too: every wait for an LDS operand then also waits for the weight fragments requested slabs ahead.)
struct X3Weights {
    __amdgpu_buffer_rsrc_t w1h, w1l, w3h, w3l;   // packed expand / project weights, hi / lo (kernels.h: packed-weight geometry)
    __amdgpu_buffer_rsrc_t dw;                   // [cop_pad / 16 tiles][16 rows: taps, BN1 bias, BN2 bias, zeros (X3Depthwise)][16 channels] floats
    int cop_pad;
};
// The pointer is wave-uniform, but read from a descriptor array in device memory the compiler has it in VGPRs and wraps EVERY buffer load
// in a waterfall loop (readfirstlane / compare / saveexec / branch: ~12 instructions per load, 33 loads per chunk): say so explicitly.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x3_rsrc(const void* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint64_t u = (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))))) << 32) |
                       uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(u), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ X3Weights x3_weights(const void* w1h, const void* w1l, const void* w3h, const void* w3l, const float* dwpk, int cop_pad) {
    X3Weights W;
    W.w1h = x3_rsrc(w1h); W.w1l = x3_rsrc(w1l); W.w3h = x3_rsrc(w3h); W.w3l = x3_rsrc(w3l);
    W.dw = x3_rsrc(dwpk);
    W.cop_pad = __builtin_amdgcn_readfirstlane(cop_pad);
    return W;
}
__device__ __forceinline__ half8 x3_frag(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, uint32_t frag) {      // fragment = 64 lanes x 16 B
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, frag * 1024u, 0));
}
}  // namespace

// ---- the run of blocks in one launch: SE gate and the residual stream in registers ----
namespace {
// x3_se_fcs: the gate from the channel means (se_mean, LDS, written and barrier'd by the caller): both FC stages of ca_se / the one of eca_se; ends with a barrier
__device__ __forceinline__ void x3_se_fcs(const X3TowerBlock& d, const float* se_mean, float* se_h, float* se_gate, const f32x4 (&wa)[16], const f32x4 (&wb)[16], int tid) {
    constexpr int GRP = 36;
    auto dot32 = [](const f32x4 (&w)[16], const float* v, float& s0, float& s1) {   // v: 32 floats, 16-byte aligned; w[i] = (a, b, a', b') of k = 2i, 2i+1
#pragma unroll
        for (int k4 = 0; k4 < 8; ++k4) {
            const f32x4 m = *reinterpret_cast<const f32x4*>(v + 4 * k4);
            s0 = fmaf(w[2 * k4][0], m[0], s0); s1 = fmaf(w[2 * k4][1], m[0], s1);
            s0 = fmaf(w[2 * k4][2], m[1], s0); s1 = fmaf(w[2 * k4][3], m[1], s1);
            s0 = fmaf(w[2 * k4 + 1][0], m[2], s0); s1 = fmaf(w[2 * k4 + 1][1], m[2], s1);
            s0 = fmaf(w[2 * k4 + 1][2], m[3], s0); s1 = fmaf(w[2 * k4 + 1][3], m[3], s1);
        }
    };
    if (d.se_kind == 1) {
        {
            const int j2 = tid >> 3, kq = tid & 7;
            float s0 = 0.f, s1 = 0.f;
            dot32(wa, se_mean + kq * GRP, s0, s1);
            s0 += dpp_mov<0x111>(s0); s1 += dpp_mov<0x111>(s1);
            s0 += dpp_mov<0x112>(s0); s1 += dpp_mov<0x112>(s1);
            s0 += dpp_mov<0x114>(s0); s1 += dpp_mov<0x114>(s1);             // lane 7 of the group of 8: the whole sum
            if (kq == 7) {                                                    // hidden j = 2*j2, +1 at (j / 32) * 36 + j % 32
                float* h = se_h + (j2 >> 4) * GRP + 2 * (j2 & 15);
                h[0] = fmaxf(s0, 0.f);
                h[1] = fmaxf(s1, 0.f);
            }
        }
        __syncthreads();
        {
            const int c2 = tid >> 2, kq = tid & 3;
            float s0 = 0.f, s1 = 0.f;
            dot32(wb, se_h + kq * GRP, s0, s1);
            s0 += dpp_mov<0x111>(s0); s1 += dpp_mov<0x111>(s1);
            s0 += dpp_mov<0x112>(s0); s1 += dpp_mov<0x112>(s1);             // lane 3 of the group of 4
            if (kq == 3) {
                se_gate[2 * c2] = hard_sigmoid(s0);
                se_gate[2 * c2 + 1] = hard_sigmoid(s1);
            }
        }
    } else {
        const int c2 = tid >> 2, kq = tid & 3;
        float s0 = 0.f, s1 = 0.f;
        dot32(wa, se_mean + (2 * kq) * GRP, s0, s1);
        dot32(wb, se_mean + (2 * kq + 1) * GRP, s0, s1);
        s0 += dpp_mov<0x111>(s0); s1 += dpp_mov<0x111>(s1);
        s0 += dpp_mov<0x112>(s0); s1 += dpp_mov<0x112>(s1);
        if (kq == 3) {
            se_gate[2 * c2] = hard_sigmoid(d.se_b[2 * c2] + s0);
            se_gate[2 * c2 + 1] = hard_sigmoid(d.se_b[2 * c2 + 1] + s1);
        }
    }
    __syncthreads();
}
// mean[c] (scratch, written by the caller) -> gate[c] in scratch: both FC stages, every thread of the workgroup.  Ends behind a barrier
// with the gate valid.
__device__ __forceinline__ void x3_se_gate_from_mean(const X3TowerBlock& d, float* scratch, int tid) {
    constexpr int GRP = 36;
    f32x4 wa[16], wb[16];
    auto load_thread_weights = [&](const float* base, f32x4 (&dst)[16]) {
        const f32x4* pk = reinterpret_cast<const f32x4*>(base) + tid;
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[i] = pk[i * 512];
    };
    load_thread_weights(d.se_w1t, wa);
    load_thread_weights(d.se_kind == 1 ? d.se_w2t : d.se_w1t + size_t(16) * 512 * 4, wb);
    __syncthreads();                                                    // the means are in
    x3_se_fcs(d, scratch, scratch + 8 * GRP, scratch + 12 * GRP, wa, wb, tid);
}

// The residual stream of the float16x3 towers lives in the project accumulators of the waves that own its couts, exact f32: a wave's
// NJ cout tiles from tile0 on (tower_x3_kernel: 2, tower_x3_roles_kernel's PROJECT waves: 4), x[j][t][r] = x[square of tile row
// t * 16 + l15][channel (tile0 + j) * 16 + lg * 4 + r].  A block adds its BN3 bias and then its project sums ON it; the block epilogue only
// writes the operand tiles xh / xl of the new x.  Both tower kernels run these helpers: the same bits.
template <int NJ>
__device__ __forceinline__ void x3_stream_load(f32x4 (&x)[NJ][4], const float* xb, int tile0, int l15, int lg) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) x[j][t] = *reinterpret_cast<const f32x4*>(xb + size_t(x3_square(t * 16 + l15)) * X3Block::C + (tile0 + j) * 16 + lg * 4);
}
template <int NJ>
__device__ __forceinline__ void x3_stream_store(const f32x4 (&x)[NJ][4], float* yb, int tile0, int l15, int lg) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(yb + size_t(x3_square(t * 16 + l15)) * X3Block::C + (tile0 + j) * 16 + lg * 4) = x[j][t];
}
template <int NJ>
__device__ __forceinline__ void x3_stream_add_bias(f32x4 (&x)[NJ][4], const float* b3, int tile0, int lg) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const f32x4 bs = *reinterpret_cast<const f32x4*>(b3 + (tile0 + j) * 16 + lg * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) x[j][t] += bs;
    }
}
template <int NJ>
__device__ __forceinline__ void x3_stream_write_tiles(const X3Tiles& T, const f32x4 (&x)[NJ][4], int tile0, int l15, int lg) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int co0 = (tile0 + j) * 16 + lg * 4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int rr = t * 16 + l15;
            const float v[4] = {x[j][t][0], x[j][t][1], x[j][t][2], x[j][t][3]};
            half4 h, l;
            split4(v, h, l);
            *reinterpret_cast<half4*>(T.xh + rr * X3Block::XROW + co0) = h;
            *reinterpret_cast<half4*>(T.xl + rr * X3Block::XROW + co0) = l;
        }
    }
}
// SE gate of a block on the stream in the registers (the waves that hold the stream; every other wave runs x3_se_gate_from_mean and a
// barrier beside it): squeeze from the registers -- the four square tiles, then the 16 lanes of the row -- the gate, x := x * gate (the
// residual uses the gated x, builder_util.py:473-475), the operand tiles rewritten.  scratch: the t2 tiles, idle between blocks.  Ends
// behind a barrier.
template <int NJ>
__device__ __forceinline__ void x3_stream_se(const X3Tiles& T, const X3TowerBlock& d, f32x4 (&x)[NJ][4], float* scratch, int tile0, int tid) {
    constexpr int GRP = 36;
    const int lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        float sum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[r] = (x[j][0][r] + x[j][1][r]) + (x[j][2][r] + x[j][3][r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sum[r] += dpp_mov<0x111>(sum[r]);    // row_shr:1
            sum[r] += dpp_mov<0x112>(sum[r]);    // row_shr:2
            sum[r] += dpp_mov<0x114>(sum[r]);    // row_shr:4
            sum[r] += dpp_mov<0x118>(sum[r]);    // row_shr:8 -> lane 15 of the row holds the row's sum
        }
        if (l15 == 15) {
            const int c = (tile0 + j) * 16 + lg * 4;                     // channel c at (c / 32) * 36 + c % 32
#pragma unroll
            for (int r = 0; r < 4; ++r) scratch[((c + r) >> 5) * GRP + ((c + r) & 31)] = sum[r] * (1.f / 64.f);
        }
    }
    x3_se_gate_from_mean(d, scratch, tid);
    const float* se_gate = scratch + 12 * GRP;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(se_gate + (tile0 + j) * 16 + lg * 4);
#pragma unroll
        for (int t = 0; t < 4; ++t) x[j][t] *= g;
    }
    x3_stream_write_tiles<NJ>(T, x, tile0, l15, lg);
    __syncthreads();
}
}  // namespace

}  // namespace cra
