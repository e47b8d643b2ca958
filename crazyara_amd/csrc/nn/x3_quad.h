// Device helpers of tower_x3_quad_kernel (x3_quad.cpp), the float16x3 two-role tower whose EXPAND waves hold their accumulators
// TRANSPOSED: the expand MFMA takes the x fragment as A and the weight fragment as B, so a lane holds ONE channel (l15 of the 16-channel
// tile) on a 4 x 4 quadrant of the board -- accumulator [tile t][register r] is rank 4 * (lg >> 1) + t, file 4 * (lg & 1) + r, which is
// what the tile row order of x3_device.h (x3_row) already gives for row 4 * lg + r of tile t.  The nine taps of the depthwise are then
// plain v_fmac_f32 on the lane's own registers; only a halo of 4 + 4 + 1 values crosses lanes (X3DepthwiseQuad).
//
// The first part of this header is plain C++ (the index maps, constexpr: scripts/studies/x3_quad_maps.cpp prints them for
// tests/test_x3_quad_maps.py); the device part needs x3_device.h in front of it.
#pragma once

namespace cra {

// ---- index maps (host-callable) ----
// square (rank * 8 + file) <-> row of the board tiles in LDS; the same map as x3_device.h's x3_row / x3_square
constexpr int x3q_row(int sq) { return ((sq >> 3) & 3) * 16 + (sq >> 5) * 8 + (sq & 7); }
constexpr int x3q_square(int row) { return ((row >> 4) + 4 * ((row >> 3) & 1)) * 8 + (row & 7); }
// the square of an EXPAND lane's accumulator: tile t, lane group lg, register r (D row 4 * lg + r of the MFMA with x as A)
constexpr int x3q_lane_square(int t, int lg, int r) { return (4 * (lg >> 1) + t) * 8 + 4 * (lg & 1) + r; }

// t2T[channel][square row]: the depthwise output of a 128-channel chunk, f16, 64 halves (128 bytes) per channel and no padding.
// A channel's row is 16 units of 4 rows (8 bytes: what an EXPAND lane stores at once, and what a lane of the transposed read names);
// unit u of channel c lies at unit u ^ x3q_swizzle(c).  With it
//   * the store (ds_write_b64, 16-lane groups = the 16 channels of a tile at one u) covers 16 different units = all 32 banks once;
//   * the transposed read (ds_read_b64_tr_b16, 32-lane halves = channels {0-3, 8-11} + 4 hh of a k-slab, units 4 t ... 4 t + 3) covers
//     the 64 banks once: odd and even channels are 32 banks apart, bits 1 and 3 of the channel pick the 8-bank band.
constexpr int X3Q_T2T_ROW = 64;                                  // halves per channel
constexpr int X3Q_T2T_HALVES = 128 * X3Q_T2T_ROW;                // per buffer (hi or lo, one chunk parity): 16 KiB of the 18 KiB the [64][144] tile has
constexpr int x3q_swizzle(int c) { return (c & 1) | (((c >> 2) & 1) << 1) | (((c >> 1) & 1) << 2) | (c & 8); }
constexpr int x3q_t2t_offset(int c, int row) { return c * X3Q_T2T_ROW + 4 * ((row >> 2) ^ x3q_swizzle(c & 15)) + (row & 3); }   // in halves
// store side: EXPAND lane (l15, lg) puts rows t * 16 + 4 lg ... + 3 of channel tile * 16 + l15 (one half4)
constexpr int x3q_store_offset(int tile, int l15, int lg, int t) { return x3q_t2t_offset(tile * 16 + l15, t * 16 + 4 * lg); }
// read side: the address PROJECT lane (l15, lg) supplies to the transposed read of k-slab s2, half hh (k = 8 lg + 4 hh ... + 3), square
// tile t: lane 4 q + p of a 16-lane group names channel q of the four and rows 4 p ... 4 p + 3; lane i receives row i of the four channels
constexpr int x3q_read_offset(int s2, int hh, int t, int l15, int lg) { return x3q_t2t_offset(s2 * 32 + lg * 8 + hh * 4 + (l15 >> 2), t * 16 + 4 * (l15 & 3)); }

}  // namespace cra

#ifdef __HIPCC__
namespace cra {
namespace {

// Lane constants of the quadrant depthwise.  A quadrant has ONE horizontal neighbour (lane group lg ^ 1), ONE vertical (lg ^ 2) and ONE
// diagonal (lg ^ 3); its other two sides are board edges.  The halo registers H (a column), V (a row) and K (the corner) therefore stand
// on BOTH sides of the quadrant, and the side that is a board edge reads its weights from the record's zero rows (the zero-rows trick of
// x3_edge_offsets): offsets in floats from a record row to a zero row (11 ... 15), or 0 where the neighbour exists.
struct X3QuadOffsets {
    int hl, hr;             // H as the left column (rows 0-2, real for odd lg) / the right column (rows 6-8, real for even lg)
    int vt, vt6;            // V as the row above (rows 0, 3 | row 6; real for lg >= 2)
    int vb2, vb;            // V as the row below (row 2 | rows 5, 8; real for lg < 2)
    int k0, k6, k2, k8;     // K as the corner above left (lg 3), above right (lg 2), below left (lg 1), below right (lg 0)
    int to_v, to_k;         // ds_bpermute addresses of lanes lane ^ 32 and lane ^ 48
};
__device__ __forceinline__ X3QuadOffsets x3_quad_offsets(int lane) {
    const int lg = lane >> 4;
    const bool odd = (lg & 1) != 0, hi = lg >= 2;
    X3QuadOffsets o;
    o.hl = odd ? 0 : 11 * 16;
    o.hr = odd ? 5 * 16 : 0;
    o.vt = hi ? 0 : 11 * 16;
    o.vt6 = hi ? 0 : 5 * 16;
    o.vb2 = hi ? 11 * 16 : 0;
    o.vb = hi ? 6 * 16 : 0;
    o.k0 = lg == 3 ? 0 : 11 * 16;
    o.k6 = lg == 2 ? 0 : 5 * 16;
    o.k2 = lg == 1 ? 0 : 11 * 16;
    o.k8 = lg == 0 ? 0 : 5 * 16;
    o.to_v = (lane ^ 32) * 4;
    o.to_k = (lane ^ 48) * 4;
    return o;
}

// D of one 16-channel tile on transposed accumulators: acc[t][r] = channel l15 at rank 4 (lg >> 1) + t, file 4 (lg & 1) + r.  BN1 bias +
// ReLU, depthwise 3x3, BN2 bias + ReLU: per output the arithmetic and the tap order of X3Depthwise::taps (per dy: left, middle, right),
// so every output has the bits it has there.  Lane moves: none in the taps; the halo goes through the LDS crossbar (ds_swizzle /
// ds_bpermute, no VALU issue slot -- the EXPAND wave's limit) behind one select per value that picks what the neighbour needs.
// In pieces (load, gather, taps_rank<T>) so that a caller can spread them over a stretch of MFMAs.
//   rec: this tile's records in LDS, [16 rows: taps dx = -1 (dy = -1, 0, 1), dx = 0, dx = +1, BN1 bias, BN2 bias, 5 rows of zeros][16 channels]
struct X3DepthwiseQuad {
    float w[11];                     // the channel's records
    float whl[3], whr[3];            // column dx = -1 / + 1 for H (by dy)
    float wvt[3], wvb[3];            // row dy = -1 / + 1 for V (by dx)
    float wk[4];                     // corners: above left, above right, below left, below right
    float S[4][4], H[4], V[4], K;
    float outv[4][4];                // [tile t][file r]

    __device__ __forceinline__ void load(const float* rec, int l15, const X3QuadOffsets& o) {
        const float* p = rec + l15;
#pragma unroll
        for (int q = 0; q < 11; ++q) w[q] = p[q * 16];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            whl[d] = p[o.hl + d * 16];
            whr[d] = p[o.hr + (6 + d) * 16];
            wvt[d] = p[(d == 2 ? o.vt6 : o.vt) + 3 * d * 16];
            wvb[d] = p[(d == 0 ? o.vb2 : o.vb) + (3 * d + 2) * 16];
        }
        wk[0] = p[o.k0];
        wk[1] = p[o.k6 + 6 * 16];
        wk[2] = p[o.k2 + 2 * 16];
        wk[3] = p[o.k8 + 8 * 16];
    }
    __device__ __forceinline__ void gather(const f32x4 (&acc)[4], int lg, const X3QuadOffsets& o) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[t][r] = (X3_ABL & 1) ? acc[t][r] + w[0] : fmaxf(acc[t][r] + w[9], 0.f);
        if constexpr (X3_ABL & 1) return;
        const bool odd = (lg & 1) != 0, hi = lg >= 2;
        float sh[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            sh[t] = odd ? S[t][0] : S[t][3];                                 // what the horizontal neighbour sees of this quadrant
            H[t] = __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, sh[t]), 0x401f));    // lane ^ 16
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sv = hi ? S[0][r] : S[3][r];
            V[r] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(o.to_v, __builtin_bit_cast(int, sv)));
        }
        const float sk = hi ? sh[0] : sh[3];
        K = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(o.to_k, __builtin_bit_cast(int, sk)));
    }
    // value and weight of the tap at (y, x) of the padded quadrant, y, x = -1 ... 4; q = the record row of the tap (3 * (dx + 1) + dy + 1)
    template <int Y, int X, int Q> __device__ __forceinline__ float tap(float a) const {
        constexpr int DX = Q / 3, DY = Q % 3;
        if constexpr (Y >= 0 && Y < 4 && X >= 0 && X < 4) return fmaf(w[Q], S[Y][X], a);
        else if constexpr (Y >= 0 && Y < 4) return fmaf(X < 0 ? whl[DY] : whr[DY], H[Y], a);
        else if constexpr (X >= 0 && X < 4) return fmaf(Y < 0 ? wvt[DX] : wvb[DX], V[X], a);
        else return fmaf(wk[(Y < 0 ? 0 : 2) + (X < 0 ? 0 : 1)], K, a);
    }
    template <int T, int R> __device__ __forceinline__ void output() {
        if constexpr (X3_ABL & 1) {
            outv[T][R] = S[T][R];
            return;
        }
        float a = w[10];
        a = tap<T - 1, R - 1, 0>(a); a = tap<T - 1, R, 3>(a); a = tap<T - 1, R + 1, 6>(a);
        a = tap<T, R - 1, 1>(a);     a = tap<T, R, 4>(a);     a = tap<T, R + 1, 7>(a);
        a = tap<T + 1, R - 1, 2>(a); a = tap<T + 1, R, 5>(a); a = tap<T + 1, R + 1, 8>(a);
        outv[T][R] = fmaxf(a, 0.f);
    }
    template <int T> __device__ __forceinline__ void taps_rank() {
        output<T, 0>(); output<T, 1>(); output<T, 2>(); output<T, 3>();
    }
    // keeps the values computed so far where they were written (a piece set between MFMAs is otherwise sunk to its first use)
    template <int T> __device__ __forceinline__ void pin_rank() {
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(outv[T][r]));
    }
};

// One 8-byte transposed read: four consecutive rows (squares) of four channels, the lane's row of each channel (x3q_read_offset)
typedef __fp16 x3q_f16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ half8 x3q_read_fragment(const half_t* lo4, const half_t* hi4) {
    typedef __attribute__((address_space(3))) x3q_f16x4 lds_f16x4;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x2 a = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_f16x4*)(lo4)));
    const u32x2 b = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_f16x4*)(hi4)));
    return __builtin_bit_cast(half8, u32x4{a.x, a.y, b.x, b.y});
}

}  // namespace
}  // namespace cra
#endif
