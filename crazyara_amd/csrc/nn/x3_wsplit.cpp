// Precision float16x3, kernel family "-wsplit": the mobile-bottleneck block of a 128 / 192 / 224-channel net over several workgroups per
// board, for nets made for few boards (RiseNet::kBoardSplitMaxBatch).
//
// block_x3w_kernel (x3_wblock.cpp) runs such a block with one workgroup per board: a call of 8 boards occupies 8 of the chip's CUs and
// pays the whole latency of every block.  block_x3w_split_kernel<C, KS> is that kernel with block_x3_split_kernel's exchange (x3.hip,
// kernels.h: X3SplitArgs) -- G workgroups ("shares") per board, no atomics:
//   * grid: 8 G ceil(boards / 8) workgroups of 512 threads; id = xcd + 8 j, board = xcd + 8 (j / G), share = j % G: a board's shares sit
//     on one XCD, whose L2 fetches the board's images once; ids beyond the call's boards leave at once
//   * the first chunk's expand fragments of this share are requested before anything else
//   * stage: x = image 0 + image 1 + ... of the launch before (gin float images [64][C] per board, added in the order of their index in
//     f32: the same bits in every share and on every run; gin = 1: the float stream itself), times the SE gate a.blk.gate if the block
//     has one -> the hi / lo tiles
//   * share g runs the chunks [g n / G, (g + 1) n / G) of the block's n chunks (a 64-channel tail counts as one): expand, depthwise and
//     project are block_x3w_kernel's code -- the same k-slab order, lo*hi, hi*lo, hi*hi, the tail chunk on waves 0-3 with K = 64
//   * store: the share's partial project sums as a float image of its own, y_parts [B][G][64][C]; share 0 adds the BN3 bias and the
//     residual, x re-read as the same index-ordered f32 sum (L2-hot) times the gate -- block_x3w_kernel's epilogue expression, so that ONE
//     share gives block_x3w_kernel's bits
// Two image sets alternate between launches.  x3w_split_finish_kernel adds a block's images into the float stream (the same order of
// addition) for whatever reads the stream -- a transformer block, a gated block, the heads -- and, for a gated block, leaves the channel
// sums of that stream in block_x3w_kernel's order of addition (BlockArgs::pool_out), from which se_gate_w_kernel makes the gate.
// Every LDS word read is written first in the same launch (the map is block_x3w_kernel's); plain vector loads and stores only.
//
// The chunk code is a copy of block_x3w_kernel's, not a shared header: that kernel's listing stays what tests/test_x3_wblock.py reads.
#include "x3_device.h"

#include <algorithm>
#include <stdexcept>
#include <type_traits>

namespace cra {

namespace {
template <int C_, int KS_> struct X3WSplit {
    static_assert(C_ % 32 == 0 && C_ >= 128 && C_ < 256, "trunk widths 128 ... 224");
    static_assert(KS_ == 3 || KS_ == 5, "depthwise 3x3 or 5x5 (X3Depthwise / X3Depthwise5)");
    static constexpr int C = C_, KS = KS_, NW = 8, CK = 128, NTHR = 64 * NW;
    static constexpr int NT = C / 16;                        // cout tiles of the project GEMM
    static constexpr int NJ = (NT + NW - 1) / NW;            // per wave at most: tile w + 8 j
    static constexpr int NSLAB = C / 32;                     // k-slabs of the expand GEMM
    static constexpr int XROW = C + 16, TROW = CK + 16;      // halves; 32-byte row pad as X3Block
    static constexpr int REC = KS == 3 ? 256 : 512;          // floats of depthwise records per 16-channel tile
    // block_x3w_kernel's map: xh, xl [64][XROW]; t2h, t2l [2 buffers = chunk parity][64][TROW]; the waves' depthwise records [NW][REC]
    static constexpr size_t lds_bytes = (size_t(2) * 64 * XROW + size_t(4) * 64 * TROW) * sizeof(half_t) + size_t(NW) * REC * sizeof(float);
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
};

// n float values (8 or 4) at p as the sum of `gin` images `stride` floats apart, added in the order of their index; every load of the
// sum is requested before the first add (GIN > 0: a compile-time count)
template <int GIN, int N>
__device__ __forceinline__ void x3w_sum_images(const float* p, int gin, size_t stride, float (&f)[N]) {
    constexpr int NG = GIN > 0 ? GIN : kX3WSplitMaxG;
    float q[NG][N];
#pragma unroll
    for (int g = 0; g < NG; ++g)
        if (GIN > 0 || g < gin) {
            if constexpr (N == 8) load8<float>(p + size_t(g) * stride, q[g]);
            else load4<float>(p + size_t(g) * stride, q[g]);
        }
#pragma unroll
    for (int j = 0; j < N; ++j) f[j] = q[0][j];
#pragma unroll
    for (int g = 1; g < NG; ++g)
        if (GIN > 0 || g < gin) {
#pragma unroll
            for (int j = 0; j < N; ++j) f[j] += q[g][j];
        }
}
template <int N> __device__ __forceinline__ void x3w_sum_images_n(const float* p, int gin, size_t stride, float (&f)[N]) {
    switch (gin) {                                           // (the usual counts with every load in flight at once)
        case 1: x3w_sum_images<1, N>(p, 1, stride, f); break;
        case 2: x3w_sum_images<2, N>(p, 2, stride, f); break;
        case 3: x3w_sum_images<3, N>(p, 3, stride, f); break;
        case 4: x3w_sum_images<4, N>(p, 4, stride, f); break;
        default: x3w_sum_images<0, N>(p, gin, stride, f); break;
    }
}
}  // namespace

template <int C, int KS>
__global__ __launch_bounds__(512) void block_x3w_split_kernel(const X3WSplitArgs a) {
    using G = X3WSplit<C, KS>;
    constexpr int CK = G::CK, XROW = G::XROW, TROW = G::TROW, NT = G::NT, NJ = G::NJ, NSLAB = G::NSLAB, REC = G::REC;
    constexpr int EW = 4, PW = 2;                            // weight windows: expand k-slabs, project k-slabs in flight
    static_assert(NSLAB >= EW, "the expand window's first fill is EW k-slabs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* const xh = reinterpret_cast<half_t*>(smem);
    half_t* const xl = xh + 64 * XROW;
    half_t* const t2h_base = xl + 64 * XROW;
    half_t* const t2l_base = t2h_base + 2 * 64 * TROW;
    float* const dws = reinterpret_cast<float*>(t2l_base + 2 * 64 * TROW);
    // workgroup -> (board, share), block_x3_split_kernel's placement: board b lives on XCD b % 8
    const int G_ = a.G, gin = a.gin;
    const int xcd = blockIdx.x & 7, jj = blockIdx.x >> 3;
    const int g = __builtin_amdgcn_readfirstlane(jj % G_), b = __builtin_amdgcn_readfirstlane(xcd + 8 * (jj / G_));
    if (b >= a.blk.batch) return;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane_off = uint32_t(lane) * 16u;
    const X3Weights W = x3_weights(a.blk.w1pk, a.blk.w1pk_lo, a.blk.w3pk, a.blk.w3pk_lo, a.blk.dwpk, a.blk.cop_pad);
    const int nfull = W.cop_pad / CK;                        // chunks of 128 channels
    const bool tail = (W.cop_pad & (CK - 1)) != 0;           // + one of 64 (cop_pad is a multiple of 64)
    const int nchunk = nfull + (tail ? 1 : 0);
    const int ch0 = g * nchunk / G_, ch1 = (g + 1) * nchunk / G_;      // this share's chunks (G <= nchunk: at least one)
    const int nslab3 = W.cop_pad >> 5;
    const bool has2 = NJ == 2 && w + 8 < NT;                 // this wave owns a second cout tile
    auto expands = [&](int ch) { return ch < nfull || w < 4; };     // a tail chunk's four tiles are waves 0-3's

    const size_t image = size_t(64) * C;
    const float* const xb = a.x_parts + size_t(b) * gin * image;
    const float* const gate = a.blk.gate ? a.blk.gate + size_t(b) * C : nullptr;

    // expand weight window: EW of the k-slabs of this wave's tile (hi, lo); slab s sits in slot s % EW and is refilled with slab s + EW
    // right behind its MFMAs; the first EW slabs of a chunk are requested a project phase ahead (the share's first: before the board is staged)
    half8 e_h[EW], e_l[EW];
    auto load_expand = [&](int ch, int s) {
        const uint32_t f = uint32_t(ch * (CK / 16) + w) * uint32_t(NSLAB) + uint32_t(s);
        e_h[s % EW] = x3_frag(W.w1h, lane_off, f);
        e_l[s % EW] = x3_frag(W.w1l, lane_off, f);
    };
    if (expands(ch0)) {
#pragma unroll
        for (int s = 0; s < EW; ++s) load_expand(ch0, s);
    }

    // stage: the board as the index-ordered sum of its images (x := x * gate[c] if the block has an SE gate) -> split tiles
#pragma unroll 1
    for (int i = tid; i < 64 * (C / 8); i += G::NTHR) {
        const int sq = i / (C / 8), v = i - sq * (C / 8), r = x3_row(sq);
        float f[8];
        x3w_sum_images_n<8>(xb + size_t(sq) * C + v * 8, gin, image, f);
        if (gate) {
            float gv[8];
            load8<float>(gate + v * 8, gv);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= gv[j];
        }
        half8 h, l;
        split8(f, h, l);
        *reinterpret_cast<half8*>(xh + r * XROW + v * 8) = h;
        *reinterpret_cast<half8*>(xl + r * XROW + v * 8) = l;
    }
    __syncthreads();

    f32x4 accP[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) accP[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool hi = l15 >= 8;                                // the tile's second rank (t + 4, x3_row)
    float* const my_dws = dws + w * REC;

    // One chunk: E and D of this wave's tile, the barrier, P.  TAIL: the 64-channel chunk -- waves 4-7 have no tile, P has two k-slabs.
    auto chunk = [&](auto tail_c, int ch) {
        constexpr bool TAIL = decltype(tail_c)::value;
        constexpr int NS2 = TAIL ? CK / 64 : CK / 32;
        half_t* const t2h = t2h_base + (ch & 1) * 64 * TROW;
        half_t* const t2l = t2l_base + (ch & 1) * 64 * TROW;
        half8 bh[2][4], bl[2][4];
        // project weight window: PW of the chunk's k-slabs x this wave's cout tiles (hi, lo); the first PW are requested between E and D
        half8 p_h[PW][NJ], p_l[PW][NJ];
        auto load_project = [&](int s2) {                     // cout tile w + 8 j, K slab ch * 4 + s2
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j == 1 && !has2) continue;
                const uint32_t f = uint32_t(w + 8 * j) * uint32_t(nslab3) + uint32_t(ch * (CK / 32) + s2);
                p_h[s2 % PW][j] = x3_frag(W.w3h, lane_off, f);
                p_l[s2 % PW][j] = x3_frag(W.w3l, lane_off, f);
            }
        };
        if (!TAIL || w < 4) {
            // ---------------- E: expand, 16 channels x 64 squares, K = C ----------------
            f32x4 accE[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) accE[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            // the tile's depthwise records: 16-byte loads per lane, parked in the wave's LDS scratch half-way through the MFMAs (the
            // wave's depthwise of the chunk before is through with them) and read back per lane as broadcast reads
            f32x4 dw_raw[REC / 256];
#pragma unroll
            for (int h2 = 0; h2 < REC / 256; ++h2)
                dw_raw[h2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.dw, lane_off, uint32_t(ch * (CK / 16) + w) * uint32_t(REC * 4) + uint32_t(h2) * 1024u, 0));
            // A slab = 12 MFMAs on the stream fragments of one k-slab.  The NEXT slab's fragments are read from LDS before this slab's
            // MFMAs issue and the window refills right behind them; the fences keep the scheduler from sinking either (x3_chunks).
            auto read_stream = [&](int s, half8 (&h)[4], half8 (&l)[4]) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    h[t] = *reinterpret_cast<const half8*>(xh + (t * 16 + l15) * XROW + s * 32 + lg * 8);
                    l[t] = *reinterpret_cast<const half8*>(xl + (t * 16 + l15) * XROW + s * 32 + lg * 8);
                }
            };
            read_stream(0, bh[0], bl[0]);
#pragma unroll
            for (int s = 0; s < NSLAB; ++s) {
                if (s + 1 < NSLAB) read_stream(s + 1, bh[(s + 1) & 1], bl[(s + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(e_l[s % EW], bh[s & 1][t], accE[t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(e_h[s % EW], bl[s & 1][t], accE[t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(e_h[s % EW], bh[s & 1][t], accE[t], true);
                if (s + EW < NSLAB) load_expand(ch, s + EW);
                if (s == NSLAB / 2) {
#pragma unroll
                    for (int h2 = 0; h2 < REC / 256; ++h2) *reinterpret_cast<f32x4*>(my_dws + h2 * 256 + lane * 4) = dw_raw[h2];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int s2 = 0; s2 < PW; ++s2) load_project(s2);   // they land while the depthwise runs
            // ---------------- D: BN1 + ReLU, depthwise on the accumulators, BN2 + ReLU, exact f32; split -> t2 ----------------
            float outv[4][4];                                   // [tile][channel r]
            if constexpr (KS == 3) {
                x3_depthwise(accE, my_dws, lg, hi, x3_edge_offsets(l15), outv);
            } else {
                X3Depthwise5 dw5;
                const X3EdgeOffsets5 edge5 = x3_edge_offsets5(l15);
                // (a fence per channel: unfenced, the scheduler hoists all four channels' 27 record reads and the kernel spills)
                dw5.template load<0>(my_dws, lg, edge5); dw5.template gather<0>(accE, hi, 1.f); dw5.template taps<0>();
                __builtin_amdgcn_sched_barrier(0);
                dw5.template load<1>(my_dws, lg, edge5); dw5.template gather<1>(accE, hi, 1.f); dw5.template taps<1>();
                __builtin_amdgcn_sched_barrier(0);
                dw5.template load<2>(my_dws, lg, edge5); dw5.template gather<2>(accE, hi, 1.f); dw5.template taps<2>();
                __builtin_amdgcn_sched_barrier(0);
                dw5.template load<3>(my_dws, lg, edge5); dw5.template gather<3>(accE, hi, 1.f); dw5.template taps<3>();
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) outv[t][r] = dw5.outv[t][r];
            }
            const int cl = w * 16 + lg * 4;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                half4 h, l;
                split4(outv[t], h, l);
                *reinterpret_cast<half4*>(t2h + (t * 16 + l15) * TROW + cl) = h;
                *reinterpret_cast<half4*>(t2l + (t * 16 + l15) * TROW + cl) = l;
            }
        } else {
#pragma unroll
            for (int s2 = 0; s2 < PW; ++s2) load_project(s2);
        }
        __syncthreads();
        if (ch + 1 < ch1 && expands(ch + 1)) {                  // the share's next chunk: its first expand slabs land while the project MFMAs run
#pragma unroll
            for (int s = 0; s < EW; ++s) load_expand(ch + 1, s);
        }
        // ---------------- P: project, this wave's cout tiles x 64 squares, K = 128 (TAIL: 64), accumulates over the chunks ----------------
        auto read_t2 = [&](int s2, half8 (&h)[4], half8 (&l)[4]) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                h[t] = *reinterpret_cast<const half8*>(t2h + (t * 16 + l15) * TROW + s2 * 32 + lg * 8);
                l[t] = *reinterpret_cast<const half8*>(t2l + (t * 16 + l15) * TROW + s2 * 32 + lg * 8);
            }
        };
        read_t2(0, bh[0], bl[0]);
#pragma unroll
        for (int s2 = 0; s2 < NS2; ++s2) {
            if (s2 + 1 < NS2) read_t2(s2 + 1, bh[(s2 + 1) & 1], bl[(s2 + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j == 1 && !has2) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(p_l[s2 % PW][j], bh[s2 & 1][t], accP[j][t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(p_h[s2 % PW][j], bl[s2 & 1][t], accP[j][t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(p_h[s2 % PW][j], bh[s2 & 1][t], accP[j][t], true);
            }
            if (s2 + PW < NS2) load_project(s2 + PW);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    const int full1 = ch1 < nfull ? ch1 : nfull;
    for (int ch = ch0; ch < full1; ++ch) chunk(std::false_type{}, ch);
    if (tail && ch1 == nchunk) chunk(std::true_type{}, nfull);

    // ---------------- epilogue: this share's image; share 0 carries the BN3 bias and the residual (the board's f32 sum again, times the gate) ----------------
    float* const yb = a.y_parts + (size_t(b) * G_ + g) * image;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j == 1 && !has2) continue;
        const int co0 = (w + 8 * j) * 16 + lg * 4;
        if (g == 0) {
            float bs[4], gv[4] = {1.f, 1.f, 1.f, 1.f};
            load4<float>(a.blk.b3 + co0, bs);
            if (gate) load4<float>(gate + co0, gv);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sq = x3_square(t * 16 + l15);
                float xr[4], v[4];
                x3w_sum_images_n<4>(xb + size_t(sq) * C + co0, gin, image, xr);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = accP[j][t][r] + bs[r] + xr[r] * gv[r];
                store4<float>(yb + size_t(sq) * C + co0, v);
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sq = x3_square(t * 16 + l15);
                const float v[4] = {accP[j][t][0], accP[j][t][1], accP[j][t][2], accP[j][t][3]};
                store4<float>(yb + size_t(sq) * C + co0, v);
            }
        }
    }
}

// A block's images -> the float stream y [B][64][C] (the staging's order of addition), and with pool_out the stream's channel sums
// [B][C] for the next block's SE gate.  One wave per board and 16-channel tile, a lane at block_x3w_kernel's epilogue position
// (channels tile * 16 + lg * 4 ..., squares x3_square(t * 16 + l15)): the sums over the squares are added in that kernel's order, so
// that the images of ONE share give its BlockArgs::pool_out bit for bit.
__global__ __launch_bounds__(256) void x3w_split_finish_kernel(const float* __restrict__ parts, int gin, float* __restrict__ y, float* __restrict__ pool_out, int batch, int C) {
    const int tiles = C / 16;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= batch * tiles) return;
    const int b = wv / tiles, tile = wv - b * tiles;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int co0 = tile * 16 + lg * 4;
    const size_t image = size_t(64) * C;
    const float* const xb = parts + size_t(b) * gin * image;
    float* const yb = y + size_t(b) * image;
    float pool[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int sq = x3_square(t * 16 + l15);
        float v[4];
        x3w_sum_images_n<4>(xb + size_t(sq) * C + co0, gin, image, v);
#pragma unroll
        for (int r = 0; r < 4; ++r) pool[r] += v[r];
        store4<float>(yb + size_t(sq) * C + co0, v);
    }
    if (pool_out) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) pool[r] += __shfl_xor(pool[r], off, 64);
        if (l15 == 0) store4<float>(pool_out + size_t(b) * C + co0, pool);
    }
}

namespace {
template <int C, int KS> void init_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&block_x3w_split_kernel<C, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, int(X3WSplit<C, KS>::lds_bytes));
}
template <int C, int KS> void launch_one(const X3WSplitArgs& a, hipStream_t s) {
    using G = X3WSplit<C, KS>;
    hipLaunchKernelGGL((block_x3w_split_kernel<C, KS>), dim3(8 * a.G * ((a.blk.batch + 7) / 8)), dim3(G::NTHR), G::lds_bytes, s, a);
}
template <int C> void launch_width(const X3WSplitArgs& a, hipStream_t s) {
    if (a.blk.ks == 5) launch_one<C, 5>(a, s);
    else launch_one<C, 3>(a, s);
}
}  // namespace

int x3w_split_chunks(int cop_pad) { return (cop_pad + 127) / 128; }

int x3w_split_shares(int cop_pad, int boards, int cu_count) {
    return std::max(1, std::min(std::min(x3w_split_chunks(cop_pad), int(kX3WSplitMaxG)), cu_count / std::max(1, boards)));
}

void init_x3_wsplit_kernel_attributes() {
    init_one<128, 3>(); init_one<128, 5>();
    init_one<192, 3>(); init_one<192, 5>();
    init_one<224, 3>(); init_one<224, 5>();
}

void launch_block_x3w_split(const X3WSplitArgs& a, hipStream_t s) {
    if (!block_x3w_supports(a.blk.C, a.blk.ks) || a.blk.cop_pad % 64 != 0 || a.blk.cop_pad <= 0) throw std::invalid_argument("launch_block_x3w_split: no kernel for this block");
    if (a.G < 1 || a.G > x3w_split_chunks(a.blk.cop_pad) || a.G > kX3WSplitMaxG || a.gin < 1 || a.gin > kX3WSplitMaxG)
        throw std::invalid_argument("block_x3w_split: 1 <= G <= min(chunks, 8), 1 <= gin <= 8");
    if (a.blk.batch < 1) throw std::invalid_argument("block_x3w_split: no boards");
    if (a.blk.C == 128) launch_width<128>(a, s);
    else if (a.blk.C == 192) launch_width<192>(a, s);
    else launch_width<224>(a, s);
}

void launch_x3w_split_finish(const float* parts, int gin, float* y, float* pool_out, int batch, int C, hipStream_t s) {
    if (gin < 1 || gin > kX3WSplitMaxG || C % 16 != 0 || batch < 1) throw std::invalid_argument("x3w_split_finish: 1 <= gin <= 8, C a multiple of 16");
    const int waves = batch * (C / 16);
    hipLaunchKernelGGL(x3w_split_finish_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, parts, gin, y, pool_out, batch, C);
}

}  // namespace cra
