// Precision float16x3, kernel family "-wblock": the one-launch mobile-bottleneck block at trunk widths other than 256.
//
// block_x3_kernel (x3.hip) runs a 3x3 block of a 256-channel net in one launch: expand (three f16 MFMAs per product on hi / lo split
// operands) -> BN1 + ReLU + depthwise + BN2 + ReLU in exact f32 on the accumulators -> split -> LDS -> project -> + BN3 bias + x.  It is
// fixed at C = 256.  block_x3w_kernel<C, KS> is its sibling for C = 128 / 192 / 224 (AlphaVile's trunks) with both depthwise sizes:
//   * one workgroup per board, 8 waves; the board is staged as hi / lo f16 tiles [64][C + 16] (optionally times the SE gate a.gate)
//   * C_op runs in chunks of 128 channels: wave w expands cout tile chunk * 8 + w (K = C: C / 32 k-slabs of 12 MFMAs, x3_mfma's order
//     lo*hi, hi*lo, hi*hi), runs that tile's depthwise (x3_depthwise / X3Depthwise5) and writes 16 columns of the chunk's t2 pair; one
//     barrier; then every wave projects the chunk (K = 128) onto its cout tiles, accumulating over the chunks
//   * cout tiles of the project GEMM: tile w + 8 j, j < NJ = ceil(C / 128).  j = 0 is every wave's; j = 1 exists for w < C / 16 - 8
//     (a wave-uniform guard): at 192 waves 0-3 own two tiles -- one wave per SIMD, the four SIMDs carry 3 tiles each --, at 224 waves 0-5
//     (SIMDs 0 and 1 carry 4 tiles, SIMDs 2 and 3 carry 3), at 128 NJ = 1.  Of the NJ * 8 tile slots of the project phase 0 / 25 % /
//     12.5 % idle at 128 / 192 / 224.
//   * the packers pad C_op to a multiple of 64, not of 128: a block whose last chunk holds 64 channels (C_op = 64, 320, 448) runs it
//     as a TAIL chunk -- waves 0-3 expand and run the depthwise of one tile each, waves 4-7 go straight to the barrier, the project
//     phase has K = 64 (two k-slabs).  The padded half does not exist in the weight images: no fragment of it can be requested.
//   * the epilogue re-reads the board's f32 tile (L2-hot) for the residual, x (* gate) in exact f32 as the layer kernels add it, adds
//     the BN3 bias, stores f32 and, with a.pool_out, leaves the channel sums of the output for the next block's SE gate.
// se_gate_w_kernel turns those sums into the gate at any width (se_gate_kernel, kernels.hip, is fixed at 256): se_kernel's arithmetic.
//
// Why this file is a .cpp: see x3_tail.cpp -- tests/test_experts_isa.py pins the kernels of the .hip listings and allows no new ones
// there; build.sources() compiles .cpp as HIP.  Nothing in x3_device.h that an existing kernel uses is changed; the width-generic
// pieces live here.
#include "x3_device.h"

#include <stdexcept>
#include <type_traits>

namespace cra {

namespace {
template <int C_, int KS_> struct X3WBlock {
    static_assert(C_ % 32 == 0 && C_ >= 128 && C_ < 256, "trunk widths 128 ... 224 (256 is block_x3_kernel's)");
    static_assert(KS_ == 3 || KS_ == 5, "depthwise 3x3 or 5x5 (X3Depthwise / X3Depthwise5)");
    static constexpr int C = C_, KS = KS_, NW = 8, CK = 128, NTHR = 64 * NW;
    static constexpr int NT = C / 16;                        // cout tiles of the project GEMM
    static constexpr int NJ = (NT + NW - 1) / NW;            // per wave at most: tile w + 8 j
    static constexpr int NSLAB = C / 32;                     // k-slabs of the expand GEMM
    static constexpr int XROW = C + 16, TROW = CK + 16;      // halves; 32-byte row pad as X3Block
    static constexpr int REC = KS == 3 ? 256 : 512;          // floats of depthwise records per 16-channel tile
    // xh, xl [64][XROW]; t2h, t2l [2 buffers = chunk parity][64][TROW]; the waves' depthwise records [NW][REC]
    static constexpr size_t lds_bytes = (size_t(2) * 64 * XROW + size_t(4) * 64 * TROW) * sizeof(half_t) + size_t(NW) * REC * sizeof(float);
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
};
}  // namespace

template <int C, int KS>
__global__ __launch_bounds__(512) void block_x3w_kernel(const BlockArgs a) {
    using G = X3WBlock<C, KS>;
    constexpr int CK = G::CK, XROW = G::XROW, TROW = G::TROW, NT = G::NT, NJ = G::NJ, NSLAB = G::NSLAB, REC = G::REC;
    constexpr int EW = 4, PW = 2;                            // weight windows: expand k-slabs, project k-slabs in flight
    static_assert(NSLAB >= EW, "the expand window's first fill is EW k-slabs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* const xh = reinterpret_cast<half_t*>(smem);
    half_t* const xl = xh + 64 * XROW;
    half_t* const t2h_base = xl + 64 * XROW;
    half_t* const t2l_base = t2h_base + 2 * 64 * TROW;
    float* const dws = reinterpret_cast<float*>(t2l_base + 2 * 64 * TROW);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane_off = uint32_t(lane) * 16u;
    const X3Weights W = x3_weights(a.w1pk, a.w1pk_lo, a.w3pk, a.w3pk_lo, a.dwpk, a.cop_pad);
    const int nfull = W.cop_pad / CK;                        // chunks of 128 channels
    const bool tail = (W.cop_pad & (CK - 1)) != 0;           // + one of 64 (cop_pad is a multiple of 64)
    const int nchunk = nfull + (tail ? 1 : 0);
    const int nslab3 = W.cop_pad >> 5;
    const bool has2 = NJ == 2 && w + 8 < NT;                 // this wave owns a second cout tile
    auto expands = [&](int ch) { return ch < nfull || w < 4; };     // a tail chunk's four tiles are waves 0-3's

    const float* const xb = reinterpret_cast<const float*>(a.x) + size_t(b) * 64 * C;
    const float* const gate = a.gate ? a.gate + size_t(b) * C : nullptr;

    // expand weight window: EW of the k-slabs of this wave's tile (hi, lo); slab s sits in slot s % EW and is refilled with slab s + EW
    // right behind its MFMAs; the first EW slabs of a chunk are requested a project phase ahead (chunk 0: before the board is staged)
    half8 e_h[EW], e_l[EW];
    auto load_expand = [&](int ch, int s) {
        const uint32_t f = uint32_t(ch * (CK / 16) + w) * uint32_t(NSLAB) + uint32_t(s);
        e_h[s % EW] = x3_frag(W.w1h, lane_off, f);
        e_l[s % EW] = x3_frag(W.w1l, lane_off, f);
    };
    if (expands(0)) {
#pragma unroll
        for (int s = 0; s < EW; ++s) load_expand(0, s);
    }

    // stage: float board tile [64][C] (x := x * gate[c] if the block has an SE gate) -> split tiles
#pragma unroll 1
    for (int i = tid; i < 64 * (C / 8); i += G::NTHR) {
        const int sq = i / (C / 8), v = i - sq * (C / 8), r = x3_row(sq);
        float f[8];
        load8<float>(xb + size_t(sq) * C + v * 8, f);
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
        if (ch + 1 < nchunk && expands(ch + 1)) {               // the next chunk's first expand slabs land while the project MFMAs run
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
    for (int ch = 0; ch < nfull; ++ch) chunk(std::false_type{}, ch);
    if (tail) chunk(std::true_type{}, nfull);

    // ---------------- epilogue: + BN3 bias + residual (the board's f32 tile again, times the gate: the value the layer kernels add) ----------------
    float* const yb = reinterpret_cast<float*>(a.y) + size_t(b) * 64 * C;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j == 1 && !has2) continue;
        const int co0 = (w + 8 * j) * 16 + lg * 4;
        float bs[4], gv[4] = {1.f, 1.f, 1.f, 1.f};
        load4<float>(a.b3 + co0, bs);
        if (gate) load4<float>(gate + co0, gv);
        float pool[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = x3_square(t * 16 + l15);
            float xr[4], v[4];
            load4<float>(xb + size_t(sq) * C + co0, xr);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = accP[j][t][r] + bs[r] + xr[r] * gv[r];
                pool[r] += v[r];
            }
            store4<float>(yb + size_t(sq) * C + co0, v);
        }
        if (a.pool_out) {                                       // squeeze (AdaptiveAvgPool2d) of the block output, fused here
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) pool[r] += __shfl_xor(pool[r], off, 64);
            if (l15 == 0) store4<float>(a.pool_out + size_t(b) * C + co0, pool);
        }
    }
}

// The SE gate from a block's channel sums at any trunk width: gate[b][c] from pool[b][c] = sum over the 64 squares.  se_kernel's
// arithmetic (kernels.hip) on the pooled sums: kind 1 ca_se (two bias-free FCs, ReLU between), 2 eca_se (centre-tap linear + bias),
// hard-sigmoid.  One workgroup per board.
__global__ __launch_bounds__(256) void se_gate_w_kernel(const float* __restrict__ pool, float* __restrict__ gate, int kind, const float* __restrict__ w1t,
                                                        const float* __restrict__ w2t, const float* __restrict__ b1, int C) {
    __shared__ float s_mean[512];
    __shared__ float s_h[256];
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += 256) s_mean[c] = pool[size_t(blockIdx.x) * C + c] * (1.f / 64.f);
    __syncthreads();
    float* const g = gate + size_t(blockIdx.x) * C;
    if (kind == 1) {
        const int H = C / 2;
        for (int j = tid; j < H; j += 256) {
            float sum = 0.f;
            for (int c = 0; c < C; ++c) sum = fmaf(w1t[size_t(c) * H + j], s_mean[c], sum);
            s_h[j] = fmaxf(sum, 0.f);
        }
        __syncthreads();
        for (int c = tid; c < C; c += 256) {
            float sum = 0.f;
            for (int j = 0; j < H; ++j) sum = fmaf(w2t[size_t(j) * C + c], s_h[j], sum);
            g[c] = hard_sigmoid(sum);
        }
    } else {
        for (int c = tid; c < C; c += 256) {
            float sum = b1[c];
            for (int i = 0; i < C; ++i) sum = fmaf(w1t[size_t(i) * C + c], s_mean[i], sum);
            g[c] = hard_sigmoid(sum);
        }
    }
}

namespace {
template <int C, int KS> void init_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&block_x3w_kernel<C, KS>), hipFuncAttributeMaxDynamicSharedMemorySize, int(X3WBlock<C, KS>::lds_bytes));
}
template <int C, int KS> void launch_one(const BlockArgs& a, hipStream_t s) {
    using G = X3WBlock<C, KS>;
    hipLaunchKernelGGL((block_x3w_kernel<C, KS>), dim3(a.batch), dim3(G::NTHR), G::lds_bytes, s, a);
}
template <int C> void launch_width(const BlockArgs& a, hipStream_t s) {
    if (a.ks == 5) launch_one<C, 5>(a, s);
    else launch_one<C, 3>(a, s);
}
}  // namespace

bool block_x3w_supports(int C, int ks) { return (C == 128 || C == 192 || C == 224) && (ks == 3 || ks == 5); }

void init_x3_wblock_kernel_attributes() {
    init_one<128, 3>(); init_one<128, 5>();
    init_one<192, 3>(); init_one<192, 5>();
    init_one<224, 3>(); init_one<224, 5>();
}

void launch_block_x3w(const BlockArgs& a, hipStream_t s) {
    if (!block_x3w_supports(a.C, a.ks) || a.cop_pad % 64 != 0 || a.cop_pad <= 0) throw std::invalid_argument("launch_block_x3w: no kernel for this block");
    if (a.C == 128) launch_width<128>(a, s);
    else if (a.C == 192) launch_width<192>(a, s);
    else launch_width<224>(a, s);
}

void launch_se_gate_w(const float* pool, float* gate, int kind, const float* w1t, const float* w2t, const float* b1, int batch, int C, hipStream_t s) {
    if (C > 512) throw std::invalid_argument("launch_se_gate_w: at most 512 channels");
    hipLaunchKernelGGL(se_gate_w_kernel, dim3(batch), dim3(256), 0, s, pool, gate, kind, w1t, w2t, b1, C);
}

}  // namespace cra
