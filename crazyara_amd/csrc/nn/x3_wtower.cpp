// Precision float16x3, kernel family "-wtower": a run of consecutive mobile-bottleneck blocks of a 128 / 192 / 224-channel net in one launch.
//
// block_x3w_kernel<C, KS> (x3_wblock.cpp) runs one such block per launch: it stages the f32 board from L2, splits it into the hi / lo operand
// tiles, waits for its first weight window with nothing else in flight and drains a grid of one wave of workgroups -- per block.
// tower_x3w_kernel<C> is that kernel's chunk code (expand, depthwise, barrier, project: the same k-slab order lo*hi, hi*lo, hi*hi, the same
// tile dealing w + 8 j, the same 64-channel tail chunk on waves 0-3) in a loop over the blocks of a run:
//   * one workgroup per board, 8 waves; the board is staged and split ONCE per run (times a.gate, if the run's first block is gated)
//   * a block's depthwise size is a wave-uniform switch inside the chunk (x3_depthwise / X3Depthwise5): 3x3 and 5x5 blocks alternate
//     irregularly in AlphaVile's trunks, so a run takes both; the waves' record areas are sized for 5x5
//   * at a block's end xh / xl are dead behind the last chunk's barrier: the epilogue writes the split of the block's output straight into
//     them at the rows and columns the lane holds (x3_row order; split4 and the staging's split8 are the same split_pair per element), one
//     barrier follows, no f32 re-stage.  The next block's first expand window is requested in front of the epilogue's arithmetic, so the
//     weights land under it.
//   * the residual is the exact f32 value: every block stores its output to the run's f32 stream y, and the next block's epilogue re-reads
//     the addresses the same lane wrote (the first block reads the board's tile, times the gate): v = accP + b3 + x * gate in
//     block_x3w_kernel's order of additions -- the bits of a launch per block.  (Kept in registers beside accP instead, the stream costs 32
//     VGPRs at 192 / 224 channels and the kernel spills: 184 / 240 bytes of scratch.)  With a.pool_out the run's last block leaves its
//     channel sums for the next block's SE gate (block_x3w_kernel's squeeze).
// No atomics, no cross-workgroup dependency; every LDS word read is written first (tests/test_x3_wtower_gpu.py runs it on poisoned LDS).
//
// Why this file is a .cpp: see x3_tail.cpp.  x3_wblock.cpp is untouched: its chunk code is restated here, not shared, so that
// block_x3w_kernel's listing stays what it is.
#include "x3_device.h"

#include <stdexcept>
#include <type_traits>

namespace cra {

static_assert(sizeof(X3WTowerBlock) == 56, "tower_x3w_kernel indexes a device array of these");

namespace {
template <int C_> struct X3WTower {
    static_assert(C_ % 32 == 0 && C_ >= 128 && C_ < 256, "trunk widths 128 ... 224");
    static constexpr int C = C_, NW = 8, CK = 128, NTHR = 64 * NW;
    static constexpr int NT = C / 16;                        // cout tiles of the project GEMM
    static constexpr int NJ = (NT + NW - 1) / NW;            // per wave at most: tile w + 8 j
    static constexpr int NSLAB = C / 32;                     // k-slabs of the expand GEMM
    static constexpr int XROW = C + 16, TROW = CK + 16;      // halves; X3WBlock's map
    static constexpr int REC = 512;                          // floats of depthwise records per wave: a 5x5 tile's (a 3x3 tile's take the first 256)
    static constexpr size_t lds_bytes = (size_t(2) * 64 * XROW + size_t(4) * 64 * TROW) * sizeof(half_t) + size_t(NW) * REC * sizeof(float);
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
};
}  // namespace

template <int C>
__global__ __launch_bounds__(512) void tower_x3w_kernel(const X3WTowerArgs a) {
    using G = X3WTower<C>;
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
    const bool has2 = NJ == 2 && w + 8 < NT;                 // this wave owns a second cout tile
    const int nblocks = __builtin_amdgcn_readfirstlane(a.nblocks);

    // the block in work: its weights, its chunks, its depthwise size
    X3Weights W;
    int nfull, nchunk, nslab3;
    bool tail, ks5;
    const float* b3;
    auto enter = [&](int k) {
        const X3WTowerBlock& d = a.blocks[k];
        W = x3_weights(d.w1pk, d.w1pk_lo, d.w3pk, d.w3pk_lo, d.dwpk, d.cop_pad);
        nfull = W.cop_pad / CK;                              // chunks of 128 channels
        tail = (W.cop_pad & (CK - 1)) != 0;                  // + one of 64 (cop_pad is a multiple of 64)
        nchunk = nfull + (tail ? 1 : 0);
        nslab3 = W.cop_pad >> 5;
        ks5 = __builtin_amdgcn_readfirstlane(d.ks) == 5;
        b3 = d.b3;
    };
    auto expands = [&](int ch) { return ch < nfull || w < 4; };     // a tail chunk's four tiles are waves 0-3's

    const float* const xb = a.x + size_t(b) * 64 * C;
    const float* const gate = a.gate ? a.gate + size_t(b) * C : nullptr;

    // expand weight window: block_x3w_kernel's.  The first EW slabs of a block's chunk 0 are requested in front of the epilogue of the block
    // before it (the run's first block: before the board is staged)
    half8 e_h[EW], e_l[EW];
    auto load_expand = [&](int ch, int s) {
        const uint32_t f = uint32_t(ch * (CK / 16) + w) * uint32_t(NSLAB) + uint32_t(s);
        e_h[s % EW] = x3_frag(W.w1h, lane_off, f);
        e_l[s % EW] = x3_frag(W.w1l, lane_off, f);
    };
    enter(0);
    if (expands(0)) {
#pragma unroll
        for (int s = 0; s < EW; ++s) load_expand(0, s);
    }

    // stage, once per run: float board tile [64][C] (x := x * gate[c] if the first block has an SE gate) -> split tiles
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
            // the tile's depthwise records (1 KiB for 3x3, 2 KiB for 5x5): 16-byte loads per lane, parked in the wave's LDS scratch half-way
            // through the MFMAs and read back per lane as broadcast reads
            f32x4 dw_raw[2];
            const uint32_t dw_tile = uint32_t(ch * (CK / 16) + w) * (ks5 ? 2048u : 1024u);
            dw_raw[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.dw, lane_off, dw_tile, 0));
            if (ks5) dw_raw[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.dw, lane_off, dw_tile + 1024u, 0));
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
                    *reinterpret_cast<f32x4*>(my_dws + lane * 4) = dw_raw[0];
                    if (ks5) *reinterpret_cast<f32x4*>(my_dws + 256 + lane * 4) = dw_raw[1];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // they land while the depthwise runs (TAIL: the second slab's are requested behind the depthwise and land under the barrier and
            // the first slab's MFMAs -- with both in flight across a 5x5 depthwise the 224-channel kernel spills)
#pragma unroll
            for (int s2 = 0; s2 < (TAIL ? 1 : PW); ++s2) load_project(s2);
            // ---------------- D: BN1 + ReLU, depthwise on the accumulators, BN2 + ReLU, exact f32; split -> t2 ----------------
            float outv[4][4];                                   // [tile][channel r]
            if (!ks5) {
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
            if (TAIL) load_project(1);
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

    // The f32 stream in the epilogue's layout: the lane holds channels (w + 8 j) * 16 + lg * 4 ... + 3 of the squares x3_square(t * 16 + l15) =
    // x3_square(l15) + 8 t.  One byte offset per lane; j and t are wave-uniform offsets of the buffer instructions (as 64-bit addresses the
    // compiler keeps all of them in registers across the run and the kernel spills).
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t x_rsrc = x3_rsrc(xb), y_rsrc = x3_rsrc(a.y + size_t(b) * 64 * C);
    const uint32_t s_lane = uint32_t(x3_square(l15) * C + w * 16 + lg * 4) * 4u;
    auto s_off = [](int j, int t) { return uint32_t(t * 8 * C + j * 128) * 4u; };
#pragma unroll 1
    for (int k = 0; k < nblocks; ++k) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) accP[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ch = 0; ch < nfull; ++ch) chunk(std::false_type{}, ch);
        if (tail) chunk(std::true_type{}, nfull);

        // ---------------- epilogue: + BN3 bias + residual, block_x3w_kernel's sum; the new stream -> y and, split, -> xh / xl ----------------
        // The residual of the run's first block is the board's f32 tile again (times the gate); every later block re-reads from y what
        // THIS lane stored there a block ago -- the same addresses, so program order is all the ordering it needs.
        const bool last = k + 1 == nblocks;
        const __amdgpu_buffer_rsrc_t rb = k == 0 ? x_rsrc : y_rsrc;
        const float* const g = k == 0 ? gate : nullptr;
        float bs[NJ][4];
        f32x4 xr[NJ][4];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j == 1 && !has2) continue;
            const int co0 = (w + 8 * j) * 16 + lg * 4;
            load4<float>(b3 + co0, bs[j]);
#pragma unroll
            for (int t = 0; t < 4; ++t) xr[j][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, s_lane, s_off(j, t), 0));
        }
        if (!last) {
            // the next block's first expand window: requested behind the epilogue's own loads, it lands under the arithmetic below
            __builtin_amdgcn_sched_barrier(0);
            enter(k + 1);
            if (expands(0)) {
#pragma unroll
                for (int s = 0; s < EW; ++s) load_expand(0, s);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j == 1 && !has2) continue;
            const int co0 = (w + 8 * j) * 16 + lg * 4;
            float pool[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {1.f, 1.f, 1.f, 1.f};
            if (g) load4<float>(g + co0, gv);                   // (a gated first block only: this one load waits behind the window)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = accP[j][t][r] + bs[j][r] + xr[j][t][r] * gv[r];
                    pool[r] += v[r];
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{v[0], v[1], v[2], v[3]}), y_rsrc, s_lane, s_off(j, t), 0);
                if (!last) {                                    // xh / xl are dead behind the last chunk's barrier: the next block's operand tiles
                    half4 h, l;
                    split4(v, h, l);
                    *reinterpret_cast<half4*>(xh + (t * 16 + l15) * XROW + co0) = h;
                    *reinterpret_cast<half4*>(xl + (t * 16 + l15) * XROW + co0) = l;
                }
            }
            if (last && a.pool_out) {                           // squeeze (AdaptiveAvgPool2d) of the run's output: block_x3w_kernel's
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int off = 8; off > 0; off >>= 1) pool[r] += __shfl_xor(pool[r], off, 64);
                if (l15 == 0) store4<float>(a.pool_out + size_t(b) * C + co0, pool);
            }
        }
        if (!last) __syncthreads();
    }
}

namespace {
template <int C> void init_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tower_x3w_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, int(X3WTower<C>::lds_bytes));
}
template <int C> void launch_one(const X3WTowerArgs& a, hipStream_t s) {
    using G = X3WTower<C>;
    hipLaunchKernelGGL((tower_x3w_kernel<C>), dim3(a.batch), dim3(G::NTHR), G::lds_bytes, s, a);
}
}  // namespace

bool tower_x3w_supports(int C, int ks) { return block_x3w_supports(C, ks); }

void init_x3_wtower_kernel_attributes() {
    init_one<128>();
    init_one<192>();
    init_one<224>();
}

void launch_tower_x3w(const X3WTowerArgs& a, hipStream_t s) {
    if (!tower_x3w_supports(a.C, 3) || a.nblocks < 1 || !a.blocks || a.batch < 1) throw std::invalid_argument("launch_tower_x3w: no kernel for this run");
    if (a.C == 128) launch_one<128>(a, s);
    else if (a.C == 192) launch_one<192>(a, s);
    else launch_one<224>(a, s);
}

}  // namespace cra
