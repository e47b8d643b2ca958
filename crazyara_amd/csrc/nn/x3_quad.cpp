// Precision float16x3: the two-role tower with a 64-channel tail chunk (x3_tail.cpp: tower_x3_tail_kernel) with the EXPAND waves'
// accumulators TRANSPOSED -- the quadrant depthwise.
//
// tower_x3_quad_kernel is tower_x3_tail_kernel -- the same roles, barriers in the same order, packed weights, LDS regions, tail chunk
// variants, gate phases and early request of the first window; the residual stream in the PROJECT waves' registers -- except:
//   E: the expand MFMA takes the x fragment as A and the weight fragment as B (both have the same lane shape: the packing is what it
//      was).  A lane then holds channel l15 of the tile on rows 4 lg + r of square tile t: with the row order of x3_row that is rank
//      4 (lg >> 1) + t, file 4 (lg & 1) + r, a 4 x 4 quadrant of the board.  The row order, and with it staging, the epilogue's xh / xl
//      stores, the store to HBM, the PROJECT accumulators' square order and the SE phases, are what they were.
//   D: X3DepthwiseQuad (x3_quad.h): the taps are v_fmac_f32 on the lane's own registers, a halo of 4 + 4 + 1 values comes from lane
//      groups lg ^ 1, lg ^ 2, lg ^ 3 through the LDS crossbar.  X3Depthwise::gather spends 16 half-rate DPP moves per channel.
//   t2: stored as t2T[channel][square row] (x3q_t2t_offset: 128-byte rows, XOR swizzle, no padding) with one ds_write_b64 per rank and
//      hi / lo, the count of before; the PROJECT waves read their B fragments with two ds_read_b64_tr_b16 each.  A fragment holds the k
//      it held: the project sums add the same terms in the same positions.
// Per output the depthwise arithmetic is tower_x3_tail_kernel's; the expand sums are the same products in the same order, but the
// accumulation inside an MFMA is not specified to be the same with A and B swapped, so the two kernels are compared within a bound
// (tests/test_x3_quad_gpu.py), not bit for bit.  3x3 runs only: launch_tower_x3 sends 5x5 runs to tower_x3_tail_kernel, and
// CRA_X3_NO_QUAD every run.
//
// Maintaining the two files: everything but three places is x3_tail.cpp's text -- the role loops, load_e / load_p and the window logic,
// the tail chunk variants, the gate phases, the epilogue and the CRA_X3_TRACE stamps -- and a fix to that schedule belongs in BOTH.  The
// three places that differ (x3_tail.cpp names the same three):
//   1. the EXPAND wave's lane constants in front of its chunk loop (x3_quad_offsets and the t2T store offsets, where the tail kernel has
//      x3_edge_offsets) and the operand order of the three expand x3_mfma calls;
//   2. the depthwise pieces set between the k-slabs (X3DepthwiseQuad's load / gather / taps_rank, KS == 3 only, where the tail kernel
//      has X3Depthwise's and X3Depthwise5's) and the half4 stores of their output (t2T offsets, where the tail kernel has [row][TROW]);
//   3. the PROJECT wave's operand reads (x3q_read_fragment on offsets computed once in front of the chunk loop, where the tail kernel
//      reads a half8 per square row).
//
// (Why a .cpp file: x3_tail.cpp.)
#include "x3_device.h"
#include "x3_quad.h"

#include <type_traits>

namespace cra {

template <int KS>
__global__ __launch_bounds__(512) void tower_x3_quad_kernel(const X3TowerArgs a) {
    static_assert(KS == 3, "depthwise 3x3 (X3DepthwiseQuad); 5x5 runs stay on tower_x3_tail_kernel");
    constexpr int REC = 256;                            // floats of depthwise records per 16-channel tile
    using G = X3Block;
    static_assert(G::NE == 1 && G::T2BUF == 2 && G::CK == 128, "the role kernel uses the NE = 1 tile geometry (two t2 buffers of 128 channels)");
    static_assert(X3Q_T2T_HALVES <= 64 * G::TROW, "t2T of a chunk lies in the [64][TROW] tile's place");
    constexpr int C = G::C, CK = G::CK, XROW = G::XROW, TROW = G::TROW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const X3Tiles T = x3_tiles(smem);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool expand_role = wave < 4;
    const int w = wave & 3;
    const uint32_t lane_off = uint32_t(lane) * 16u;
    x3_stage_tile(T, a.x + size_t(b) * 64 * C, nullptr, tid);
    __syncthreads();
    // EXPAND role: the expand weight window, its first two k-slabs of a block requested at the END of the block before (tower_x3_roles_kernel)
    constexpr int EW = 2;
    half8 e_h[EW][2], e_l[EW][2];
    bool first_chunk_requested = false;
    // The two roles run the block loop separately (the same barriers in the same order): with one loop around an if / else, a value an EXPAND
    // wave carries from one block into the next -- the first chunk's fragments -- counts as live through the PROJECT branch of the
    // iteration between (the allocator does not know that a wave never changes its role), and that branch has no register to spare.
    if (expand_role) {
    for (int blk = 0; blk < a.nblocks; ++blk) {
        const X3TowerBlock& d = a.blocks[blk];
        if (blk > 0 && d.se_kind != 0) {
            x3_se_gate_from_mean(d, reinterpret_cast<float*>(T.t2h), tid);     // (the squeeze and x *= gate are the PROJECT waves': x3_stream_se)
            __syncthreads();                                            // the gated operand tiles are written
            // (never requested in front of a gate phase.  The flag alone does not tell the register allocator: an empty definition of every
            // fragment here ends their live ranges in front of the phase, which needs the registers)
            first_chunk_requested = false;
#pragma unroll
            for (int ne = 0; ne < 2; ++ne) {
#pragma unroll
                for (int q = 0; q < EW; ++q) { asm volatile("" : "=v"(e_h[q][ne])); asm volatile("" : "=v"(e_l[q][ne])); }
            }
        }
        const X3Weights W = x3_weights(d.w1pk, d.w1pk_lo, d.w3pk, d.w3pk_lo, d.dwpk, d.cop_pad);
        const int n = W.cop_pad / CK;
        const bool tail = __builtin_amdgcn_readfirstlane(d.tail) != 0;     // chunk n - 1 holds 64 channels: one tile per EXPAND wave
#ifdef CRA_X3_TRACE
        const bool tracing = (b == 0 || b == 131) && blk == CRA_X3_TRACE;
        int trace_n = 0;
#endif
        // barriers of a block, the same for both roles: one behind each of the halves 0 ... 2n, then the one behind the epilogue
        {
            const X3QuadOffsets qo = x3_quad_offsets(lane);              // which sides of the lane's quadrant are board edges (zero rows of the records)
            int sto[4];                                                 // t2T offsets of the lane's four ranks (tile 0)
#pragma unroll
            for (int t = 0; t < 4; ++t) sto[t] = x3q_store_offset(0, l15, lg, t);
            // expand weight window: EW of the 8 k-slabs x 2 channel tiles x (hi, lo); the stream runs on across chunk boundaries: slab s of
            // chunk i sits in slot s % EW and is refilled with the slab EW positions ahead right behind its MFMAs
            // cout tile (16 channels) of (chunk i, wave w, ne): i * 8 + w * 2 + ne; in the tail chunk the wave owns ONE tile, i * 8 + w (asked
            // for its second tile it names the same one: a valid address where the window runs on into the tail chunk with both loads)
            auto e_tile = [&](int i, int ne) { return i * (CK / 16) + (tail && i == n - 1 ? w : w * 2 + ne); };
            auto load_e = [&](auto one_c, int i, int s) {
                if constexpr (X3_ABL & 16) return;
#pragma unroll
                for (int ne = 0; ne < (decltype(one_c)::value ? 1 : 2); ++ne) {
                    const uint32_t f = uint32_t(e_tile(i, ne)) * (C / 32) + uint32_t(s);
                    e_h[s % EW][ne] = x3_frag(W.w1h, lane_off, f);
                    e_l[s % EW][ne] = x3_frag(W.w1l, lane_off, f);
                }
            };
            auto load_first_chunk = [&](const X3Weights& Wx, bool one) { // the window's slots with the first k-slabs of chunk 0's tiles (one: a block that is only a tail)
                if constexpr (X3_ABL & 16) return;
#pragma unroll
                for (int s = 0; s < EW; ++s)
#pragma unroll
                    for (int ne = 0; ne < 2; ++ne) {
                        const uint32_t f = uint32_t(one ? w : w * 2 + ne) * (C / 32) + uint32_t(s);
                        e_h[s][ne] = x3_frag(Wx.w1h, lane_off, f);
                        e_l[s][ne] = x3_frag(Wx.w1l, lane_off, f);
                    }
            };
            if constexpr (X3_ABL & 16) {
#pragma unroll
                for (int s = 0; s < EW; ++s)
#pragma unroll
                    for (int ne = 0; ne < 2; ++ne) e_h[s][ne] = e_l[s][ne] = *reinterpret_cast<const half8*>(T.xh + lane * 8);
            }
            if (!first_chunk_requested) load_first_chunk(W, tail && n == 1);
            float* const my_dws = T.dws + (w * 2) * REC;               // this wave's two record tiles
            f32x4 accE[2][4], accD[2][4];                               // chunk i being expanded / chunk i - 1 in the depthwise
            X3DepthwiseQuad dw;
            // Interval i: E(i) (HASE) with D(i - 1) (HASD) cut into sixteen pieces, two per k-slab: tile 0 in slabs 0-3, tile 1 in 4-7.
            // ONEE: chunk i is the tail, E(i) expands the wave's one tile (half the MFMAs per k-slab); ONED: chunk i - 1 is the tail, D(i - 1) is
            // tile 0's eight pieces in four k-slabs' time and writes columns w * 16 ... of t2.  The tail is a block's last chunk: never both.
            auto interval = [&](auto hase_c, auto hasd_c, auto onee_c, auto oned_c, int i) {
                constexpr bool HASE = decltype(hase_c)::value, HASD = decltype(hasd_c)::value;
                constexpr bool ONEE = decltype(onee_c)::value, ONED = decltype(oned_c)::value;
                static_assert(!(ONEE && !HASE) && !(ONED && (HASE || !HASD)), "the tail chunk is expanded in interval n - 1 and runs the depthwise alone in interval n");
                constexpr int NEE = ONEE ? 1 : 2;                        // channel tiles E(i) expands
                // stream fragments (A operands) through a ring of four (k-slab, square tile) steps: a step's pair (hi, lo) is requested
                // three steps = 18 MFMAs ahead (a slab's eight pairs double-buffered would be 64 registers beside the depthwise's state)
                half8 ring_h[4], ring_l[4];
                auto read_step = [&](int st) {                          // step st = k-slab st / 4, square tile st % 4
                    if constexpr (X3_ABL & 8) {
                        ring_h[st % 4] = e_h[0][0];
                        ring_l[st % 4] = e_l[0][0];
                    } else {
                        ring_h[st % 4] = *reinterpret_cast<const half8*>(T.xh + ((st & 3) * 16 + l15) * XROW + (st >> 2) * 32 + lg * 8);
                        ring_l[st % 4] = *reinterpret_cast<const half8*>(T.xl + ((st & 3) * 16 + l15) * XROW + (st >> 2) * 32 + lg * 8);
                    }
                };
                f32x4 dw_raw[NEE][REC / 256];
                if constexpr (HASE) {
                    // depthwise records of chunk i's tiles: one 16-byte load per lane and tile (x3_chunks); they go to LDS at the end of
                    // the interval, behind the depthwise that still reads chunk i - 1's
#pragma unroll
                    for (int ne = 0; ne < NEE; ++ne)
#pragma unroll
                        for (int h2 = 0; h2 < REC / 256; ++h2)
                            dw_raw[ne][h2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W.dw, lane_off, uint32_t(e_tile(i, ne) * 16) * uint32_t(REC / 4) + uint32_t(h2) * 1024u, 0));
#pragma unroll
                    for (int ne = 0; ne < NEE; ++ne)
#pragma unroll
                        for (int t = 0; t < 4; ++t) accE[ne][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    read_step(0); read_step(1); read_step(2);
                }
                if constexpr (HASD) dw.load(my_dws, l15, qo);
                half_t* const t2h = T.t2h + ((i - 1) & 1) * 64 * TROW;
                half_t* const t2l = T.t2l + ((i - 1) & 1) * 64 * TROW;
#pragma unroll
                for (int sl = 0; sl < (ONED ? C / 64 : C / 32); ++sl) {
                    const int dt = sl / 4, ph = sl % 4;                 // the depthwise's tile and quarter
                    if constexpr (HASD) {
                        if (!ONED && sl == 3) dw.load(my_dws + 256, l15, qo);   // tile 1's records (tile 0's last taps ran in slab 2)
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (HASE) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int st = sl * 4 + t;
                            if (st + 3 < 4 * (C / 32)) read_step(st + 3);
#pragma unroll
                            for (int ne = 0; ne < NEE; ++ne) {
                                x3_mfma(ring_h[st % 4], e_l[sl % EW][ne], accE[ne][t], !(X3_ABL & 2));      // x is A: D[row 4 lg + r][channel l15]
                                x3_mfma(ring_l[st % 4], e_h[sl % EW][ne], accE[ne][t], !(X3_ABL & 2));
                                x3_mfma(ring_h[st % 4], e_h[sl % EW][ne], accE[ne][t], !(X3_ABL & 2));
                            }
                        }
                        if (sl + EW < C / 32) load_e(onee_c, i, sl + EW);
                        else if constexpr (ONEE) load_e(onee_c, i, sl + EW - C / 32);      // (behind the last chunk: a valid address, no branch in the stretch)
                        else load_e(onee_c, i + 1 < n ? i + 1 : i, sl + EW - C / 32);      // (the next chunk's tiles, e_tile: one tile twice if it is the tail)
                    }
                    if constexpr (HASD) {
                        // a tile's depthwise in four k-slabs: BN1 + ReLU and the halo exchange; ranks 0, 1; ranks 2, 3; split and store
                        if (ph == 0) dw.gather(accD[dt], lg, qo);
                        if (ph == 1) { dw.template taps_rank<0>(); dw.template taps_rank<1>(); dw.template pin_rank<0>(); dw.template pin_rank<1>(); }
                        if (ph == 2) { dw.template taps_rank<2>(); dw.template taps_rank<3>(); dw.template pin_rank<2>(); dw.template pin_rank<3>(); }
                        if (ph == 3) {
                            const int tile = ONED ? w : w * 2 + dt;            // split -> t2T of chunk i - 1: the lane's channel, its four files of rank t
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                half4 h, l;
                                split4(dw.outv[t], h, l);
                                if constexpr (X3_ABL & 64) {
                                    asm volatile("" ::"v"(h), "v"(l));
                                } else {
                                    *reinterpret_cast<half4*>(t2h + tile * 16 * X3Q_T2T_ROW + sto[t]) = h;
                                    *reinterpret_cast<half4*>(t2l + tile * 16 * X3Q_T2T_ROW + sto[t]) = l;
                                }
                            }
                        }
                    }
                    if constexpr (HASE && HASD) {
#pragma unroll
                        for (int r = 0; r < 12 * NEE; ++r) {             // behind every MFMA up to four VALU instructions (the tail's half as many MFMAs: eight)
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x002, ONEE ? 8 : 4, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (HASE) {                                    // the depthwise is through with chunk i - 1: its records and accumulators make room
#pragma unroll
                    for (int ne = 0; ne < NEE; ++ne)
#pragma unroll
                        for (int h2 = 0; h2 < REC / 256; ++h2) *reinterpret_cast<f32x4*>(my_dws + ne * REC + h2 * 256 + lane * 4) = dw_raw[ne][h2];
#pragma unroll
                    for (int ne = 0; ne < NEE; ++ne)
#pragma unroll
                        for (int t = 0; t < 4; ++t) accD[ne][t] = accE[ne][t];
                }
            };
            // the block's n + 1 intervals, each closed by the workgroup barrier: the full chunks in a loop, the tail's two intervals behind it
            constexpr std::true_type yes{};
            constexpr std::false_type no{};
            auto run = [&](auto hase_c, auto hasd_c, auto onee_c, auto oned_c, int i) {
                const int kk = i - 1;                                    // (stamp bookkeeping)
                X3_STAMP(0);
                interval(hase_c, hasd_c, onee_c, oned_c, i);
                X3_STAMP(3);
                if constexpr (!(X3_ABL & 32)) __syncthreads();
                X3_STAMP(4);
            };
            const int nfull = tail ? n - 1 : n;                          // chunks of 128 channels
            if (nfull == 0) run(yes, no, yes, no, 0);                    // (a block that is only a tail)
            else run(yes, no, no, no, 0);
            for (int i = 1; i < nfull; ++i) run(yes, yes, no, no, i);
            if (tail) {
                if (nfull > 0) run(yes, yes, yes, no, n - 1);
                run(no, yes, no, yes, n);
            } else run(no, yes, no, no, n);
            // the next block's first fragments (unless a gate phase comes first): they land while the PROJECT waves finish this block
            first_chunk_requested = false;
            if (blk + 1 < a.nblocks && a.blocks[blk + 1].se_kind == 0) {
                const X3TowerBlock& dn = a.blocks[blk + 1];
                load_first_chunk(x3_weights(dn.w1pk, dn.w1pk_lo, dn.w3pk, dn.w3pk_lo, dn.dwpk, dn.cop_pad), dn.tail != 0 && dn.cop_pad == CK);
                first_chunk_requested = true;
            }
            __syncthreads();                                            // the PROJECT waves' block epilogue
            { const int kk = n; X3_STAMP(5); }
        }
    }
    } else {
    // PROJECT waves: the residual stream of this wave's 64 couts lives in accX (x3_stream_load) from the first block to the last
    constexpr int NJ = 4;
    f32x4 accX[NJ][4];
    x3_stream_load<NJ>(accX, a.x + size_t(b) * 64 * C, w * NJ, l15, lg);
    for (int blk = 0; blk < a.nblocks; ++blk) {
        const X3TowerBlock& d = a.blocks[blk];
        if (blk > 0 && d.se_kind != 0) x3_stream_se<NJ>(T, d, accX, reinterpret_cast<float*>(T.t2h), w * NJ, tid);
        const X3Weights W = x3_weights(d.w1pk, d.w1pk_lo, d.w3pk, d.w3pk_lo, d.dwpk, d.cop_pad);
        const int n = W.cop_pad / CK;
        const int nslab3 = W.cop_pad >> 5;
        const bool tail = __builtin_amdgcn_readfirstlane(d.tail) != 0;     // P(n - 1) has K = 64
#ifdef CRA_X3_TRACE
        const bool tracing = (b == 0 || b == 131) && blk == CRA_X3_TRACE;
        int trace_n = 0;
#endif
        {
            // project weight window: 2 of a chunk's 4 k-slabs x 4 cout tiles x (hi, lo), running on across chunk boundaries
            constexpr int PW = 2;
            half8 p_h[PW][NJ], p_l[PW][NJ];
            int rdo[2][4];                                              // t2T offsets of the lane's transposed reads (every lane supplies one, in bounds: EXEC is all ones here)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int t = 0; t < 4; ++t) rdo[hh][t] = x3q_read_offset(0, hh, t, l15, lg);
            auto load_p = [&](int k, int s2) {                         // cout tile = w * 4 + j, K slab = k * 4 + s2
                if constexpr (X3_ABL & 16) return;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const uint32_t f = uint32_t(w * NJ + j) * uint32_t(nslab3) + uint32_t(k * (CK / 32) + s2);
                    p_h[s2 % PW][j] = x3_frag(W.w3h, lane_off, f);
                    p_l[s2 % PW][j] = x3_frag(W.w3l, lane_off, f);
                }
            };
            if constexpr (X3_ABL & 16) {
#pragma unroll
                for (int s2 = 0; s2 < PW; ++s2)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) p_h[s2][j] = p_l[s2][j] = *reinterpret_cast<const half8*>(T.xl + lane * 8);
            }
            x3_stream_add_bias<NJ>(accX, d.b3, w * NJ, lg);             // the block's project sums are accumulated on x + b3
#pragma unroll
            for (int s2 = 0; s2 < PW; ++s2) load_p(0, s2);
            if constexpr (!(X3_ABL & 32)) {
                __syncthreads();                                        // intervals 0 and 1: chunk 0 is expanded, then run through the depthwise
                __syncthreads();
            }
            // P(kk): K = 128 in four k-slabs; ONE: the tail chunk, K = 64 in two.  The window runs on into the next chunk behind the last two
            // slabs of a full chunk; behind the block's last real slab it asks for that chunk's first slabs again (a valid address, as the
            // full-chunk kernel does there), never for a slab of the padded half.
            auto project = [&](auto one_c, int kk) {
                constexpr int NS2 = decltype(one_c)::value ? CK / 64 : CK / 32;
                const half_t* const t2h = T.t2h + (kk & 1) * 64 * TROW;
                const half_t* const t2l = T.t2l + (kk & 1) * 64 * TROW;
                const half_t* rd[2][4];                                  // the lane's addresses in k-slab 0 (x3q_read_offset)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                    for (int t = 0; t < 4; ++t) rd[hh][t] = t2h + rdo[hh][t];
                const int to_lo = int(t2l - t2h);
                X3_STAMP(8);
                half8 bh[2][4], bl[2][4];
                auto read_t2 = [&](int s2, half8 (&h)[4], half8 (&l)[4]) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if constexpr (X3_ABL & 8) {
                            h[t] = p_h[s2 % PW][0];
                            l[t] = p_l[s2 % PW][0];
                        } else {
                            h[t] = x3q_read_fragment(rd[0][t] + s2 * 32 * X3Q_T2T_ROW, rd[1][t] + s2 * 32 * X3Q_T2T_ROW);
                            l[t] = x3q_read_fragment(rd[0][t] + s2 * 32 * X3Q_T2T_ROW + to_lo, rd[1][t] + s2 * 32 * X3Q_T2T_ROW + to_lo);
                        }
                    }
                };
                read_t2(0, bh[0], bl[0]);
#pragma unroll
                for (int s2 = 0; s2 < NS2; ++s2) {
                    if (s2 + 1 < NS2) read_t2(s2 + 1, bh[(s2 + 1) & 1], bl[(s2 + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int t = 0; t < 4; ++t) x3_mfma(p_l[s2 % PW][j], bh[s2 & 1][t], accX[j][t], !(X3_ABL & 4));
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int t = 0; t < 4; ++t) x3_mfma(p_h[s2 % PW][j], bl[s2 & 1][t], accX[j][t], !(X3_ABL & 4));
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int t = 0; t < 4; ++t) x3_mfma(p_h[s2 % PW][j], bh[s2 & 1][t], accX[j][t], !(X3_ABL & 4));
                    if (s2 + PW < NS2) load_p(kk, s2 + PW);
                    else if constexpr (decltype(one_c)::value) load_p(kk, s2 + PW - NS2);
                    else load_p(kk + 1 < n ? kk + 1 : kk, s2 + PW - NS2);
                    if (s2 == 1) X3_STAMP(9);
                    __builtin_amdgcn_sched_barrier(0);
                }
                X3_STAMP(10);
            };
            const int nfull = tail ? n - 1 : n;                          // chunks of 128 channels
            for (int kk = 0; kk < nfull; ++kk) {                        // P(kk) runs in interval kk + 2
                project(std::false_type{}, kk);
                if (kk + 1 < n) {
                    if constexpr (!(X3_ABL & 32)) __syncthreads();      // (the last chunk's project phase has no partner: the epilogue's barrier follows)
                }
                X3_STAMP(11);
            }
            if (tail) {
                const int kk = n - 1;
                project(std::true_type{}, kk);
                X3_STAMP(11);
            }
            // block epilogue: accX IS the new stream; its operand forms go to LDS for the next block unless that block gates it first
            // (x3_stream_se writes them then) or there is none (the result leaves from the registers).  Every EXPAND wave is behind its
            // last read of the tiles: it waits at the barrier below.
            if (blk + 1 < a.nblocks && a.blocks[blk + 1].se_kind == 0) x3_stream_write_tiles<NJ>(T, accX, w * NJ, l15, lg);
            { const int kk = n; X3_STAMP(12); }
            __syncthreads();
            { const int kk = n; X3_STAMP(13); }
        }
    }
    x3_stream_store<NJ>(accX, a.y + size_t(b) * 64 * C, w * NJ, l15, lg);     // the stream -> HBM straight from the registers
    }
}

void init_x3_quad_kernel_attributes() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tower_x3_quad_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, int(X3Block::lds_bytes));
}
void launch_tower_x3_quad(const X3TowerArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tower_x3_quad_kernel<3>, dim3(a.batch), dim3(X3Block::NTHR), X3Block::lds_bytes, s, a);
}

}  // namespace cra
