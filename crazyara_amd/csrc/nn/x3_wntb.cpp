// Precision float16x3, kernel family "-wnet": a NextViT transformer block (NTB) of a 128 / 192 / 224-channel net in one launch.
//
// On the layer kernels an NTB is nine launches (rise_net_build.hip: Builder::transformer_block) and every intermediate -- the C-wide tile
// xs, q | k | v, the attention output, the MHCA tile, the Mlp's hidden layer -- goes through HBM.  ntb_x3w_kernel<C> runs the same nine
// stages on the same folded weights (pack.cpp: fold_ntb) with one workgroup of 8 waves per board; xs stays in LDS as f32 from the first
// stage to the last, every GEMM reads its stream operand as a hi / lo f16 pair from LDS and its weights as packed fragments through raw
// buffer loads (x3_device.h), three MFMAs per product in x3_mfma's order lo*hi, hi*lo, hi*hi.
//
//   LDS (halves unless said):  xs f32 [64][C + 4] | op hi, lo [65][C + 16] (row 64: zeros, what out-of-board taps read) | T
//   T, stage by stage:         qkv f32 [64][100] + o hi, lo [64][40]   one head's q | k | v and its attention output
//                              f hi, lo [64][M + 16]                   MHCA's 3x3 output
//                              t2 hi, lo [64][144]                     one chunk of the Mlp's hidden layer
//
//   1  patch_embed   stream (f32, HBM) -> op[0, C); GEMM K = C -> + bias -> xs[0, D); op[0, D) := split(xs[0, D))
//   2  per head h    q | k | v of the head (6 cout tiles, waves 0-5, K = D) + bias -> qkv;  attention_kernel's arithmetic on waves 0-3
//                    (S^T = K Q^T, softmax with expf, O^T = V^T S^T; wave w owns the queries 16 w ...) -> o;  proj's k-slab h (= the head's
//                    32 channels) accumulates onto the proj accumulators, which live in registers across the heads
//   3  proj          + bias + xs[0, D) -> xs[0, D), op[0, D)
//   4  projection    K = D -> + bias -> u = xs[D, C), op[D, C)
//   5  MHCA          grouped 3x3 as groups of 32 (9 taps x one k-slab: the zero blocks of the layer path's dense image are not multiplied)
//                    + bias, ReLU -> f;  1x1 K = M, + u -> xs[D, C), op[D, C)
//   6  Mlp           H in chunks of 128 (a last chunk of 64: H = 448): conv1 K = C, wave w the chunk's tile w, + bias, ReLU -> t2; conv2
//                    K = 128 (64) accumulates onto the wave's cout tiles w + 8 j (x3_wblock.cpp's dealing); epilogue + bias + xs -> HBM
//
// Summation order: every accumulator walks its k-slabs in conv_gemm_x3_kernel's order (x3.hip) from zero, bias and shortcut are added as
// conv_x3_finish adds them, the attention core is attention_kernel<2>'s code on the same f32 values: the block's output has the bits of
// the nine launches.  No atomics; every LDS word read was written by this workgroup.
//
// Why this file is a .cpp: see x3_tail.cpp -- tests/test_experts_isa.py pins the kernels of the .hip listings and allows no new ones.
#include "x3_device.h"

#include <stdexcept>

namespace cra {

namespace {
template <int C_> struct X3WNtb {
    static_assert(C_ == 128 || C_ == 192 || C_ == 224, "rise_config.ntb_widths");
    static constexpr int C = C_, D = C == 128 ? 96 : 160, M = C - D, H = 2 * C, NHEAD = D / 32, NW = 8, NTHR = 64 * NW, CK = 128;
    static constexpr int XSP = C + 4;                         // floats; the 16 rows of an epilogue access land in different banks
    static constexpr int OPP = C + 16;                        // halves; 32-byte row pad as X3Block
    static constexpr int QP = 100, OP = 40, FP = M + 16, TP = CK + 16;
    static constexpr size_t xs_bytes = size_t(64) * XSP * sizeof(float);
    static constexpr size_t op_bytes = size_t(2) * 65 * OPP * sizeof(half_t);
    static constexpr size_t head_bytes = size_t(64) * QP * sizeof(float) + size_t(2) * 64 * OP * sizeof(half_t);
    static constexpr size_t t2_bytes = size_t(2) * 64 * TP * sizeof(half_t);
    static constexpr size_t f_bytes = size_t(2) * 64 * FP * sizeof(half_t);
    static constexpr size_t t_bytes = head_bytes > t2_bytes ? head_bytes : t2_bytes;
    static_assert(f_bytes <= t_bytes, "the MHCA tile shares the region");
    static constexpr size_t lds_bytes = xs_bytes + op_bytes + t_bytes;
    static_assert(lds_bytes <= 160 * 1024, "LDS budget");
    static constexpr int NT = C / 16, NJ = (NT + NW - 1) / NW;   // cout tiles of a C-wide GEMM, per wave at most (tile w + 8 j)
    static constexpr int NTD = D / 16, NJD = (NTD + NW - 1) / NW;
};

constexpr float kNtbScale = 0.17677669529663687f;            // 32^-0.5 (attention.hip)

// attention.hip's split8, restated: the attention core splits between its MFMAs, where the compiler has to see the instructions to keep
// their distance from the matrix unit's register writes (the inline-assembly split of x3_device.h gives the same halves)
__device__ __forceinline__ void ntb_split8(const float (&v)[8], half8& hi, half8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = half_t(v[j]);
        lo[j] = half_t(v[j] - float(hi[j]));
    }
}

// One GEMM of a wave: NJ cout tiles x 64 squares over NS k-slabs, the weight fragments through a window of W slabs (requested by
// prefetch(), refilled right behind their MFMAs), the stream fragments of the next slab read from LDS before this slab's MFMAs.
template <int NS, int NJ> struct X3WGemm {
    static constexpr int W = NS < 4 ? NS : 4;
    half8 ah[W][NJ], al[W][NJ];
    template <typename Frag> __device__ __forceinline__ void wload(const __amdgpu_buffer_rsrc_t& wh, const __amdgpu_buffer_rsrc_t& wl, uint32_t lane_off, const bool (&on)[NJ], Frag frag, int s) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (!on[j]) continue;
            ah[s % W][j] = x3_frag(wh, lane_off, frag(j, s));
            al[s % W][j] = x3_frag(wl, lane_off, frag(j, s));
        }
    }
    template <typename Frag> __device__ __forceinline__ void prefetch(const __amdgpu_buffer_rsrc_t& wh, const __amdgpu_buffer_rsrc_t& wl, uint32_t lane_off, const bool (&on)[NJ], Frag frag) {
#pragma unroll
        for (int s = 0; s < W; ++s) wload(wh, wl, lane_off, on, frag, s);
    }
    // read(s, bh, bl): the four square tiles' fragments of k-slab s
    template <typename Frag, typename Read>
    __device__ __forceinline__ void run(const __amdgpu_buffer_rsrc_t& wh, const __amdgpu_buffer_rsrc_t& wl, uint32_t lane_off, const bool (&on)[NJ], Frag frag, Read read, f32x4 (&acc)[NJ][4]) {
        half8 bh[2][4], bl[2][4];
        read(0, bh[0], bl[0]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s + 1 < NS) read(s + 1, bh[(s + 1) & 1], bl[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!on[j]) continue;
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(al[s % W][j], bh[s & 1][t], acc[j][t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(ah[s % W][j], bl[s & 1][t], acc[j][t], true);
#pragma unroll
                for (int t = 0; t < 4; ++t) x3_mfma(ah[s % W][j], bh[s & 1][t], acc[j][t], true);
            }
            if (s + W < NS) wload(wh, wl, lane_off, on, frag, s + W);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

template <int NJ> __device__ __forceinline__ void zero_acc(f32x4 (&acc)[NJ][4]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
}  // namespace

template <int C>
__global__ __launch_bounds__(512) void ntb_x3w_kernel(const NtbArgs a) {
    using G = X3WNtb<C>;
    constexpr int D = G::D, M = G::M, H = G::H, NHEAD = G::NHEAD, CK = G::CK, XSP = G::XSP, OPP = G::OPP, QP = G::QP, OP = G::OP, FP = G::FP, TP = G::TP;
    constexpr int NT = G::NT, NJ = G::NJ, NTD = G::NTD, NJD = G::NJD;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const xs = reinterpret_cast<float*>(smem);
    half_t* const oph = reinterpret_cast<half_t*>(smem + G::xs_bytes);
    half_t* const opl = oph + 65 * OPP;
    char* const tbase = smem + G::xs_bytes + G::op_bytes;
    float* const qkv = reinterpret_cast<float*>(tbase);
    half_t* const oh = reinterpret_cast<half_t*>(tbase + size_t(64) * QP * sizeof(float));
    half_t* const ol = oh + 64 * OP;
    half_t* const fh = reinterpret_cast<half_t*>(tbase);
    half_t* const fl = fh + 64 * FP;
    half_t* const t2h = reinterpret_cast<half_t*>(tbase);
    half_t* const t2l = t2h + 64 * TP;

    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lane_off = uint32_t(lane) * 16u;
    const float* const xb = a.x + size_t(b) * 64 * C;

    // the stream operand of a 1x1 GEMM: k-slab s of the tile (src_h, src_l) with row pitch P, from column col0 on
    auto reader = [&](const half_t* src_h, const half_t* src_l, int P, int col0) {
        return [=](int s, half8 (&h)[4], half8 (&l)[4]) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                h[t] = *reinterpret_cast<const half8*>(src_h + (t * 16 + l15) * P + col0 + s * 32 + lg * 8);
                l[t] = *reinterpret_cast<const half8*>(src_l + (t * 16 + l15) * P + col0 + s * 32 + lg * 8);
            }
        };
    };
    // v (4 consecutive channels of one square) -> the split pair at (row, col) of a tile with pitch P
    auto put_split = [&](half_t* dst_h, half_t* dst_l, int P, int row, int col, const float (&v)[4]) {
        half4 h, l;
        split4(v, h, l);
        *reinterpret_cast<half4*>(dst_h + row * P + col) = h;
        *reinterpret_cast<half4*>(dst_l + row * P + col) = l;
    };

    // ---------------- 1: patch_embed ----------------
    const __amdgpu_buffer_rsrc_t pe_h = x3_rsrc(a.patch.wh), pe_l = x3_rsrc(a.patch.wl);
    bool onD[NJD];
#pragma unroll
    for (int j = 0; j < NJD; ++j) onD[j] = w + 8 * j < NTD;
    X3WGemm<C / 32, NJD> g_pe;
    auto pe_frag = [&](int j, int s) { return uint32_t(w + 8 * j) * uint32_t(C / 32) + uint32_t(s); };
    g_pe.prefetch(pe_h, pe_l, lane_off, onD, pe_frag);
    for (int i = tid; i < OPP; i += G::NTHR) {
        oph[64 * OPP + i] = half_t(0.f);
        opl[64 * OPP + i] = half_t(0.f);
    }
#pragma unroll 1
    for (int i = tid; i < 64 * (C / 8); i += G::NTHR) {
        const int sq = i / (C / 8), v = i - sq * (C / 8);
        float f[8];
        load8<float>(xb + size_t(sq) * C + v * 8, f);
        half8 h, l;
        split8(f, h, l);
        *reinterpret_cast<half8*>(oph + sq * OPP + v * 8) = h;
        *reinterpret_cast<half8*>(opl + sq * OPP + v * 8) = l;
    }
    __syncthreads();
    {
        f32x4 acc[NJD][4];
        zero_acc<NJD>(acc);
        g_pe.run(pe_h, pe_l, lane_off, onD, pe_frag, reader(oph, opl, OPP, 0), acc);
        float keep[NJD][4][4];
#pragma unroll
        for (int j = 0; j < NJD; ++j) {
            if (!onD[j]) continue;
            const int co0 = (w + 8 * j) * 16 + lg * 4;
            float bs[4];
            load4<float>(a.patch.bias + co0, bs);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) keep[j][t][r] = acc[j][t][r] + bs[r];
                store4<float>(xs + (t * 16 + l15) * XSP + co0, keep[j][t]);
            }
        }
        __syncthreads();                                       // every wave is through with the stream's operand tiles
#pragma unroll
        for (int j = 0; j < NJD; ++j) {
            if (!onD[j]) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) put_split(oph, opl, OPP, t * 16 + l15, (w + 8 * j) * 16 + lg * 4, keep[j][t]);
        }
    }
    __syncthreads();

    // ---------------- 2: attention head by head, proj accumulating over the heads ----------------
    {
        const __amdgpu_buffer_rsrc_t qkv_h = x3_rsrc(a.qkv.wh), qkv_l = x3_rsrc(a.qkv.wl);
        const __amdgpu_buffer_rsrc_t pj_h = x3_rsrc(a.proj.wh), pj_l = x3_rsrc(a.proj.wl);
        f32x4 accP[NJD][4];
        zero_acc<NJD>(accP);
        const bool on_qkv[1] = {w < 6};
        const int part = w >> 1;                               // q, k, v
#pragma unroll 1
        for (int h = 0; h < NHEAD; ++h) {
            const int tile = part * NTD + 2 * h + (w & 1);     // of the 3 D couts
            X3WGemm<D / 32, 1> g_qkv;
            auto qkv_frag = [&](int, int s) { return uint32_t(tile) * uint32_t(D / 32) + uint32_t(s); };
            g_qkv.prefetch(qkv_h, qkv_l, lane_off, on_qkv, qkv_frag);
            X3WGemm<1, NJD> g_pj;                              // proj's k-slab h
            auto pj_frag = [&](int j, int) { return uint32_t(w + 8 * j) * uint32_t(D / 32) + uint32_t(h); };
            g_pj.prefetch(pj_h, pj_l, lane_off, onD, pj_frag);
            if (on_qkv[0]) {
                f32x4 acc[1][4];
                zero_acc<1>(acc);
                g_qkv.run(qkv_h, qkv_l, lane_off, on_qkv, qkv_frag, reader(oph, opl, OPP, 0), acc);
                float bs[4];
                load4<float>(a.qkv.bias + tile * 16 + lg * 4, bs);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = acc[0][t][r] + bs[r];
                    store4<float>(qkv + (t * 16 + l15) * QP + part * 32 + (w & 1) * 16 + lg * 4, v);
                }
            }
            __syncthreads();
            if (w < 4) {                                       // attention_kernel<2> (attention.hip), wave w: the queries 16 w ... 16 w + 15
                float q[8];
                load8<float>(qkv + (16 * w + l15) * QP + lg * 8, q);
                half8 qh, ql;
                ntb_split8(q, qh, ql);
                f32x4 s[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float k[8];
                    load8<float>(qkv + (16 * t + l15) * QP + 32 + lg * 8, k);
                    half8 kh, kl;
                    ntb_split8(k, kh, kl);
                    s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    x3_mfma(kl, qh, s[t], true);
                    x3_mfma(kh, ql, s[t], true);
                    x3_mfma(kh, qh, s[t], true);
                }
                float e[4][4];
                float mx = -INFINITY;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        e[t][r] = s[t][r] * kNtbScale;
                        mx = fmaxf(mx, e[t][r]);
                    }
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float sum = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        e[t][r] = expf(e[t][r] - mx);
                        sum += e[t][r];
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    float p[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) p[j] = e[2 * ks + j / 4][j % 4] / sum;
                    half8 ph, pl;
                    ntb_split8(p, ph, pl);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        float v[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = qkv[(16 * (2 * ks + j / 4) + 4 * lg + j % 4) * QP + 64 + dt * 16 + l15];
                        half8 vh, vl;
                        ntb_split8(v, vh, vl);
                        x3_mfma(vl, ph, o[dt], true);
                        x3_mfma(vh, pl, o[dt], true);
                        x3_mfma(vh, ph, o[dt], true);
                    }
                }
                mfma_retire(o[0], o[1]);                       // the split below reads them in inline assembly
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const float v[4] = {o[dt][0], o[dt][1], o[dt][2], o[dt][3]};
                    put_split(oh, ol, OP, 16 * w + l15, dt * 16 + 4 * lg, v);
                }
            }
            __syncthreads();
            g_pj.run(pj_h, pj_l, lane_off, onD, pj_frag, reader(oh, ol, OP, 0), accP);
        }
        // ---------------- 3: proj + bias + the patch-embed output, in place ----------------
#pragma unroll
        for (int j = 0; j < NJD; ++j) {
            if (!onD[j]) continue;
            const int co0 = (w + 8 * j) * 16 + lg * 4;
            float bs[4];
            load4<float>(a.proj.bias + co0, bs);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float rv[4], v[4];
                load4<float>(xs + (t * 16 + l15) * XSP + co0, rv);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = (accP[j][t][r] + bs[r]) + rv[r];
                store4<float>(xs + (t * 16 + l15) * XSP + co0, v);
                put_split(oph, opl, OPP, t * 16 + l15, co0, v);
            }
        }
    }
    __syncthreads();

    // ---------------- 4: projection, 5: MHCA -- the M / 16 cout tiles are waves 0 ... M / 16 - 1's ----------------
    const bool on_m[1] = {w < M / 16};
    X3WGemm<CK / 32, 1> g_c1;                                  // (the Mlp's first chunk is requested under stages 4 and 5)
    const __amdgpu_buffer_rsrc_t m1_h = x3_rsrc(a.mlp1.wh), m1_l = x3_rsrc(a.mlp1.wl);
    if (on_m[0]) {
        const __amdgpu_buffer_rsrc_t pr_h = x3_rsrc(a.projection.wh), pr_l = x3_rsrc(a.projection.wl);
        X3WGemm<D / 32, 1> g_pr;
        auto pr_frag = [&](int, int s) { return uint32_t(w) * uint32_t(D / 32) + uint32_t(s); };
        g_pr.prefetch(pr_h, pr_l, lane_off, on_m, pr_frag);
        f32x4 acc[1][4];
        zero_acc<1>(acc);
        g_pr.run(pr_h, pr_l, lane_off, on_m, pr_frag, reader(oph, opl, OPP, 0), acc);
        const int co0 = w * 16 + lg * 4;
        float bs[4];
        load4<float>(a.projection.bias + co0, bs);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[0][t][r] + bs[r];
            store4<float>(xs + (t * 16 + l15) * XSP + D + co0, v);
            put_split(oph, opl, OPP, t * 16 + l15, D + co0, v);
        }
    }
    __syncthreads();
    if (on_m[0]) {
        // grouped 3x3: cout tile w lies in group w / 2; tap by tap the neighbour square's 32 channels of the group, row 64 off the board
        const __amdgpu_buffer_rsrc_t mh_h = x3_rsrc(a.mhca.wh), mh_l = x3_rsrc(a.mhca.wl);
        X3WGemm<9, 1> g_mh;
        auto mh_frag = [&](int, int tap) { return uint32_t(w) * 9u + uint32_t(tap); };
        g_mh.prefetch(mh_h, mh_l, lane_off, on_m, mh_frag);
        const int col0 = D + (w >> 1) * 32 + lg * 8;
        auto read_tap = [&](int tap, half8 (&hh)[4], half8 (&ll)[4]) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sq = t * 16 + l15;
                const int ny = (sq >> 3) + dy, nx = (sq & 7) + dx;
                const bool ok = (unsigned(ny) < 8u) && (unsigned(nx) < 8u);
                const int off = (ok ? ny * 8 + nx : 64) * OPP + col0;
                hh[t] = *reinterpret_cast<const half8*>(oph + off);
                ll[t] = *reinterpret_cast<const half8*>(opl + off);
            }
        };
        f32x4 acc[1][4];
        zero_acc<1>(acc);
        g_mh.run(mh_h, mh_l, lane_off, on_m, mh_frag, read_tap, acc);
        const int co0 = w * 16 + lg * 4;
        float bs[4];
        load4<float>(a.mhca.bias + co0, bs);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[0][t][r] + bs[r], 0.f);
            put_split(fh, fl, FP, t * 16 + l15, co0, v);
        }
    }
    auto c1_frag = [&](int ch) { return [=](int, int s) { return uint32_t(ch * (CK / 16) + w) * uint32_t(C / 32) + uint32_t(s); }; };
    const bool on_all[1] = {true};
    g_c1.prefetch(m1_h, m1_l, lane_off, on_all, c1_frag(0));
    __syncthreads();
    if (on_m[0]) {
        const __amdgpu_buffer_rsrc_t mp_h = x3_rsrc(a.mhca_proj.wh), mp_l = x3_rsrc(a.mhca_proj.wl);
        X3WGemm<M / 32, 1> g_mp;
        auto mp_frag = [&](int, int s) { return uint32_t(w) * uint32_t(M / 32) + uint32_t(s); };
        g_mp.prefetch(mp_h, mp_l, lane_off, on_m, mp_frag);
        f32x4 acc[1][4];
        zero_acc<1>(acc);
        g_mp.run(mp_h, mp_l, lane_off, on_m, mp_frag, reader(fh, fl, FP, 0), acc);
        const int co0 = w * 16 + lg * 4;
        float bs[4];
        load4<float>(a.mhca_proj.bias + co0, bs);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float rv[4], v[4];
            load4<float>(xs + (t * 16 + l15) * XSP + D + co0, rv);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (acc[0][t][r] + bs[r]) + rv[r];
            store4<float>(xs + (t * 16 + l15) * XSP + D + co0, v);
            put_split(oph, opl, OPP, t * 16 + l15, D + co0, v);
        }
    }
    __syncthreads();

    // ---------------- 6: Mlp, the hidden layer chunk by chunk ----------------
    const __amdgpu_buffer_rsrc_t m2_h = x3_rsrc(a.mlp2.wh), m2_l = x3_rsrc(a.mlp2.wl);
    bool onC[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) onC[j] = w + 8 * j < NT;
    f32x4 accM[NJ][4];
    zero_acc<NJ>(accM);
    constexpr int NFULL = H / CK;
    constexpr bool TAIL = H % CK != 0;                          // 64 channels: tiles for waves 0-3, conv2 with two k-slabs
    static_assert(!TAIL || H % CK == 64, "a tail chunk holds 64 channels");
    static_assert(C / 32 >= 4, "conv1's window is CK / 32 = 4 slabs of its C / 32");
    auto conv1 = [&](int ch) {                                  // this wave's tile of the chunk; the first four k-slabs' weights are in g_c1
        f32x4 acc[1][4];
        zero_acc<1>(acc);
        // (X3WGemm<C / 32, 1> with the window of 4 that g_c1 holds)
        half8 bh[2][4], bl[2][4];
        const auto read = reader(oph, opl, OPP, 0);
        const auto frag = c1_frag(ch);
        read(0, bh[0], bl[0]);
#pragma unroll
        for (int s = 0; s < C / 32; ++s) {
            if (s + 1 < C / 32) read(s + 1, bh[(s + 1) & 1], bl[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t) x3_mfma(g_c1.al[s % 4][0], bh[s & 1][t], acc[0][t], true);
#pragma unroll
            for (int t = 0; t < 4; ++t) x3_mfma(g_c1.ah[s % 4][0], bl[s & 1][t], acc[0][t], true);
#pragma unroll
            for (int t = 0; t < 4; ++t) x3_mfma(g_c1.ah[s % 4][0], bh[s & 1][t], acc[0][t], true);
            if (s + 4 < C / 32) g_c1.wload(m1_h, m1_l, lane_off, on_all, frag, s + 4);
            __builtin_amdgcn_sched_barrier(0);
        }
        const int co0 = w * 16 + lg * 4;
        float bs[4];
        load4<float>(a.mlp1.bias + ch * CK + co0, bs);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[0][t][r] + bs[r], 0.f);
            put_split(t2h, t2l, TP, t * 16 + l15, co0, v);
        }
    };
    auto chunk = [&](auto tail_c, int ch) {
        constexpr bool IS_TAIL = decltype(tail_c)::value;
        constexpr int NS2 = IS_TAIL ? 2 : 4;
        X3WGemm<NS2, NJ> g_c2;
        auto c2_frag = [&](int j, int s) { return uint32_t(w + 8 * j) * uint32_t(H / 32) + uint32_t(ch * (CK / 32) + s); };
        const bool mine = !IS_TAIL || w < 4;
        if (mine) conv1(ch);
        g_c2.prefetch(m2_h, m2_l, lane_off, onC, c2_frag);
        __syncthreads();
        const bool next_mine = ch + 1 < NFULL || (TAIL && ch + 1 == NFULL && w < 4);
        if (next_mine) g_c1.prefetch(m1_h, m1_l, lane_off, on_all, c1_frag(ch + 1));
        g_c2.run(m2_h, m2_l, lane_off, onC, c2_frag, reader(t2h, t2l, TP, 0), accM);
        if (ch + 1 < NFULL + (TAIL ? 1 : 0)) __syncthreads();  // the next chunk's conv1 overwrites t2
    };
#pragma unroll 1
    for (int ch = 0; ch < NFULL; ++ch) chunk(std::false_type{}, ch);
    if constexpr (TAIL) chunk(std::true_type{}, NFULL);

    // ---------------- epilogue: + bias + xs (exact f32) -> the stream ----------------
    float* const yb = a.y + size_t(b) * 64 * C;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!onC[j]) continue;
        const int co0 = (w + 8 * j) * 16 + lg * 4;
        float bs[4];
        load4<float>(a.mlp2.bias + co0, bs);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sq = t * 16 + l15;
            float rv[4], v[4];
            load4<float>(xs + sq * XSP + co0, rv);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (accM[j][t][r] + bs[r]) + rv[r];
            store4<float>(yb + size_t(sq) * C + co0, v);
        }
    }
}

namespace {
template <int C> void init_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ntb_x3w_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, int(X3WNtb<C>::lds_bytes));
}
template <int C> void launch_one(const NtbArgs& a, hipStream_t s) {
    using G = X3WNtb<C>;
    hipLaunchKernelGGL((ntb_x3w_kernel<C>), dim3(a.batch), dim3(G::NTHR), G::lds_bytes, s, a);
}
template <int C> bool widths_are(int D, int M, int H) { return D == X3WNtb<C>::D && M == X3WNtb<C>::M && H == X3WNtb<C>::H; }
}  // namespace

bool ntb_x3w_supports(int C, int D, int M, int H) {
    return (C == 128 && widths_are<128>(D, M, H)) || (C == 192 && widths_are<192>(D, M, H)) || (C == 224 && widths_are<224>(D, M, H));
}

void init_x3_wntb_kernel_attributes() {
    init_one<128>();
    init_one<192>();
    init_one<224>();
}

void launch_ntb_x3w(const NtbArgs& a, hipStream_t s) {
    if (!ntb_x3w_supports(a.C, a.D, a.M, a.H) || a.batch <= 0) throw std::invalid_argument("launch_ntb_x3w: no kernel for this transformer block");
    if (a.C == 128) launch_one<128>(a, s);
    else if (a.C == 192) launch_one<192>(a, s);
    else launch_one<224>(a, s);
}

}  // namespace cra
