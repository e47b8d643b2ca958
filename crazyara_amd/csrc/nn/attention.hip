// gfx950 kernel of the NextViT transformer block's attention core (E_MHSA, next_vit_official_modules.py:201-265, sr_ratio 1): per board
// and head of 32 channels, S = Q K^T * 32^-0.5 over the board's 64 squares, a row softmax, O = S V.  Q, K and V come from one [B][64][3D]
// tile (the q / k / v Linears as one conv GEMM, rise_net.hip: Builder::transformer_block); O goes to [B][64][D], channel 32 h + d.
//
// One workgroup per (head, board), four waves; wave w owns the queries 16 w ... 16 w + 15.  K and V of the head are staged in LDS once
// and read by all four waves; a wave reads its own 16 query rows from global memory.  Both products run on 16x16x32 matrix fragments
// (device_utils.h: mma_k32) in the three arithmetic forms of the precision modes: f16 operands (float16), exact f32 (float32, 8 x
// 16x16x4 f32) and the hi / lo f16 split of both operands with three MFMAs (float16x3, as x3.hip's conv GEMM: lo*hi, hi*lo, hi*hi).
//
// The first product is computed transposed, S^T = K Q^T: lane (l15 = lane & 15, lg = lane >> 4) then holds, of query 16 w + l15, the
// keys 16 t + 4 lg + r (t = key tile, r = accumulator register) -- a whole query row over the four lanes of equal l15, so the softmax
// needs two cross-lane steps, and the scores feed the second product, O^T = V^T S^T, as its B operand with no data movement: element j
// of k-step s is key 16 (2 s + j / 4) + 4 lg + j % 4, and the A operand (V^T from LDS) takes its keys in that same order.  The row
// maximum and sum are combined over lanes with xor shuffles; each step adds two operands that are the same pair on both lanes, so the
// four lanes of a row hold the same bits.  expf is the accurate one.  No atomics; every LDS word read was written by this workgroup.
#include "kernels.h"

#include <stdexcept>
#include "device_utils.h"

namespace cra {

namespace {
constexpr int kHeadDim = 32;
constexpr float kScale = 0.17677669529663687f;    // 32^-0.5 (E_MHSA.scale = head_dim ** -0.5)

// MODE 0: float16 (T = half_t), 1: float32 (T = float, exact f32 MFMA), 2: float16x3 (T = float, split operands)
template <int MODE> struct AttnT { typedef float T; };
template <> struct AttnT<0> { typedef half_t T; };

__device__ __forceinline__ void split8(const float (&v)[8], half8& hi, half8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = half_t(v[j]);
        lo[j] = half_t(v[j] - float(hi[j]));
    }
}

// acc += A B over 32 k: A and B given as 8 floats per lane in the mma_k32 labelling (k = (lane >> 4) * 8 + j on both)
template <int MODE> __device__ __forceinline__ void mma32(const float (&a)[8], const float (&b)[8], f32x4& acc) {
    if constexpr (MODE == 0) {
        half8 ah, bh;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ah[j] = half_t(a[j]); bh[j] = half_t(b[j]); }
        mma_k32(ah, bh, acc);
    } else if constexpr (MODE == 1) {
        float8 af, bf;
#pragma unroll
        for (int j = 0; j < 4; ++j) { af.lo[j] = a[j]; af.hi[j] = a[4 + j]; bf.lo[j] = b[j]; bf.hi[j] = b[4 + j]; }
        mma_k32(af, bf, acc);
    } else {
        half8 ah, al, bh, bl;
        split8(a, ah, al);
        split8(b, bh, bl);
        mma_k32(al, bh, acc);
        mma_k32(ah, bl, acc);
        mma_k32(ah, bh, acc);
    }
}
}  // namespace

template <int MODE>
__global__ __launch_bounds__(256) void attention_kernel(const AttentionArgs a) {
    typedef typename AttnT<MODE>::T T;
    constexpr int KP = kHeadDim + 16 / int(sizeof(T));          // LDS row pitch: +16 B, rows stay 16-B aligned
    __shared__ __attribute__((aligned(16))) T kv[2][64 * KP];    // K, V of this head: [key][d]

    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int D = a.D, ld = 3 * a.D;
    const T* base = reinterpret_cast<const T*>(a.qkv) + size_t(b) * kSquares * ld;

    // stage K and V: 2 x 64 rows x 8 pieces of 4 channels
    for (int i = tid; i < 2 * 64 * 8; i += 256) {
        const int m = i >> 9, r = (i >> 3) & 63, v = i & 7;
        float f[4];
        load4<T>(base + size_t(r) * ld + (1 + m) * D + h * kHeadDim + v * 4, f);
        store4<T>(&kv[m][r * KP + v * 4], f);
    }
    // this wave's query rows as the B operand of S^T = K Q^T: query 16 wave + l15, channels lg * 8 + j
    float q[8];
    load8<T>(base + size_t(16 * wave + l15) * ld + h * kHeadDim + lg * 8, q);
    __syncthreads();

    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float k[8];
        load8<T>(&kv[0][(16 * t + l15) * KP + lg * 8], k);
        s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        mma32<MODE>(k, q, s[t]);                                   // s[t][r] = S^T[key 16 t + 4 lg + r][query 16 wave + l15]
    }

    // softmax over the query's 64 keys: 16 in this lane, the rest in lanes l15 + 16, + 32, + 48
    float e[4][4];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            e[t][r] = s[t][r] * kScale;
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

    // O^T = V^T S^T: k-step ks covers the key tiles 2 ks and 2 ks + 1; element j <-> key 16 (2 ks + j / 4) + 4 lg + j % 4
    f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        float p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = e[2 * ks + j / 4][j % 4] / sum;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = to_f(kv[1][(16 * (2 * ks + j / 4) + 4 * lg + j % 4) * KP + dt * 16 + l15]);
            mma32<MODE>(v, p, o[dt]);                              // o[dt][r] = O[query 16 wave + l15][d = dt * 16 + 4 lg + r]
        }
    }
    T* out = reinterpret_cast<T*>(a.out) + (size_t(b) * kSquares + 16 * wave + l15) * D + h * kHeadDim;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        float v[4] = {o[dt][0], o[dt][1], o[dt][2], o[dt][3]};
        store4<T>(out + dt * 16 + 4 * lg, v);
    }
}

void launch_attention(const AttentionArgs& a, hipStream_t s) {
    if (a.D <= 0 || a.D % kHeadDim != 0) throw std::invalid_argument("attention_kernel: the width must be a positive multiple of 32 (head_dim 32)");
    const dim3 grid(a.D / kHeadDim, a.batch), block(256);
    if (a.mode == 0) hipLaunchKernelGGL(attention_kernel<0>, grid, block, 0, s, a);
    else if (a.mode == 1) hipLaunchKernelGGL(attention_kernel<1>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(attention_kernel<2>, grid, block, 0, s, a);
}

}  // namespace cra
